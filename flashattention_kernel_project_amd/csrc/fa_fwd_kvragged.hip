// fa_fwd_kvragged.hip -- a query count per sequence on KV-cache decode (fa_kvcache_decode with seqlens_q) against a 16-bit cache,
// contiguous and paged: the streams of fa_fwd_kvlogits.hip with the padded rows of each sequence cut to its own n_b, read on the
// device.  DESIGN.md section 7.10 has the reasoning; the kernels are the RaggedArgs<LogitArgs<WindowArgs<...>>> instantiations of
// fa_fwd_split_kernel.hpp, launched through fa_fwd_kvdecode.hpp.  The fp8 forms are in fa_fwd_kvragged_fp8.hip.  Also here, for both
// units: the merge that maps padded rows to the packed workspace rows and writes the dead ones.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvragged_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<RaggedArgs<LogitArgs<WindowArgs<CacheArgs>>>>(d, lg_page)
                    : dispatch_kvdecode<RaggedArgs<LogitArgs<WindowArgs<PagedArgs>>>>(d, lg_page);
}

// kvcache_combine over the PADDED output rows: the RaggedLse instantiations of the merge kernel.  The grid follows the host shape;
// which rows are live is decided on the device.
hipError_t kvragged_combine(const void* ws, void* O, float* lse, const float* sinks, const int* seqlens_q, int BH, int rows, int Hkv,
                            int Nq, int D, int S, int in_dtype, int out_dtype, hipStream_t stream)
{
    const long long out_rows = (long long)BH * rows;   // one wave per output row
    if (out_rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
        FA_LAUNCH((fa_split_combine_kernel<decltype(t), decltype(f32)::value, true, RaggedLse>), dim3((unsigned)out_rows), dim3(64), 0,
                  stream, static_cast<const float*>(ws), O, BH, rows, D, S, RaggedLse{lse, sinks, seqlens_q, Hkv, Nq});
        return launch_status();
    });
}

}  // namespace fa

// fa_fwd_kvlogits.hip -- attention sinks and soft-capped logits on KV-cache decode (fa_kvcache_decode) against a 16-bit cache,
// contiguous and paged: the streams of fa_fwd_kvwindow.hip with the two options of LogitArgs.  DESIGN.md section 7.9 has the
// reasoning; the kernels are the LogitArgs<WindowArgs<...>> instantiations of fa_fwd_split_kernel.hpp, launched through
// fa_fwd_kvdecode.hpp.  The fp8 forms are in fa_fwd_kvlogits_fp8.hip.  Also here, for both units: the merge that joins the sinks.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvlogits_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<LogitArgs<WindowArgs<CacheArgs>>>(d, lg_page)
                    : dispatch_kvdecode<LogitArgs<WindowArgs<PagedArgs>>>(d, lg_page);
}

// kvcache_combine with the sink of each row's query head joined to (M, L): the SinkLse instantiations of the merge kernel.
hipError_t kvlogits_combine(const void* ws, void* O, float* lse, const float* sinks, int BH, int rows, int Hkv, int Nq, int D, int S,
                            int in_dtype, int out_dtype, hipStream_t stream)
{
    const long long out_rows = (long long)BH * rows;   // one wave per output row
    if (out_rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
        FA_LAUNCH((fa_split_combine_kernel<decltype(t), decltype(f32)::value, true, SinkLse>), dim3((unsigned)out_rows), dim3(64), 0,
                  stream, static_cast<const float*>(ws), O, BH, rows, D, S, SinkLse{lse, sinks, Hkv, Nq});
        return launch_status();
    });
}

}  // namespace fa

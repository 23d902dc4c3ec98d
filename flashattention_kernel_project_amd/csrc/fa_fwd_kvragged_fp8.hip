// fa_fwd_kvragged_fp8.hip -- a query count per sequence on KV-cache decode (fa_kvcache_decode with seqlens_q) against an fp8 (OCP
// e4m3fn) cache, contiguous and paged: fa_fwd_kvragged.hip's row packing over the streams of fa_fwd_kvlogits_fp8.hip.  The kernels
// are the RaggedArgs<LogitArgs<WindowArgs<Fp8Args<...>>>> instantiations of fa_fwd_split_kernel.hpp, launched through
// fa_fwd_kvdecode.hpp; the merge is fa_fwd_kvragged.hip's.  DESIGN.md sections 7.4 and 7.10.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvragged_fp8_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<CacheArgs>>>>>(d, lg_page)
                    : dispatch_kvdecode<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<PagedArgs>>>>>(d, lg_page);
}

}  // namespace fa

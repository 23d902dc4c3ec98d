// fa_fwd_kvlogits_fp8.hip -- attention sinks and soft-capped logits on KV-cache decode (fa_kvcache_decode) against an fp8 (OCP
// e4m3fn) cache, contiguous and paged: fa_fwd_kvlogits.hip's options over the streams of fa_fwd_kvwindow_fp8.hip.  The kernels are
// the LogitArgs<WindowArgs<Fp8Args<...>>> instantiations of fa_fwd_split_kernel.hpp, launched through fa_fwd_kvdecode.hpp; the sinks
// are in natural-log units and take neither k_scale nor v_scale (their V row is zero).  DESIGN.md sections 7.4 and 7.9.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvlogits_fp8_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<LogitArgs<WindowArgs<Fp8Args<CacheArgs>>>>(d, lg_page)
                    : dispatch_kvdecode<LogitArgs<WindowArgs<Fp8Args<PagedArgs>>>>(d, lg_page);
}

}  // namespace fa

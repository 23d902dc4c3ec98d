// fa_fwd_kvwindow_fp8.hip -- sliding-window decode against an fp8 (OCP e4m3fn) KV cache, contiguous (fa_forward_kvcache_fp8_window)
// and paged (fa_forward_kvcache_paged_fp8_window): fa_fwd_kvwindow.hip's window over the streams of fa_fwd_kvfp8.hip.  The kernels
// are the WindowArgs<Fp8Args<...>> instantiations of fa_fwd_split_kernel.hpp, launched through fa_fwd_kvdecode.hpp; DESIGN.md
// sections 7.4 and 7.6.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvwindow_fp8_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<WindowArgs<Fp8Args<CacheArgs>>>(d, lg_page)
                    : dispatch_kvdecode<WindowArgs<Fp8Args<PagedArgs>>>(d, lg_page);
}

}  // namespace fa

// fa_fwd_kvwindow_fp8.hip -- sliding-window decode against an fp8 (OCP e4m3fn) KV cache, contiguous (fa_forward_kvcache_fp8_window)
// and paged (fa_forward_kvcache_paged_fp8_window): fa_fwd_kvwindow.hip's window over the streams of fa_fwd_kvfp8.hip.  Owns the
// fp8 kernels of level kWindow; DESIGN.md sections 7.4 and 7.6.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kWindow, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kWindow, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

// fa_fwd_kvpacked_fp8.hip -- token-packed (cu_seqlens) split-KV decode against an fp8 (OCP e4m3fn) cache, contiguous and paged
// (fa_kvcache_decode_varlen with FA_KV_FP8_E4M3): fa_fwd_kvpacked.hip's addressing over the streams of fa_fwd_kvragged_fp8.hip.  Owns
// the fp8 kernels of level kPacked; the checks are fa_fwd_kvpacked.hip's.  DESIGN.md sections 7.4 and 7.17.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kPacked, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kPacked, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

// fa_fwd_kvragged_fp8.hip -- a query count per sequence on KV-cache decode (fa_kvcache_decode with seqlens_q) against an fp8 (OCP
// e4m3fn) cache, contiguous and paged: fa_fwd_kvragged.hip's row packing over the streams of fa_fwd_kvlogits_fp8.hip.  Owns the
// fp8 kernels of level kRagged.  DESIGN.md sections 7.4 and 7.10.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kRagged, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kRagged, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

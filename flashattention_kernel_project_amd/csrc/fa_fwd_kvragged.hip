// fa_fwd_kvragged.hip -- a query count per sequence on KV-cache decode (fa_kvcache_decode with seqlens_q) against a 16-bit cache,
// contiguous and paged: the streams of fa_fwd_kvlogits.hip with the padded rows of each sequence cut to its own n_b, read on the
// device.  DESIGN.md section 7.10 has the reasoning.  Owns the 16-bit kernels of level kRagged; the fp8 forms are in
// fa_fwd_kvragged_fp8.hip.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kRagged, false, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kRagged, false, true>(const KvDecodeArgs&, int);

}  // namespace fa

// fa_fwd_kvfp8.hip -- decode against an fp8 (OCP e4m3fn) KV cache, contiguous (fa_forward_kvcache_fp8) and paged
// (fa_forward_kvcache_paged_fp8), with a dequantisation scale per K/V head.  K and V are widened to the query's 16-bit type while a
// tile is written to LDS, so the LDS images, the MFMAs, the softmax, the splits, the merge and the masks are those of
// fa_fwd_kvcache.hip / fa_fwd_kvpaged.hip; half the bytes cross HBM.  DESIGN.md section 7.4 has the reasoning.  Owns the plain fp8
// kernels.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

// Grid, split count and workspace are those of the 16-bit entry for the same shape.
template hipError_t kvdecode_unit<KvLevel::kPlain, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kPlain, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

// fa_fwd_kvlogits_fp8.hip -- attention sinks and soft-capped logits on KV-cache decode (fa_kvcache_decode) against an fp8 (OCP
// e4m3fn) cache, contiguous and paged: fa_fwd_kvlogits.hip's options over the streams of fa_fwd_kvwindow_fp8.hip.  Owns the fp8
// kernels of level kLogits; the sinks are in natural-log units and take neither k_scale nor v_scale (their V row is
// zero).  DESIGN.md sections 7.4 and 7.9.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kLogits, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kLogits, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

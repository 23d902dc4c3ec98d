// fa_fwd_kvlogits.hip -- attention sinks and soft-capped logits on KV-cache decode (fa_kvcache_decode) against a 16-bit cache,
// contiguous and paged: the streams of fa_fwd_kvwindow.hip with the two options of LogitArgs.  DESIGN.md section 7.9 has the
// reasoning.  Owns the 16-bit kernels of level kLogits; the fp8 forms are in fa_fwd_kvlogits_fp8.hip.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kLogits, false, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kLogits, false, true>(const KvDecodeArgs&, int);

}  // namespace fa

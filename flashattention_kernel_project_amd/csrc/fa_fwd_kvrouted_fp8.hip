// fa_fwd_kvrouted_fp8.hip -- the SHORT half of fa_kvcache_attend_varlen against an fp8 (OCP e4m3fn) cache, contiguous and paged.
// Owns the fp8 kernels of level kRouted; the hand-over is fa_fwd_kvrouted.hip's.  DESIGN.md sections 7.4 and 7.20.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kRouted, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kRouted, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

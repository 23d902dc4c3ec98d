// fa_fwd_kvtree_fp8.hip -- tree-mask token-packed split-KV decode against an fp8 (OCP e4m3fn) cache, contiguous and paged
// (fa_kvcache_decode_varlen_ex with a tree_mask and FA_KV_FP8_E4M3): fa_fwd_kvtree.hip's mask over the streams of
// fa_fwd_kvpacked_fp8.hip.  Owns the fp8 kernels of level kTree; the checks are fa_fwd_kvtree.hip's and
// fa_fwd_kvpacked.hip's.
// DESIGN.md sections 7.4 and 7.18.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kTree, true, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kTree, true, true>(const KvDecodeArgs&, int);

}  // namespace fa

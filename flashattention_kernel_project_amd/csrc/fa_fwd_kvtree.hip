// fa_fwd_kvtree.hip -- tree-mask token-packed split-KV decode against a 16-bit cache, contiguous and paged
// (fa_kvcache_decode_varlen_ex with a tree_mask): the streams of fa_fwd_kvpacked.hip with the causal triangle over the step's own
// tokens replaced by one 64-bit ancestor word per token row, read on the device.  DESIGN.md section 7.18 has the reasoning.
// Owns the 16-bit kernels of level kTree; the merge behind a split is level kPacked's, as it is.  The fp8 forms are
// in fa_fwd_kvtree_fp8.hip.  Also here, for both units: the options' checks.
#include "../../include/fa_mi355.h"
#include "fa_fwd_kvdecode.hpp"

namespace fa {

template hipError_t kvdecode_unit<KvLevel::kTree, false, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kTree, false, true>(const KvDecodeArgs&, int);

// No options, or no mask: fa_kvcache_decode_varlen's call, whatever else the descriptor holds.  The mask's own rules (causal == 1,
// max_q <= 64, 8-byte alignment) are kvpacked_dispatch's, next to the descriptor's.
hipError_t kvtree_dispatch(const fa_kvdecode_varlen_desc* desc, const fa_kvdecode_tree_opts* opts)
{
    if (opts && opts->size != sizeof(fa_kvdecode_tree_opts)) return hipErrorInvalidValue;
    return kvpacked_dispatch(desc, opts ? opts->tree_mask : nullptr);
}

}  // namespace fa

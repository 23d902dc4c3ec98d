// fa_fwd_varlen.hip -- fa_forward_varlen: prefill on token-packed Q, K, V (cu_seqlens), grouped-query heads, a causal mask
// aligned to the END of each sequence's keys, lse out.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md 7.12.
// The kernel template and the checks are fa_fwd_varlen_kernel.hpp's; this unit holds the 16 plain instantiations (T x d x out x
// causal).  The windowed / soft-capped / sink ones are fa_fwd_varlen_logits.hip's, so that neither set perturbs the other's code.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

hipError_t varlen_dispatch(const fa_varlen_desc* d)
{
    VarlenArgs a;
    dim3 grid;
    const hipError_t e = varlen_check(d, a, grid);
    if (e != hipSuccess) return e;
    return varlen_launch<false>(d, a, grid);
}

}  // namespace fa

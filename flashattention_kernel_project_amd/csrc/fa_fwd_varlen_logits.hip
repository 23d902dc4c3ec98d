// fa_fwd_varlen_logits.hip -- fa_forward_varlen_ex: the variable-length packed prefill with a sliding window, soft-capped logits
// and attention sinks.  The contract is include/fa_mi355.h's; the reasons are DESIGN.md 7.13.  The kernels are the 16 kLogits
// instantiations of fa_fwd_varlen_kernel.hpp (T x d x out x causal); the three options are runtime values inside them.
#include "fa_fwd_varlen_kernel.hpp"

namespace fa {

hipError_t varlen_logits_dispatch(const fa_varlen_desc* d, const fa_varlen_opts* o)
{
    if (!o) return varlen_dispatch(d);
    if (o->size != sizeof(fa_varlen_opts)) return hipErrorInvalidValue;
    if (o->window < 0) return hipErrorInvalidValue;
    if (!(o->softcap >= 0.0f) || isinf(o->softcap)) return hipErrorInvalidValue;   // negative, NaN or inf
    if (!o->sinks && o->window == 0 && o->softcap == 0.0f) return varlen_dispatch(d);   // all off: the base entry itself
    VarlenLogitArgs a;
    dim3 grid;
    const hipError_t e = varlen_check(d, static_cast<VarlenArgs&>(a), grid);
    if (e != hipSuccess) return e;
    a.sinks = o->sinks;
    // "no window" and every W that no sequence can feel run as total_q + total_k, which masks nothing (lo_i <= Lk_b - W <= 0) and
    // keeps the kernel's 32-bit limits from wrapping: the totals are below 2^26 each by the 32-bit offset check above
    const long long wmax = (long long)d->total_q + d->total_k;
    a.window = (int)(o->window == 0 || o->window > wmax ? wmax : o->window);
    a.cap2 = o->softcap * kLog2e;
    a.cap_rk = o->softcap > 0.0f ? 2.0f / o->softcap : 0.0f;
    return varlen_launch<true>(d, a, grid);
}

}  // namespace fa

// fa_fwd_kv256_fp8.hip -- the kernels of fa_kvcache_decode_d256_fp8: fa_fwd_kv256_kernel.hpp's template with kFp8, sixteen decode
// kernels (fp16 / bf16 Q x two output types x direct / partial x contiguous / paged: the last two inside kv256_launch) and four merge
// kernels.  A K or V row is 256 e4m3fn codes under the head's device-side scale; the codes are widened exactly to Q's type on their
// way into LDS.  The checks and the plan are fa_fwd_kv256.hip's.  DESIGN.md section 7.27, profiles/kv256_fp8.txt.
#include "fa_fwd_kv256_kernel.hpp"

namespace fa {

hipError_t kv256_launch_fp8(const kv256::Dev& a, bool bf16, bool f32, bool paged, hipStream_t stream)
{
    if (bf16) return f32 ? kv256_launch<BF16, true, true>(a, paged, stream) : kv256_launch<BF16, false, true>(a, paged, stream);
    return f32 ? kv256_launch<F16, true, true>(a, paged, stream) : kv256_launch<F16, false, true>(a, paged, stream);
}

}  // namespace fa

// fa_fwd_varlen256_fp8.hip -- the kernels of fa_forward_varlen_kvcache_d256_fp8: fa_fwd_varlen256_kernel.hpp's template with kFp8,
// eight kernels (fp16 / bf16 Q x two output types x contiguous / paged; there is no packed e4m3fn source).  A K or V row is 256
// e4m3fn codes under the head's device-side scale; the codes are widened exactly to Q's type on their way into LDS.  The checks are
// fa_fwd_varlen256.hip's.  DESIGN.md section 7.28, profiles/varlen_d256_fp8.txt.
#include "fa_fwd_varlen256_kernel.hpp"

namespace fa {

hipError_t varlen256_launch_fp8(const varlen256::Dev& a, dim3 grid, int in_dtype, int out_dtype, bool paged, void* stream)
{
    return paged ? varlen256_launch<varlen256::kPaged, true>(a, grid, in_dtype, out_dtype, stream)
                 : varlen256_launch<varlen256::kContig, true>(a, grid, in_dtype, out_dtype, stream);
}

}  // namespace fa

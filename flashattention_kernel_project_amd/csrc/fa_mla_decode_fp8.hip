// fa_mla_decode_fp8.hip -- the kernels of fa_mla_decode_fp8: fa_mla_decode_kernel.hpp's template with kFp8, sixteen decode kernels
// (fp16 / bf16 Q x two output types x direct / partial x contiguous / paged: the last two inside mla_launch) and four merge kernels.
// A latent row is 576 e4m3fn codes under one device-side scale; the codes are widened exactly to Q's type on their way into LDS.
// The checks and the plan are fa_mla_decode.hip's.  DESIGN.md section 7.24, profiles/mla_decode_fp8.txt.
#include "fa_mla_decode_kernel.hpp"

namespace fa {

hipError_t mla_launch_fp8(const mla::Dev& a, bool bf16, bool f32, bool paged, hipStream_t stream)
{
    return mla_launch_typed<true>(a, bf16, f32, paged, stream);
}

}  // namespace fa

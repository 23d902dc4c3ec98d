// fa_kvcache_append_varlen256.hip -- fa_kvcache_append_varlen_d256: the packed append at head dimension 256, the write half of
// fa_kvcache_decode_d256 and fa_kvcache_decode_d256_fp8.  fa_kvcache_append_varlen_kernel.hpp's kernel template at D = 256 -- a row
// is 32 chunks of 16 bytes, 512 bytes in a 16-bit cache and 256 in an e4m3fn one -- in all eight forms, with and without positions,
// behind the same checks with d == 256 and the capacity bound of the d = 256 decode.  The older entries keep refusing d = 256.
// DESIGN.md section 7.27.
#include "fa_kvcache_append_varlen_kernel.hpp"

namespace fa {

hipError_t kvcache_append_varlen_d256(const ::fa_kvappend_varlen_desc* d, const ::fa_kvappend_varlen_opts* opts)
{
    if (opts && opts->size != sizeof(fa_kvappend_varlen_opts)) return hipErrorInvalidValue;
    return append_varlen_checked<true>(d, opts ? opts->positions : nullptr);
}

}  // namespace fa

// fa_kvcache_append_varlen.hip -- fa_kvcache_append_varlen and fa_kvcache_append_varlen_ex: the append of a token-packed batch at
// d in {64, 128}.  The kernel template, the checks and the launches are fa_kvcache_append_varlen_kernel.hpp's; this unit instantiates
// them for rows of 8 and 16 chunks.  DESIGN.md section 7.16.
#include "fa_kvcache_append_varlen_kernel.hpp"

namespace fa {

hipError_t kvcache_append_varlen(const ::fa_kvappend_varlen_desc* d) { return append_varlen_checked<false>(d, nullptr); }

hipError_t kvcache_append_varlen_ex(const ::fa_kvappend_varlen_desc* d, const ::fa_kvappend_varlen_opts* opts)
{
    if (opts && opts->size != sizeof(fa_kvappend_varlen_opts)) return hipErrorInvalidValue;
    return append_varlen_checked<false>(d, opts ? opts->positions : nullptr);
}

}  // namespace fa

// fa_fwd_kvrouted_fp8.hip -- the SHORT half of fa_kvcache_attend_varlen against an fp8 (OCP e4m3fn) cache, contiguous and paged: the
// RoutedArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<...>>>>>> instantiations of fa_fwd_split_kernel.hpp, launched through
// fa_fwd_kvdecode.hpp; the hand-over and the merge are fa_fwd_kvrouted.hip's.  DESIGN.md sections 7.4 and 7.20.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvrouted_fp8_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<RoutedArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<CacheArgs>>>>>>>(d, lg_page)
                    : dispatch_kvdecode<RoutedArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<PagedArgs>>>>>>>(d, lg_page);
}

}  // namespace fa

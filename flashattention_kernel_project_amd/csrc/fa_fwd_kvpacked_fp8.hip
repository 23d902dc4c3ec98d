// fa_fwd_kvpacked_fp8.hip -- token-packed (cu_seqlens) split-KV decode against an fp8 (OCP e4m3fn) cache, contiguous and paged
// (fa_kvcache_decode_varlen with FA_KV_FP8_E4M3): fa_fwd_kvpacked.hip's addressing over the streams of fa_fwd_kvragged_fp8.hip.  The
// kernels are the PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<...>>>>> instantiations of fa_fwd_split_kernel.hpp, launched
// through fa_fwd_kvdecode.hpp; the checks and the merge are fa_fwd_kvpacked.hip's.  DESIGN.md sections 7.4 and 7.17.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvpacked_fp8_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<CacheArgs>>>>>>(d, lg_page)
                    : dispatch_kvdecode<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<PagedArgs>>>>>>(d, lg_page);
}

}  // namespace fa

// fa_fwd_kvtree_fp8.hip -- tree-mask token-packed split-KV decode against an fp8 (OCP e4m3fn) cache, contiguous and paged
// (fa_kvcache_decode_varlen_ex with a tree_mask and FA_KV_FP8_E4M3): fa_fwd_kvtree.hip's mask over the streams of
// fa_fwd_kvpacked_fp8.hip.  The kernels are the TreeArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<...>>>>>> instantiations
// of fa_fwd_split_kernel.hpp, launched through fa_fwd_kvdecode.hpp; the checks are fa_fwd_kvtree.hip's and fa_fwd_kvpacked.hip's.
// DESIGN.md sections 7.4 and 7.18.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

hipError_t kvtree_fp8_decode(const KvDecodeArgs& d, int lg_page)
{
    return !d.paged ? dispatch_kvdecode<TreeArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<CacheArgs>>>>>>>(d, lg_page)
                    : dispatch_kvdecode<TreeArgs<PackedArgs<RaggedArgs<LogitArgs<WindowArgs<Fp8Args<PagedArgs>>>>>>>(d, lg_page);
}

}  // namespace fa

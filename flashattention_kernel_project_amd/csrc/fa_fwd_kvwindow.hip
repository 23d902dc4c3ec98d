// fa_fwd_kvwindow.hip -- sliding-window decode against a 16-bit KV cache, contiguous (fa_forward_kvcache_window) and paged
// (fa_forward_kvcache_paged_window): the streams of fa_fwd_kvcache.hip / fa_fwd_kvpaged.hip with a lower key limit per row and a
// first tile per sequence.  DESIGN.md section 7.6 has the reasoning.  Owns the 16-bit kernels of level kWindow; the
// fp8 forms are in fa_fwd_kvwindow_fp8.hip.  Also here: the window's span and the two windowed sizing functions.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

// The longest key range one sequence can stream under a window, in keys: the window of the last row plus the Nq - 1 keys the rows
// before it add, rounded up to tiles, plus one tile because the range starts inside a tile; never more than the capacity.
int window_span_cap(int Nq, int Ncap, int window)
{
    const long long need = (long long)window + Nq - 1;
    if (need >= Ncap) return Ncap;
    const long long span = (need + kBlockN - 1) / kBlockN * kBlockN + kBlockN;
    return span < Ncap ? (int)span : Ncap;
}

size_t kvwindow_workspace_bytes(int B, int Hkv, int G, int Nq, int Ncap, int D, int window)
{
    if (window < 0) return 0;
    // the un-windowed sizing on the longest range a sequence can stream, which is positive exactly when the capacity is
    return kvcache_workspace_bytes(B, Hkv, G, Nq, window == 0 ? Ncap : window_span_cap(Nq, Ncap, window), D);
}

size_t kvpaged_window_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int D, int window)
{
    // 0 for the (max_pages, page_size) the paged entries reject, as in kvpaged_workspace_bytes
    if (max_pages <= 0 || page_log2(page_size) < 0 || (long long)max_pages * page_size > 0x7FFFFFFFll) return 0;
    return kvwindow_workspace_bytes(B, Hkv, G, Nq, max_pages * page_size, D, window);
}

// The split count follows from window_span_cap, not from the capacity; grid and workspace follow from it.
template hipError_t kvdecode_unit<KvLevel::kWindow, false, false>(const KvDecodeArgs&, int);
template hipError_t kvdecode_unit<KvLevel::kWindow, false, true>(const KvDecodeArgs&, int);

}  // namespace fa

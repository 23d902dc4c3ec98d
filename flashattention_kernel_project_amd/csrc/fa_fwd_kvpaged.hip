// fa_fwd_kvpaged.hip -- decode against a paged KV cache (fa_forward_kvcache_paged): the KV-cache stream of fa_fwd_kvcache.hip with
// every tile's rows taken from pages of a pool through a block table that is read on the device.  DESIGN.md section 7.2 has the
// reasoning.  Owns the plain 16-bit paged kernels.  Also here: the page-geometry checks every paged entry (decode
// and append) shares.
#include "fa_fwd_kvdecode.hpp"

namespace fa {

// log2 of a page size the kernel takes (a power of two, at least 16 keys), else -1
int page_log2(int page_size)
{
    if (page_size < 16 || (page_size & (page_size - 1)) != 0) return -1;
    int lg = 4;
    while ((1 << lg) != page_size) ++lg;
    return lg;
}

size_t kvpaged_workspace_bytes(int B, int Hkv, int G, int Nq, int max_pages, int page_size, int D)
{
    if (max_pages <= 0 || page_log2(page_size) < 0 || (long long)max_pages * page_size > 0x7FFFFFFFll) return 0;
    return kvcache_workspace_bytes(B, Hkv, G, Nq, max_pages * page_size, D);
}

// What the paged entries (the fp8 and windowed ones too) reject before the device is touched.  On success q is p with the capacity
// filled in and lg_page the log2 of the page size.
hipError_t kvpaged_check(const KvPagedArgs& p, KvPagedArgs& q, int& lg_page)
{
    lg_page = page_log2(p.page_size);
    if (!p.table || lg_page < 0 || p.num_pages <= 0 || p.max_pages <= 0) return hipErrorInvalidValue;
    if ((long long)p.max_pages * p.page_size > 0x7FFFFFFFll) return hipErrorInvalidValue;   // the capacity is an int
    q = p;
    q.c.Ncap = p.max_pages * p.page_size;
    // from here on the checks of kvcache_check, on that capacity.  Its bound on the byte offsets covers what is 32 bit in the
    // kernel here: a tile's byte offset before it is reduced to the page (hence the page-head block too)
    return kvcache_check(q.c);
}

template hipError_t kvdecode_unit<KvLevel::kPlain, false, true>(const KvDecodeArgs&, int);

}  // namespace fa

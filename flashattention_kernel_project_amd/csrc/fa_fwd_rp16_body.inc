// fa_fwd_rp16_body.inc -- the body of the rolling half-tile pipeline's kernel; fa_fwd_rp16_kernel.hpp, which documents it, includes
// it twice.  FA_RP16_DEVICE_BODY = 0: as the body of the __global__ function itself, for every family WITHOUT the in-launch
// running-max pass -- statement for statement the kernel as it was before that pass existed, so that those families' device code does
// not change (wrapped into a device function the same statements get another register allocation).  FA_RP16_DEVICE_BODY = 1:
// as the body of rp16_body<..., kInLaunch = true>, the device function the in-launch families' kernel wrapper calls.
    using namespace rp16;
    constexpr int kW = kWv;   // (hides rp16::kW, the default)
    static_assert(kWv == 8 || (kWv == 4 && !kDma && !kScan), "waves per (key-split group of a) workgroup: 8 or 4");
    static_assert(kKeySplit == 1 || (kKeySplit == 2 && ((kWv == 8 && X == 1) || (kWv == 4 && X == 2)) && D == 64 && !kDma && !kCausal && !kScan),
                  "key split: 128-row workgroups at D = 64 (2 x 8 waves of 16 rows, or 2 x 4 waves of 32 rows)");
    using M = Mx<T>;
    using G = TileGeom<D>;
    // The folded pass multiplies Q'.K on the fp16 matrix instruction whatever the input type: Q' = fp16(Q * scale * log2 e)
    // (bf16's 8 bits would move a logit by |logit| * 2^-8), and bf16 K is converted to fp16 while it is staged -- exact for
    // every bf16 value up to 65504 in magnitude (larger ones raise the gate; smaller ones lose at most 2^-25 absolutely).
    // P and V stay in the input type for O^T += V^T.P^T.
    constexpr bool kCvtK = kFold && T::id == 1;
    static_assert(!kScan || (!kFold && !kDma), "the redo kernel runs the running-max pass only");
    // full-width waves (64 rows at D = 64, 32 at D = 128): the running-max pass lives in a kScan body -- in this launch (kAppend
    // below) or in the redo kernel behind it (fa_fwd_rp16_kernel.hpp, kScan)
    constexpr bool kSplitTrack = !kScan && !kDma && 16 * X * (D / 64) >= 64;
    constexpr unsigned kMarker = 0x7FA5C0DEu;
#if !FA_RP16_DEVICE_BODY   // (the kernel-body form has no such template parameter)
    constexpr bool kInLaunch = false;
#endif
    constexpr bool kAppend = kSplitTrack && kInLaunch;   // refused blocks go onto the list in LDS ...
    constexpr bool kTail = kScan && kInLaunch;           // ... and this body computes the listed blocks
    static_assert(!kInLaunch || ((kAppend || kTail) && kWv == 8 && kKeySplit == 1), "the in-launch tail: full-width eight-wave families");
    // a vector pair-step is spread over its matrix slots (one v_exp behind each of the first two, the v_cvt_pk behind the second /
    // third) instead of all behind the last (DESIGN.md 3.6 (4)); under the mask the pins cost the two-wave full-width kernels spills
    constexpr bool kVSplit = !kCausal || (kWv == 4 && kKeySplit == 1);
    static_assert(!(kCvtK && kDma), "the DMA path cannot convert K on the way");
    static_assert(!kDma || D == 64, "the DMA piece maps are written for 128-byte rows");
    constexpr int kRows = 16 * X * kW;
    constexpr int kKS = D / 32, kDB = D / 16;   // k-steps of QK^T, 16-row blocks of O^T
    constexpr int kNF = 2 * kKS + kDB;          // fragments per step (K and V^T alternate: 2 kKS == kDB)
    // fragment registers and read-ahead: a fragment feeds X matrix instructions, so the narrow waves (X < 4 at D = 64: small
    // grids) need more of them in flight to cover the LDS latency.  (32-row waves at D = 128 count as wide although a fragment
    // there feeds two matrix instructions only: the ring of eight, read four ahead, measured -0.5 %, inside that A/B's noise -- DESIGN.md 3.6 (7)(a))
    constexpr bool kWide = 16 * X * (D / 64) >= 64;
    constexpr int kRing = kWide ? 4 : 8;
    constexpr int kAhead = kWide ? kAheadWide : (X == 2 ? 4 : 6);
    constexpr int kSlots = kNF * X;             // matrix instructions per step (32 for the 64-row waves: X = 4 at D = 64, 2 at D = 128)
    static_assert(2 * kKS == kDB && kNF % kRing == 0 && kSlots % (4 * X) == 0, "fragment ring / vector pair-steps divide a step");
    constexpr int kLoads = (kBlockN * G::kChunks) / (64 * kW);   // 16-B chunks of K (and of V) per thread and tile
    // LDS instructions a wave issues in the second step behind the landing of tile j+2 (fragment reads: one ds_read_b128 per K
    // fragment, two ds_read_b64_tr_b16 per V^T fragment)
    constexpr int kLandSlot = kStageSlot * kSlots / 32;
    // one wave per SIMD: no second wave issues while this one works through a bunch of loads or LDS writes, so tile j+2 is
    // requested one chunk per matrix slot (first step) and landed one chunk per slot (second step, from kLandSlot on)
    // (DESIGN.md 3.6 (7), "issue slots")
    constexpr bool kOneWave = kWv == 4 && kKeySplit == 1;   // one wave per SIMD
    constexpr bool kSpread = kOneWave && !kDma;
    constexpr int kLandLast = kSpread ? kLandSlot + 2 * kLoads - 1 : kLandSlot;   // the slot of the last landing write
    // ... and the tile barrier is replaced by one flag word per wave behind the ring: a wave publishes "tile j+2 landed" (its
    // iteration count) right behind its last landing write and looks at all four flags only in front of its first read of that
    // tile, most of a step later -- LDS operations of a wave complete in order, so the flag follows the data and the reads
    // follow the look.  A lone wave per SIMD that waits at s_barrier for the slowest of four idles its matrix pipe; here the
    // waves may drift by most of a step.  (Ring reuse: a wave lands tile j+3 over tile j-1 only behind its look of iteration
    // j+1, i.e. when every wave has landed tile j+2 -- 16 slots into the second step of iteration j, past its last read of
    // tile j-1 in the first.)  The two-wave kernels keep s_barrier: it holds the two waves of a SIMD in the phase the slot
    // placement assumes, and flags lost there (DESIGN.md 3.6 (7), "No s_barrier").
    constexpr bool kFlagBar = kSpread && (FA_RP16_ABL & 24) == 0;
    constexpr int kFlagCheck = (kNF - kAhead) * X + X - 2, kFlagRead = kFlagCheck >= 8 ? kFlagCheck - 8 : 0;   // the slot in front of the first read-ahead into the next step
    static_assert(!kFlagBar || (kFlagRead >= 0 && kFlagRead < kFlagCheck && kLandLast + 1 < kSlots), "flag slots");
    static_assert(kLandLast < kSlots && 2 * kLoads <= kSlots, "the landing fits the step");
    constexpr int kLdsAfterLand = [] {
        int n = 0;
        for (int i = kLandLast; i < kSlots; ++i)
            if (i % X == X - 1) n += ((i / X + kAhead) & 1) ? 2 : 1;
        return n;
    }();
    constexpr unsigned kRowB = D * 2;
    constexpr unsigned kTile = kBlockN * D * 2;
    constexpr unsigned kSlotBytes = 2 * kTile;      // [K tile][V tile]
    constexpr bool kPair = pair_tiles(D, X, kDma) && kKeySplit == 1 && kWv == 8;   // (two rings of eight slots do not fit; one-wave kernels land per slot and use flags)
    // one wave per SIMD: QK^T spelled out with the scores in architectural registers (Mx::mfma_v*).  Every vector read of a score
    // lies at least X P.V matrix instructions behind the instruction that wrote it (the units alternate QK^T and P.V fragments and a
    // step ends with a P.V fragment); the prologue, whose reference maximum reads unit 0 at once, waits explicitly (settle).
    // (With the builtin the scores land in the accumulator half and cost a v_accvgpr_read each: 5 % slower, DESIGN.md 3.6 (7).)
    constexpr bool kAsmQK = kOneWave;   // (the key-split kernel has four waves per GROUP: two per SIMD, builtins)
    constexpr unsigned kRingSlots = kPair ? 8u : 4u, kRingMask = kRingSlots - 1u;
    constexpr int kLook = kPair ? 3 : 2;            // a tile is landed this many tiles ahead of the iteration that starts with it
    extern __shared__ __attribute__((aligned(16))) char smem_all[];   // one ring of slots per key-split group
#if FA_RP16_DEVICE_BODY   // (only in the device-function form; the kernel-body form must stay statement for statement what it was, see the top)
    // kInLaunch: the list both bodies share, behind the larger ring (the half-width body's)
    constexpr unsigned kListOff = tail_list_off(D, kTail ? X : X / 2);
    static_assert(!kInLaunch || kListOff >= kRingSlots * kSlotBytes, "the list lies behind this body's ring");
    static_assert(!kTail || kListOff == kRingSlots * kSlotBytes, "the half-width body's ring is the one tail_list_off() measures");
    [[maybe_unused]] unsigned* const tail_list = reinterpret_cast<unsigned*>(smem_all + kListOff);
#endif
    const unsigned grp = kKeySplit == 1 ? 0u : (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x / (64u * kW));
    char* const smem = smem_all + grp * (kRingSlots * kSlotBytes);
#if FA_RP16_DEVICE_BODY
    // (kTail: the thread id through an opaque copy, so that this body's lane constants are formed when it is entered -- hoisted to
    // the top of the kernel they are spilled across the full-width body, whose stream has no register to spare)
    unsigned tid_raw = threadIdx.x;
    if constexpr (kTail) asm volatile("" : "+v"(tid_raw));
    const unsigned tid  = kKeySplit == 1 ? tid_raw : tid_raw % (64u * kW);   // within the group
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
    const unsigned tid  = kKeySplit == 1 ? threadIdx.x : threadIdx.x % (64u * kW);   // within the group
#endif
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane = tid & 63u;
    const unsigned c16 = lane & 15u, g = lane >> 4;
    const float c = fabsf(scale_log2e);
    const unsigned q_flip = scale_log2e < 0.0f ? 0x80008000u : 0u;
    const int Nkv = N / kKeySplit;                       // keys of this group (the host checked the divisibility)
    const size_t kv_first = (size_t)grp * Nkv * D;       // its first K / V element inside a head
    const unsigned kv_bytes = (unsigned)((size_t)Nkv * D * 2);
    const int ntiles = (Nkv + kBlockN - 1) / kBlockN;
    const bool partial = (Nkv % kBlockN) != 0;

    unsigned st_goff[kLoads], sv_goff[kLoads], k_lds[kLoads], v_lds[kLoads];
#pragma unroll
    for (int p = 0; p < kLoads; ++p) {
        const unsigned idx = tid + p * 64u * kW;
        const unsigned srow = idx / G::kChunks, sch = idx % G::kChunks;
        st_goff[p] = srow * kRowB + sch * 16u;
        k_lds[p] = G::k_off(srow, sch);
        // V: the eight lanes of a ds_write_b128 group take 4 keys x 2 chunks of one head-dim block (128 contiguous bytes of the
        // image) instead of one key's 8 chunks (8 slots 256 B apart: 4-way on the 128-B bank row of a write; DESIGN.md 3.6 (3))
        constexpr unsigned ndb = G::kChunks / 2, rpw = 64u / G::kChunks;   // head-dim blocks; key rows per wave-instruction
        const unsigned w = idx >> 6, l = idx & 63u, t = l >> 3;
        const unsigned vrow = w * rpw + 4u * (t / ndb) + ((l >> 1) & 3u), vch = 2u * (t % ndb) + (l & 1u);
        sv_goff[p] = vrow * kRowB + vch * 16u;
        v_lds[p] = kTile + ((vrow >> 3) * (unsigned)kDB + (vch >> 1)) * 256u + ((vrow & 7u) << 5) + ((vch & 1u) << 4);
    }
    // LDS-DMA: this wave's 1-KB piece of an image is bytes [1024 wave, +1024), lane l lands at +16 l; where that comes from
    const unsigned dk_row = 8u * wave + (lane >> 3), dk_slot = lane & 7u;
    const unsigned k_src = dk_row * kRowB + ((dk_slot ^ G::k_swz(dk_row)) << 4);
    const unsigned dv_l = 1024u * wave + 16u * lane, dv_blk = dv_l >> 8;
    const unsigned dv_row = (dv_blk / (unsigned)kDB) * 8u + ((dv_l & 255u) >> 5), dv_ch = (dv_blk % (unsigned)kDB) * 2u + ((dv_l >> 4) & 1u);
    const unsigned v_src = dv_row * kRowB + dv_ch * 16u;
    typedef __attribute__((address_space(3))) void lds_void;
    auto dma_tile = [&](__amdgpu_buffer_rsrc_t rks, __amdgpu_buffer_rsrc_t rvs, unsigned tile_off, unsigned slot_off) __attribute__((always_inline)) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rks, (lds_void*)(smem + slot_off + 1024u * wave), 16, tile_off + k_src, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rvs, (lds_void*)(smem + slot_off + kTile + 1024u * wave), 16, tile_off + v_src, 0, 0, 0);
    };
    unsigned k_rd[kKS];
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) k_rd[ks] = c16 * kRowB + (((4u * ks + g) ^ G::k_swz(c16)) << 4);
    // (four equal elements, of which [0] is read.  As a scalar or a one-element array the same matrix instructions get another
    // register allocation, i.e. a kernel nobody has timed: the array stays until somebody does)
    unsigned v_rd4[4];
#pragma unroll
    for (unsigned dq = 0; dq < 4u; ++dq)
        v_rd4[dq] = kTile + (g >> 1) * (unsigned)kDB * 256u + ((4u * (g & 1u) + (c16 >> 2)) << 5) + (c16 & 3u) * 8u;

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const u32x4 zero4u = {0u, 0u, 0u, 0u};
    const std::true_type yes{};
    const std::false_type no{};
    using c0 = std::integral_constant<int, 0>;
    using c1 = std::integral_constant<int, 1>;
    // v of the lane `sh` places further round the lane's row of 16 (DPP row_ror: no LDS round trip like ds_bpermute); four
    // doubling steps (1, 2, 4, 8) leave the row's maximum / sum in every lane
    auto row_ror = [&](float v, int sh) -> float {
        const int iv = __builtin_bit_cast(int, v);
        int r;
        switch (sh) {
            case 1: r = __builtin_amdgcn_update_dpp(0, iv, 0x121, 0xF, 0xF, true); break;
            case 2: r = __builtin_amdgcn_update_dpp(0, iv, 0x122, 0xF, 0xF, true); break;
            case 4: r = __builtin_amdgcn_update_dpp(0, iv, 0x124, 0xF, 0xF, true); break;
            default: r = __builtin_amdgcn_update_dpp(0, iv, 0x128, 0xF, 0xF, true); break;
        }
        return __builtin_bit_cast(float, r);
    };
    auto across_max = [&](float v) -> float {   // over the four lanes that share a query row
        v = fmaxf(v, __shfl_xor(v, 16, 64));
        return fmaxf(v, __shfl_xor(v, 32, 64));
    };
    auto across_sum = [&](float v) -> float {
        v += __shfl_xor(v, 16, 64);
        return v + __shfl_xor(v, 32, 64);
    };

#if FA_RP16_DEVICE_BODY
    const unsigned nwg = kTail ? 2u * n_listed : total_wg;   // kTail: items are the half-blocks of the listed entries, in order
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
    const unsigned nwg = total_wg;
#endif
    // work item -> (head, query block): XCD-aware remap of the persistent grid's item index
    // (tests/test_gpu_single_launch.py::owners is a copy of this map: change both)
    auto locate = [&](unsigned bid_, unsigned& bh_, unsigned& qb_) __attribute__((always_inline)) {
        const unsigned xq = nwg >> 3, xr = nwg & 7u, xcd = bid_ & 7u;
        const unsigned wgid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid_ >> 3);
        bh_ = wgid / (unsigned)nqb;
        const unsigned qbi = wgid - bh_ * (unsigned)nqb;
        qb_ = qbi;
        if constexpr (kCausal) {
            // Alternate the direction of the query blocks from one round of the persistent grid to the next, so that a CU's
            // items add up to about the same number of tiles.  The direction must be a function of the HEAD alone (all its
            // query blocks flip together, else two items would compute the same block): take the round of the head's first
            // item, found through the inverse of the XCD remap above.
            const unsigned t0 = bh_ * (unsigned)nqb, big = xr * (xq + 1u);
            const unsigned x0 = t0 < big ? t0 / (xq + 1u) : xr + (t0 - big) / (xq ? xq : 1u);
            const unsigned start0 = x0 < xr ? x0 * (xq + 1u) : big + (x0 - xr) * xq;
            const unsigned bid0 = 8u * (t0 - start0) + x0;
            if (((bid0 / gridDim.x) & 1u) == 0u) qb_ = (unsigned)nqb - 1u - qbi;
        }
    };
#if FA_RP16_DEVICE_BODY
    // item -> (head, row block of THIS body's width).  kTail: read from the list (no remap: the entry is resolved already)
    auto item_of = [&](unsigned it, unsigned& bh_, unsigned& qb_) __attribute__((always_inline)) {
        if constexpr (kTail) {
            bh_ = (unsigned)__builtin_amdgcn_readfirstlane(tail_list[2u * (it >> 1)]);
            qb_ = (unsigned)__builtin_amdgcn_readfirstlane(tail_list[2u * (it >> 1) + 1u]) / (unsigned)kRows + (it & 1u);
        } else {
            locate(it, bh_, qb_);
        }
    };
    // kTail: the first half-block at or behind `it` that has rows (only an entry's second half can lie behind the sequence)
    auto tail_from = [&](unsigned it) __attribute__((always_inline)) -> unsigned {
        if ((it & 1u) != 0u && it < nwg &&
            (unsigned)__builtin_amdgcn_readfirstlane(tail_list[2u * (it >> 1) + 1u]) + (unsigned)kRows >= (unsigned)N) ++it;
        return it;
    };
#define FA_RP16_ITEM_OF item_of
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
#define FA_RP16_ITEM_OF locate
#endif
    const size_t head_elems = (size_t)N * D;
    const unsigned head_bytes = (unsigned)(head_elems * 2);
    // Between two items of the persistent loop everything is a latency chain (stamps: Q 2.8-4.4 us, then K/V 2.2, reference
    // 2.2, gates 1.8, stores 1.6 of ~116 us per item at B8 H16 N4096).  kPrefetch: the NEXT item's Q rows are requested
    // (raw, into qf -- dead by then) as soon as the first pass' tile loop is over, i.e. ahead of this item's stores in the
    // in-order vector memory queue, and every item requests its first three K/V tiles before it waits for its Q.  (The K/V
    // tiles are not carried across the boundary as well: the allocator spills them, DESIGN.md 3.2.)
    constexpr bool kPrefetch = !kDma;
    u32x4 qf[X][kKS];   // B operand of QK^T: Q[row of block x][32 ks + 8 g .. +7]
    u32x4 kst[kLoads], vst[kLoads];
    u32x4 kst2[kLoads], vst2[kLoads];   // kPair: the second tile of an iteration
    u32x4 pfk[2][kLoads], pfv[2][kLoads];
    // hb: the head's Q; row_base: the wave's first row (wave-uniform, folded into the descriptor: the bounds check -- rows past
    // N read zeros -- covers the per-lane and the immediate offset only).  One per-lane address, recomputed here from the lane
    // id so that nothing of it lives across the tile loop.
    auto q_issue = [&](const uint16_t* hb, unsigned row_base) __attribute__((always_inline)) {
        unsigned l = lane;
        asm volatile("" : "+v"(l));
        const unsigned voff = (l & 15u) * kRowB + (l >> 4) * 16u;
        const unsigned rb = __builtin_amdgcn_readfirstlane(row_base);
        const unsigned skip = rb * kRowB;
        // (the pointer is wave-uniform by construction; saying so spares the descriptor a waterfall loop per load)
        const unsigned long long pa = (unsigned long long)(hb + (size_t)rb * D);
        const unsigned p_lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)pa);   // (the builtin returns int: no sign
        const unsigned p_hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(pa >> 32));   // extension into the high half)
        const unsigned long long pu = (unsigned long long)p_lo | ((unsigned long long)p_hi << 32);
        const __amdgpu_buffer_rsrc_t rq_ = make_rsrc(reinterpret_cast<const uint16_t*>(pu),
                                                     __builtin_amdgcn_readfirstlane(skip < head_bytes ? head_bytes - skip : 0u));
#pragma unroll
        for (int x = 0; x < X; ++x)
#pragma unroll
            for (int ks = 0; ks < kKS; ++ks) {
                if constexpr ((FA_RP16_ABL & 64) != 0) qf[x][ks] = zero4u;
                else qf[x][ks] = buf_load16(rq_, voff + ((16u * x) * kRowB + 64u * ks));
            }
    };
    auto kv_issue = [&](__amdgpu_buffer_rsrc_t rk_, __amdgpu_buffer_rsrc_t rv_) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < kLoads; ++p) {   // all loads of the three tiles in flight together
            if constexpr ((FA_RP16_ABL & 128) != 0) {
                pfk[0][p] = pfv[0][p] = pfk[1][p] = pfv[1][p] = kst[p] = vst[p] = zero4u;
                continue;
            }
            pfk[0][p] = buf_load16(rk_, st_goff[p]);
            pfv[0][p] = buf_load16(rv_, sv_goff[p]);
            pfk[1][p] = buf_load16(rk_, kTile + st_goff[p]);
            pfv[1][p] = buf_load16(rv_, kTile + sv_goff[p]);
            kst[p] = buf_load16(rk_, 2u * kTile + st_goff[p]);
            vst[p] = buf_load16(rv_, 2u * kTile + sv_goff[p]);
        }
    };
    // kScan: the marked row blocks among those this workgroup owns (block b = blockIdx.x + i gridDim.x).  Thread t looks at the
    // t-th of them, all loads in flight together; the marked ones are collected in LDS behind the ring and computed in turn.
    constexpr unsigned kScanBatch = 64u * kW;
    unsigned scan_base = 0, scan_n = 0, scan_i = 0;
    auto scan_next = [&]() __attribute__((always_inline)) -> unsigned {
        unsigned* list = reinterpret_cast<unsigned*>(smem + kRingSlots * kSlotBytes);   // [0] = count, [1 ..] = block ids
        while (scan_i == scan_n) {
            if (blockIdx.x + scan_base * gridDim.x >= nwg) return nwg;
            const unsigned long long b = (unsigned long long)blockIdx.x + (unsigned long long)(scan_base + tid) * gridDim.x;
            bool marked = false;
            if (b < nwg) {
                unsigned bh_, qb_;
                locate((unsigned)b, bh_, qb_);
                constexpr unsigned es_ = kOutF32 ? 4u : 2u;
                const unsigned* w0 = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(Og) +
                                                                       ((size_t)bh_ * head_elems + (size_t)qb_ * kRows * D) * es_);
                marked = *w0 == kMarker;
            }
            scan_i = scan_n = 0;
            scan_base += kScanBatch;
            // (the vote is also the barrier behind which every wave is done with the previous batch's list and with the ring)
            if (!__syncthreads_or(marked ? 1 : 0)) continue;   // the common case: nothing to do in this batch
            if (tid == 0) list[0] = 0u;
            __syncthreads();
            if (marked) list[1u + atomicAdd(&list[0], 1u)] = (unsigned)b;
            __syncthreads();
            scan_n = __builtin_amdgcn_readfirstlane(list[0]);
        }
        const unsigned r = __builtin_amdgcn_readfirstlane(list[1u + scan_i]);
        ++scan_i;
        return r;
    };
    // (the block after the current one, if the list already holds it: its Q rows are requested ahead, like the fast kernels do)
    auto scan_peek = [&]() __attribute__((always_inline)) -> unsigned {
        const unsigned* list = reinterpret_cast<const unsigned*>(smem + kRingSlots * kSlotBytes);
        return scan_i < scan_n ? (unsigned)__builtin_amdgcn_readfirstlane(list[1u + scan_i]) : nwg;
    };
#if FA_RP16_DEVICE_BODY
    const unsigned first_bid = kTail ? 0u : kScan ? scan_next() : first_item;
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
    const unsigned first_bid = kScan ? scan_next() : blockIdx.x;
#endif
    [[maybe_unused]] bool q_pending = false;   // kScan: the current block's Q rows were requested by the block before it
    constexpr unsigned kStores = (unsigned)(X * kDB);   // store instructions per item
    if constexpr (kPrefetch) {
        // The first item's inputs, requested the way every later item's are (at the end of the item before it, ahead of that
        // item's stores) -- including kStores stores, so that both ways into the loop look alike to the wait-count
        // bookkeeping (s_waitcnt vmcnt counts in order: with the same instructions behind the loads on both paths the waits
        // for Q and K/V can leave exactly the stores outstanding).  The stand-in stores put one zero chunk per wave on the first
        // row the wave will really store later (same wave, same address, program order: the real value wins).
        if (first_bid < nwg) {
            unsigned bh0, qb0;
            FA_RP16_ITEM_OF(first_bid, bh0, qb0);
            q_pending = true;
            bh0 = __builtin_amdgcn_readfirstlane(bh0);
            qb0 = __builtin_amdgcn_readfirstlane(qb0);
            const unsigned rb0 = qb0 * kRows + wave * (16u * X);
            q_issue(Qg + bh0 * head_elems, rb0);
            constexpr unsigned es0 = kOutF32 ? 4u : 2u;
            const __amdgpu_buffer_rsrc_t ro0 =
                make_rsrc(reinterpret_cast<char*>(Og) + (size_t)bh0 * head_elems * es0, (unsigned)(head_elems * es0));
#pragma unroll
            for (unsigned i = 0; i < (grp == 0u ? kStores : 0u); ++i) {   // (key-split group 1 never stores to O)
                u32x4 z = zero4u;
                asm volatile("" : "+v"(z));
                if constexpr (kOutF32) buf_store16(ro0, rb0 * D * 4u, z);
                else buf_store8(ro0, rb0 * D * 2u, u32x2{z[0], z[1]});
            }
        }
    }
    [[maybe_unused]] unsigned epoch = 0u, flag_seen = 0u;   // kFlagBar: iterations this wave has published (uniform; the same in every wave)
    [[maybe_unused]] const unsigned flag_base = lds_addr(smem_all) + kRingSlots * kSlotBytes;
    if constexpr (kFlagBar) {
        if (tid < (unsigned)kW) lds_write4_at(flag_base + 4u * tid, 0u);
        __syncthreads();
    }
#if FA_RP16_DEVICE_BODY
    unsigned bid = first_bid;
    for (; bid < nwg; bid = kTail ? tail_from(bid + 1u) : kScan ? scan_next() : bid + gridDim.x) {
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
    for (unsigned bid = first_bid; bid < nwg; bid = kScan ? scan_next() : bid + gridDim.x) {
#endif
#ifdef FA_RP16_STAMPS   // (see the top of the file)
    unsigned long long ts[8] = {};
#define FA_STAMP(i) ts[i] = wall_clock64()
#else
#define FA_STAMP(i)
#endif
    FA_STAMP(0);
    // No barrier here: the ring is only written again after the item's prologue loads have arrived, and every wave's last
    // LDS read of the previous item (the epilogue's V fragments) lies before that item's vote (__syncthreads_or) -- or the
    // barrier behind the tracked pass, which has no vote after it.  A wave therefore requests its K/V tiles as soon as its
    // own stores are issued, not when the slowest wave's are.
    unsigned bh, qb;
    FA_RP16_ITEM_OF(bid, bh, qb);
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(Kg + bh * head_elems + kv_first, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(Vg + bh * head_elems + kv_first, kv_bytes);
    [[maybe_unused]] const char* const k_head = reinterpret_cast<const char*>(Kg + bh * head_elems + kv_first);
    [[maybe_unused]] const char* const v_head = reinterpret_cast<const char*>(Vg + bh * head_elems + kv_first);
    const unsigned q_row0 = qb * kRows + wave * (16u * X) + c16;   // row of block 0; block x is 16x rows further
    // causal: tiles [0, nt) with nt up to the diagonal of the workgroup's last (existing) row; tiles >= jc cross its row range
    const int nt = kCausal ? min(ntiles, (int)(min((unsigned)N - 1u, qb * kRows + kRows - 1u) / kBlockN) + 1) : ntiles;
    const int jc = kCausal ? (int)((qb * kRows) / kBlockN) : nt;

    int q_bad = 0;
    auto q_finish = [&](auto fold_c) __attribute__((always_inline)) {   // raw rows in qf -> the B operands of this pass
        constexpr bool fold = decltype(fold_c)::value;
#pragma unroll
        for (int x = 0; x < X; ++x) {
            float amax = 0.0f;
#pragma unroll
            for (int ks = 0; ks < kKS; ++ks) {
                u32x4 raw = qf[x][ks];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if constexpr (fold) {
                        const float lo = T::lo(raw[w]) * scale_log2e, hi = T::hi(raw[w]) * scale_log2e;
                        amax = max3(amax, fabsf(lo), fabsf(hi));
                        raw[w] = F16::pack2(lo, hi);
                    } else {
                        raw[w] ^= q_flip;
                    }
                }
                qf[x][ks] = raw;
            }
            if constexpr (fold) q_bad |= (int)!(amax <= 65504.0f) | ((int)(amax != 0.0f) & (int)(amax < 6.2e-5f));
        }
        // pin the flag HERE: left to itself the compiler evaluates it after the tile loop and keeps all 64 fp32
        // products alive (spilled) across it -- 33 MB of scratch written and read back per item
        if constexpr (fold) asm volatile("" : "+v"(q_bad));
    };
    auto load_q = [&](auto fold_c) __attribute__((always_inline)) {
        q_issue(Qg + bh * head_elems, q_row0 - c16);
        q_finish(fold_c);
    };

    // bf16 K chunk -> fp16 (folded pass of bf16 inputs); k_amax collects the largest magnitude this thread converted
    float k_amax = 0.0f;
    auto k_to_f16 = [&](u32x4 kb) -> u32x4 {
        u32x4 r;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float lo = BF16::lo(kb[w]), hi = BF16::hi(kb[w]);
            k_amax = max3(k_amax, fabsf(lo), fabsf(hi));
            r[w] = F16::pack2(lo, hi);
        }
        return r;
    };

    f32x4 o[X][kDB];
    float m_ref[X] = {};
    u32x4 frag[kRing];
    f32x4 minit;   // folded pass: every score chain starts at -(wave reference maximum)
    // row sums on the matrix pipe: lacc[x][i] = sum over keys of the ROUNDED weights of row (lane & 15) of block x, the
    // same in every register and every lane group (all 16 "head-dim rows" of the ones fragment are equal): one more PV block
    // against a fragment of ones, X matrix instructions per step instead of 32 v_add_f32 per lane (DESIGN.md 3.2, 3.3)
    f32x4 lacc[X];
    u32x4 ones;   // written by an instruction the optimiser cannot hoist out of the item loop (and spill around the tile loop)
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("v_mov_b32 %0, %1" : "=v"(ones[i]) : "s"(T::kOnes2));

    // K fragment (key block kbl of half h in slot offset so, k-step ks); V^T fragment (head-dim block db) of half h
    auto read_kf = [&](unsigned so, int h, int kbl, int ks) -> u32x4 {
        return lds_read16(smem, so + (unsigned)(2 * h + kbl) * 16u * kRowB + k_rd[ks]);
    };
    auto read_vf = [&](unsigned so, int h, int db) -> u32x4 {
        u32x4 vf;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const u32x2 half = lds_read_tr8(smem, so + v_rd4[0] + (4u * h + 2u * jj) * (unsigned)kDB * 256u + db * 256u);
            vf[2 * jj] = half[0];
            vf[2 * jj + 1] = half[1];
        }
        return vf;
    };
    // kBases (one wave per SIMD): a step's fragment addresses from per-step lane bases (ring slot + lane offset, one v_add
    // each at the top of the step) plus immediates, instead of one s_add + v_add in front of every fragment read -- with a
    // lone wave per SIMD every such instruction is a cycle the matrix pipe waits for
    constexpr bool kBases = kSpread && (FA_RP16_ABL & 257) == 0;
    auto read_frag_b = [&](auto fc, const unsigned (&kb)[kKS], unsigned vb, int h_q, int h_v) {
        constexpr int f = decltype(fc)::value;
        if constexpr ((f & 1) == 0) {
            constexpr int kbl = (f >> 1) / kKS, ks = (f >> 1) % kKS;
            frag[f % kRing] = lds_read16_at(kb[ks] + (unsigned)(2 * h_q + kbl) * 16u * kRowB);
        } else {
            constexpr int db = f >> 1;
            u32x4 vf;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const u32x2 half = lds_read_tr8_at(vb + (4u * h_v + 2u * jj) * (unsigned)kDB * 256u + db * 256u);
                vf[2 * jj] = half[0];
                vf[2 * jj + 1] = half[1];
            }
            frag[f % kRing] = vf;
        }
    };
    // fragment f (0..kNF-1) of a step: even f -> K fragment (kbl = (f/2) / kKS, ks = (f/2) % kKS) of the QK^T unit,
    // odd f -> V^T fragment db = f/2 of the PV unit
    auto read_frag = [&](auto fc, unsigned so_q, int h_q, unsigned so_v, int h_v) {
        constexpr int f = decltype(fc)::value;
        if constexpr ((FA_RP16_ABL & 1) != 0) {   // "defined" without an instruction, so that no consumer is folded away
            asm volatile("" : "=v"(frag[f % kRing]));
            return;
        }
        if constexpr ((f & 1) == 0) frag[f % kRing] = read_kf(so_q, h_q, (f >> 1) / kKS, (f >> 1) % kKS);
        else frag[f % kRing] = read_vf(so_v, h_v, f >> 1);
        if constexpr ((FA_RP16_ABL & 256) != 0) {   // lab: every fragment read issued twice (the neighbouring fragment, discarded): what LDS operand traffic costs
            u32x4 dup;
            if constexpr ((f & 1) == 0) dup = read_kf(so_q, h_q, (f >> 1) / kKS, ((f >> 1) % kKS) ^ 1);
            else dup = read_vf(so_v, h_v, (f >> 1) ^ 1);
            asm volatile("" :: "v"(dup));
        }
    };
    auto mask_unit = [&](int tile, int h, f32x4 (&s)[X][2]) {   // keys >= N (causal: keys after the query) -> -inf (p = 0)
#pragma unroll
        for (int x = 0; x < X; ++x)
#pragma unroll
            for (int kbl = 0; kbl < 2; ++kbl)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = tile * kBlockN + 32 * h + 16 * kbl + 4 * (int)g + i;
                    if (key >= Nkv || (kCausal && (unsigned)key > q_row0 + 16u * x)) s[x][kbl][i] = -INFINITY;
                }
    };
    auto row_max = [&](const f32x4 (&s)[2]) -> float {   // this row's 32 keys of the unit, unscaled
        const float a = max3(s[0][0], s[0][1], s[0][2]), b = max3(s[1][0], s[1][1], s[1][2]);
        return across_max(max3(a, b, fmaxf(s[0][3], s[1][3])));
    };

    // One step of an optimistic pass.  h = half of tile `tile` being softmaxed (s_cur -> pk_cur); the QK^T unit is
    // (so_q, 1-h) -> s_nxt, the PV unit (so_v, 1-h) <- pk_prev.  so_nq / so_nv: slots of the NEXT step's units.
    auto step = [&](auto h_c, auto masked_c, auto fast_c, auto track_c, int tile, f32x4 (&s_cur)[X][2], f32x4 (&s_nxt)[X][2],
                    u32x4 (&pk_prev)[X], u32x4 (&pk_cur)[X], unsigned so_q, unsigned so_v, unsigned so_nq, unsigned so_nv,
                    unsigned so_land, auto set_c, auto req_c) __attribute__((always_inline)) {
        u32x4 (&k_land)[kLoads] = decltype(set_c)::value == 0 ? kst : kst2;   // the staging registers this step lands (h = 1)
        u32x4 (&v_land)[kLoads] = decltype(set_c)::value == 0 ? vst : vst2;
        constexpr int h = decltype(h_c)::value, ho = 1 - h;
        constexpr bool kFast = decltype(fast_c)::value;
        if constexpr (decltype(masked_c)::value) mask_unit(tile, h, s_cur);
        if constexpr (decltype(track_c)::value) {
            // The running maximum of the online softmax (flashattn_streaming_16x16_mw.cu:200-229, _v12f.cu:193-220), lazily: the
            // reference of a row moves only when this unit's scores exceed it by more than kThr log2 units (p <= 2^kThr fits the
            // 16-bit weights), decided by ONE wave vote over per-lane maxima -- no cross-lane step unless it fires.  When it does,
            // everything still in the old scale is multiplied by 2^(old - new) exactly once: O, the row sums and the packed P of
            // the previous unit, whose P.V is issued during this step (guide T13: the decision must not split a pending P.V).
            // (v_max3_f32 spelled out: fmaxf on matrix results gets a canonicalising v_max per operand in front of it)
            auto max3r = [](float a, float b, float d) -> float {
                float r;
                asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(d));
                return r;
            };
            auto lane_max = [&](int x) -> float {   // this lane's 8 keys of block x's row, scaled
                const float a = max3r(s_cur[x][0][0], s_cur[x][0][1], s_cur[x][0][2]), b = max3r(s_cur[x][1][0], s_cur[x][1][1], s_cur[x][1][2]);
                return max3r(a, b, max3r(s_cur[x][0][3], s_cur[x][1][3], s_cur[x][1][3])) * c;
            };
            int need = 0;   // (no short-circuit: one compare per block, no branch)
#pragma unroll
            for (int x = 0; x < X; ++x) need |= (int)(lane_max(x) - m_ref[x] > kThr);
            if (__any(need != 0)) {
#pragma unroll
                for (int x = 0; x < X; ++x) {
                    const float m_new = fmaxf(m_ref[x], across_max(lane_max(x)));   // (a row that stayed below simply moves to its own maximum)
                    const float alpha = fast_exp2(m_ref[x] - m_new);
                    m_ref[x] = m_new;
#pragma unroll
                    for (int db = 0; db < kDB; ++db)
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[x][db][i] *= alpha;
#pragma unroll
                    for (int i = 0; i < 4; ++i) lacc[x][i] *= alpha;
#pragma unroll
                    for (int w = 0; w < 4; ++w) pk_prev[x][w] = T::pack2(T::lo(pk_prev[x][w]) * alpha, T::hi(pk_prev[x][w]) * alpha);
                }
            }
        }

        constexpr int kPairs = 4 * X;   // vector pair-steps: pair j = (block j/4, key block (j/2)&1, registers 2(j&1), 2(j&1)+1)
        auto fma_pair = [&](auto jc) {
            constexpr int j = decltype(jc)::value, x = j >> 2, kbl = (j >> 1) & 1, e = 2 * (j & 1);
            s_cur[x][kbl][e] = __builtin_fmaf(s_cur[x][kbl][e], c, -m_ref[x]);
            s_cur[x][kbl][e + 1] = __builtin_fmaf(s_cur[x][kbl][e + 1], c, -m_ref[x]);
        };
        auto exp_pair = [&](auto jc) {
            constexpr int j = decltype(jc)::value, x = j >> 2, kbl = (j >> 1) & 1, e = 2 * (j & 1);
            s_cur[x][kbl][e] = fast_exp2(s_cur[x][kbl][e]);
            s_cur[x][kbl][e + 1] = fast_exp2(s_cur[x][kbl][e + 1]);
        };
        auto fma_one = [&](auto jc, auto ec) {
            constexpr int j = decltype(jc)::value, x = j >> 2, kbl = (j >> 1) & 1, e = 2 * (j & 1) + decltype(ec)::value;
            s_cur[x][kbl][e] = __builtin_fmaf(s_cur[x][kbl][e], c, -m_ref[x]);
        };
        auto exp_one = [&](auto jc, auto ec) {   // (pinned: the value exists at this point of the stream, not where its consumer is)
            constexpr int j = decltype(jc)::value, x = j >> 2, kbl = (j >> 1) & 1, e = 2 * (j & 1) + decltype(ec)::value;
            float p = fast_exp2(s_cur[x][kbl][e]);
            asm volatile("" : "+v"(p));
            s_cur[x][kbl][e] = p;
        };
        auto fin_pair = [&](auto jc) {
            constexpr int j = decltype(jc)::value, x = j >> 2, kbl = (j >> 1) & 1, e = 2 * (j & 1);
            unsigned w = T::pack2(s_cur[x][kbl][e], s_cur[x][kbl][e + 1]);
            if constexpr (kVSplit) asm volatile("" : "+v"(w));
            pk_cur[x][2 * kbl + (j & 1)] = w;
        };
        auto valu_step = [&](auto jc) {   // skewed: nothing waits on the instruction before it
            constexpr int j = decltype(jc)::value;
            if constexpr ((FA_RP16_ABL & 2) != 0) {   // keep the scores "used" without an instruction
                if constexpr (j == 0) {
#pragma unroll
                    for (int x = 0; x < X; ++x) asm volatile("" :: "v"(s_cur[x][0]), "v"(s_cur[x][1]));
                }
                return;
            }
            if constexpr (j + 2 < kPairs && !kFast) fma_pair(std::integral_constant<int, j + 2>{});
            if constexpr (j + 1 < kPairs) exp_pair(std::integral_constant<int, j + 1>{});
            fin_pair(jc);
        };
        auto issue_mfma = [&](auto ic) {
            constexpr int i = decltype(ic)::value, f = i / X, x = i % X;
            if constexpr ((FA_RP16_ABL & 4) != 0) {   // the fragment stays "used"
                if constexpr (x == 0) asm volatile("" :: "v"(frag[f % kRing]));
                return;
            }
            if constexpr ((f & 1) == 0) {
                constexpr int kbl = (f >> 1) / kKS, ks = (f >> 1) % kKS;
                using MQ = std::conditional_t<kCvtK && kFast, Mx<F16>, M>;
                if constexpr (kAsmQK) {
                    if constexpr (ks != 0) MQ::mfma_v_acc(s_nxt[x][kbl], frag[f % kRing], qf[x][ks]);
                    else if constexpr (kFast) s_nxt[x][kbl] = MQ::mfma_v_init(frag[f % kRing], qf[x][ks], minit);
                    else s_nxt[x][kbl] = MQ::mfma_v_zero(frag[f % kRing], qf[x][ks]);
                } else {
                    s_nxt[x][kbl] = MQ::mfma(frag[f % kRing], qf[x][ks], ks == 0 ? (kFast ? minit : zero4) : s_nxt[x][kbl]);
                }
            } else {
                constexpr int db = f >> 1;
                o[x][db] = M::mfma(frag[f % kRing], pk_prev[x], o[x][db]);
            }
        };

        if constexpr (!kFast && (FA_RP16_ABL & 2) == 0) {
            fma_pair(c0{});
            fma_pair(c1{});
        }
        if constexpr ((FA_RP16_ABL & 2) == 0) exp_pair(c0{});
        [[maybe_unused]] unsigned kb_q[kKS], kb_n[kKS], vb_v = 0u, vb_n = 0u, land_k = 0u, land_v = 0u;
        [[maybe_unused]] __amdgpu_buffer_rsrc_t rk_t = rk, rv_t = rv;
        // (each base is formed behind the matrix instruction in front of its first read, not in a bunch at the top of the step)
        static_assert(!kBases || kAhead <= 2 * kKS, "the fragments read ahead into the next step are of its first key block");
        auto form_base = [&](auto fc) {
            constexpr int f = decltype(fc)::value;   // fragment about to be read; f >= kNF: of the next step
            const unsigned smem_a = lds_addr(smem);
            if constexpr (f >= kNF) {
                constexpr int fp = f - kNF;
                if constexpr ((fp & 1) == 0) { kb_n[fp >> 1] = smem_a + so_nq + k_rd[fp >> 1]; asm volatile("" : "+v"(kb_n[fp >> 1])); }
                if constexpr (fp == 1) { vb_n = smem_a + so_nv + v_rd4[0]; asm volatile("" : "+v"(vb_n)); }
            } else if constexpr ((f & 1) == 0) {
                constexpr int ks = (f >> 1) % kKS;
                if constexpr (f - 2 * kKS < kAhead) {   // no earlier in-step fragment with this ks
                    kb_q[ks] = smem_a + so_q + k_rd[ks];
                    asm volatile("" : "+v"(kb_q[ks]));
                }
            } else if constexpr (f - 2 < kAhead) {
                vb_v = smem_a + so_v + v_rd4[0];
                asm volatile("" : "+v"(vb_v));
            }
        };
        sfor<kSlots>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (kFlagBar) {
                if constexpr (h == 0 && i == kFlagRead) flag_seen = lds_read4_at(flag_base + 4u * (lane & (unsigned)(kW - 1)));
                if constexpr (h == 0 && i == kFlagCheck) {   // every wave has landed the tile the next fragment reads touch
                    while (!__all((int)(flag_seen - epoch) >= 0)) {
                        __builtin_amdgcn_s_sleep(1);
                        flag_seen = lds_read4_at(flag_base + 4u * (lane & (unsigned)(kW - 1)));
                    }
                }
                if constexpr (h == 1 && i == kLandLast + 1) {   // this wave's chunks of tile j+2 are in LDS (in order behind them)
                    ++epoch;
                    lds_write4_at(flag_base + 4u * wave, epoch);
                }
            }
            if constexpr (kSpread && (FA_RP16_ABL & 8) == 0) {
                if constexpr (h == 0 && i < 2 * kLoads && decltype(req_c)::value) {   // request chunk i of tile j+2
                    constexpr int p = i >> 1;
                    if constexpr (kBases) {
                        // the tile's offset goes into the DESCRIPTOR (base up, bytes down: scalar instructions, and the bounds still
                        // cut at the end of the head) instead of into eight per-lane offsets
                        if constexpr (i == 0) {
                            const unsigned t_off = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(tile + kLook) * kTile);
                            const unsigned left = (unsigned)__builtin_amdgcn_readfirstlane(t_off < kv_bytes ? kv_bytes - t_off : 0u);
                            auto uniform_ptr = [](const char* q) -> const char* {   // (uniform anyway: spares the descriptor a waterfall loop)
                                const unsigned long long a = (unsigned long long)q;
                                const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a);
                                const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
                                return reinterpret_cast<const char*>((unsigned long long)lo | ((unsigned long long)hi << 32));
                            };
                            rk_t = make_rsrc(uniform_ptr(k_head + t_off), left);
                            rv_t = make_rsrc(uniform_ptr(v_head + t_off), left);
                        }
                        if constexpr ((i & 1) == 0) kst[p] = buf_load16(rk_t, st_goff[p]);
                        else vst[p] = buf_load16(rv_t, sv_goff[p]);
                    } else {
                        if constexpr ((i & 1) == 0) kst[p] = buf_load16(rk, (unsigned)(tile + kLook) * kTile + st_goff[p]);
                        else vst[p] = buf_load16(rv, (unsigned)(tile + kLook) * kTile + sv_goff[p]);
                    }
                }
                if constexpr (h == 1 && i >= kLandSlot && i <= kLandLast) {   // land chunk i - kLandSlot
                    constexpr int p = (i - kLandSlot) >> 1;
                    if constexpr (kBases) {
                        // chunk p of a thread lies 64 kW / kChunks rows below chunk 0 in both images (the K swizzle and the V block
                        // map repeat every 16 rows at D = 128): one address each, the rest in the immediate
                        static_assert(!kBases || ((64 * kW) % G::kChunks == 0 && ((64 * kW) / G::kChunks) % 16 == 0), "chunk p = chunk 0 + p rows, a multiple of 16 (both image maps repeat)");
                        constexpr unsigned kStepK = (64u * kW / G::kChunks) * kRowB, kStepV = (64u * kW / G::kChunks / 8u) * (unsigned)kDB * 256u;
                        if constexpr (i == kLandSlot) {
                            land_k = lds_addr(smem) + so_land + k_lds[0];
                            asm volatile("" : "+v"(land_k));
                            land_v = lds_addr(smem) + so_land + v_lds[0];
                            asm volatile("" : "+v"(land_v));
                        }
                        if constexpr (((i - kLandSlot) & 1) == 0) lds_write16_at(land_k + p * kStepK, (kCvtK && kFast) ? k_to_f16(k_land[p]) : k_land[p]);
                        else lds_write16_at(land_v + p * kStepV, v_land[p]);
                    } else {
                        if constexpr (((i - kLandSlot) & 1) == 0) lds_write16(smem, so_land + k_lds[p], (kCvtK && kFast) ? k_to_f16(k_land[p]) : k_land[p]);
                        else lds_write16(smem, so_land + v_lds[p], v_land[p]);
                    }
                }
            } else if constexpr (h == 1 && i == kLandSlot && !kDma && (FA_RP16_ABL & 8) == 0) {   // land tile j+2 (requested at the top of the iteration)
#pragma unroll
                for (int p = 0; p < kLoads; ++p) {
                    lds_write16(smem, so_land + k_lds[p], (kCvtK && kFast) ? k_to_f16(k_land[p]) : k_land[p]);
                    lds_write16(smem, so_land + v_lds[p], v_land[p]);
                }
            }
            issue_mfma(ic);
            if constexpr ((FA_RP16_ABL & 4) == 0 && i % kNF == kNF - 1)   // the X row-sum instructions of the step, one per kNF slots
                lacc[i / kNF] = M::mfma(ones, pk_prev[i / kNF], lacc[i / kNF]);
            if constexpr (i % X == X - 1) {   // the fragment just consumed X times is free: read kAhead ahead
                constexpr int f = i / X + kAhead;
                if constexpr (kBases) {
                    form_base(std::integral_constant<int, f>{});
                    if constexpr (f < kNF) read_frag_b(std::integral_constant<int, f>{}, kb_q, vb_v, ho, ho);
                    else read_frag_b(std::integral_constant<int, f - kNF>{}, kb_n, vb_n, h, h);
                } else {
                    if constexpr (f < kNF) read_frag(std::integral_constant<int, f>{}, so_q, ho, so_v, ho);
                    else read_frag(std::integral_constant<int, f - kNF>{}, so_nq, h, so_nv, h);
                }
            }
            constexpr int kPer = kSlots / kPairs;   // matrix slots per vector pair-step (2 at D = 64, 4 at D = 128)
            if constexpr (kVSplit && (FA_RP16_ABL & 2) == 0) {
                // the pair-step's instructions one by one behind consecutive matrix instructions: a v_exp (or v_cvt_pk) of ~8 issue
                // cycles fits in the shadow of the 16-cycle matrix instruction in front of it, three in a row do not
                constexpr int j = i / kPer, sub = i % kPer;
                if constexpr (sub < 2) {
                    if constexpr (j + 2 < kPairs && !kFast) fma_one(std::integral_constant<int, j + 2>{}, std::integral_constant<int, sub>{});
                    if constexpr (j + 1 < kPairs) exp_one(std::integral_constant<int, j + 1>{}, std::integral_constant<int, sub>{});
                }
                if constexpr (sub == (kPer == 2 ? 1 : 2)) fin_pair(std::integral_constant<int, j>{});
            } else if constexpr (i % kPer == kPer - 1) {   // the whole pair-step behind the last matrix instruction of its group
                valu_step(std::integral_constant<int, i / kPer>{});
            }
        });
        __builtin_amdgcn_sched_barrier(0);
    };

    // a packed weight can only have overflowed if the fp32 row sum reached the 16-bit format's range; bf16 keeps a finite bound with
    // room for sum(p*v) in fp32
    const float lim = T::id == 1 ? 0x1p+96f : 60000.0f;
    constexpr int kCheckEvery = 8;   // exact optimistic pass, fp16: tiles between two looks at the row sums (an overflow ends the pass there)
    // mode 0: folded fast pass; 1: exact, reference max fixed after the first 32 keys; 2: exact, lazy running max (same pipeline)
    // returns true when the folded pass gave up right after its reference was known (nothing computed yet)
    // pre_c: the item's first three K/V tiles are already in flight (requested at the end of the previous item)
    auto run = [&](auto mode_c, auto pre_c) __attribute__((always_inline)) -> bool {
        constexpr int kMode = decltype(mode_c)::value;
        constexpr bool kPre = decltype(pre_c)::value;
        constexpr bool kTrack = kMode == 2, kFast = kMode == 0;
        const std::integral_constant<bool, kFast> fast_c{};
        const std::integral_constant<bool, kTrack> track_c{};
        f32x4 sA[X][2], sB[X][2];
        u32x4 pkA[X], pkB[X];
#pragma unroll
        for (int x = 0; x < X; ++x) {
#pragma unroll
            for (int db = 0; db < kDB; ++db) o[x][db] = zero4;
            lacc[x] = zero4;
            pkB[x] = zero4u;   // "P(-1)" = 0 against the zeroed V of the ring's last slot
        }
        // ---- prologue: tiles 0 and 1 -> slots 0 and 1; V of slot 3 ("tile -1") zeroed ----
        if constexpr (kDma) {
#pragma unroll
            for (int p = 0; p < kLoads; ++p) lds_write16(smem, kRingMask * kSlotBytes + v_lds[p], zero4u);
            dma_tile(rk, rv, 0u, 0u);
            dma_tile(rk, rv, kTile, kSlotBytes);
        } else {   // tiles 0 and 1 -> LDS; tile 2 stays in the staging registers until iteration 0 lands it
            if constexpr (!kPre) kv_issue(rk, rv);
#pragma unroll
            for (int p = 0; p < kLoads; ++p) {
                lds_write16(smem, kRingMask * kSlotBytes + v_lds[p], zero4u);
                lds_write16(smem, k_lds[p], (kCvtK && kFast) ? k_to_f16(pfk[0][p]) : pfk[0][p]);
                lds_write16(smem, v_lds[p], pfv[0][p]);
                lds_write16(smem, kSlotBytes + k_lds[p], (kCvtK && kFast) ? k_to_f16(pfk[1][p]) : pfk[1][p]);
                lds_write16(smem, kSlotBytes + v_lds[p], pfv[1][p]);
                if constexpr (kPair) {   // tile 2 as well: an iteration starts with the tiles up to two ahead of it in LDS
                    lds_write16(smem, 2u * kSlotBytes + k_lds[p], (kCvtK && kFast) ? k_to_f16(kst[p]) : kst[p]);
                    lds_write16(smem, 2u * kSlotBytes + v_lds[p], vst[p]);
                }
            }
        }
        __syncthreads();
        if constexpr (kMode == (kFold ? 0 : 1)) FA_STAMP(2);
        if constexpr (kAsmQK) {   // Q' may have been finished by vector instructions just above: wait states the compiler would count for a builtin
#pragma unroll
            for (int x = 0; x < X; ++x)
#pragma unroll
                for (int ks = 0; ks < kKS; ++ks) asm volatile("s_nop 4" : "+v"(qf[x][ks]));
        }
#pragma unroll
        for (int kbl = 0; kbl < 2; ++kbl)   // S(unit 0)
#pragma unroll
            for (int ks = 0; ks < kKS; ++ks) {
                const u32x4 kf = read_kf(0u, 0, kbl, ks);
                using MQ = std::conditional_t<kCvtK && kFast, Mx<F16>, M>;
#pragma unroll
                for (int x = 0; x < X; ++x) {
                    if constexpr (!kAsmQK) sA[x][kbl] = MQ::mfma(kf, qf[x][ks], ks == 0 ? zero4 : sA[x][kbl]);
                    else if (ks == 0) sA[x][kbl] = MQ::mfma_v_zero(kf, qf[x][ks]);
                    else MQ::mfma_v_acc(sA[x][kbl], kf, qf[x][ks]);
                }
            }
        if constexpr (kAsmQK) {   // the matrix results are read by vector instructions right below: 16 wait states behind each
#pragma unroll
            for (int x = 0; x < X; ++x) asm volatile("s_nop 15" : "+v"(sA[x][0]), "+v"(sA[x][1]));
        }
        {
            // reference max from the first 32 keys (masked copy when N < 32; the step masks again)
            f32x4 s0[X][2];
#pragma unroll
            for (int x = 0; x < X; ++x) { s0[x][0] = sA[x][0]; s0[x][1] = sA[x][1]; }
            if ((partial && ntiles == 1) || (kCausal && jc == 0)) mask_unit(0, 0, s0);
            if constexpr (kFast) {   // one reference for the wave; the folded scores already carry the scale
                float mw = -INFINITY;
#pragma unroll
                for (int x = 0; x < X; ++x) mw = fmaxf(mw, row_max(s0[x]));
#pragma unroll
                for (int sh = 1; sh < 16; sh <<= 1) mw = fmaxf(mw, row_ror(mw, sh));   // over the 16 rows of a lane group (DPP)
                if (kCausal || (partial && ntiles == 1)) {
                    mw += kHeadroomFold;
                } else {
                    // Place the reference so that a typical row sum lands mid-window (2^kFoldAim; the window is
                    // [N 2^-16, 60000) for fp16 weights): the mean weight of these 64 x 32 scores relative to their maximum
                    // predicts the row sum N * mean * 2^(max - reference).  With the maximum + 1 alone, rows of a wave whose
                    // first scores hold an outlier fell below the window once the logits spread a little (sigma ~ 3 log2 units).
                    float e = 0.0f;
#pragma unroll
                    for (int x = 0; x < X; ++x)
#pragma unroll
                        for (int kbl = 0; kbl < 2; ++kbl)
#pragma unroll
                            for (int i = 0; i < 4; ++i) e += fast_exp2(s0[x][kbl][i] - mw);
                    e = across_sum(e);
#pragma unroll
                    for (int sh = 1; sh < 16; sh <<= 1) e += row_ror(e, sh);
                    // (N through an opaque copy: hoisted out of the item loop, the product would be spilled around the tile
                    // loop and its reload -- s_waitcnt vmcnt(0) -- would sit behind whatever memory traffic is in flight)
                    int n_here = Nkv;
                    asm volatile("" : "+s"(n_here));
                    const float shift = __builtin_amdgcn_logf((float)n_here * e * (1.0f / (16.0f * X * 32.0f))) - kFoldAim;
                    mw += fminf(fmaxf(shift, -kFoldShiftMin), kFoldMax);
                }
#pragma unroll
                for (int x = 0; x < X; ++x) m_ref[x] = mw;
                // the gates that are known now (reference beyond kFoldMax, folded Q out of range) end the pass before it costs
                // anything: one workgroup vote per item
                if (__syncthreads_or(((((FA_RP16_GATES & 4) != 0) && !(fabsf(mw) <= kFoldMax)) || (((FA_RP16_GATES & 8) != 0) && q_bad != 0)) ? 1 : 0)) return true;
#pragma unroll
                for (int i = 0; i < 4; ++i) minit[i] = -mw;
#pragma unroll
                for (int x = 0; x < X; ++x)
#pragma unroll
                    for (int kbl = 0; kbl < 2; ++kbl)
#pragma unroll
                        for (int i = 0; i < 4; ++i) sA[x][kbl][i] -= mw;   // unit 0 was accumulated from zero
            } else {
#pragma unroll
                for (int x = 0; x < X; ++x) m_ref[x] = row_max(s0[x]) * c + (kTrack ? 0.0f : kHeadroom);
            }
        }
        // the first kAhead fragments of the first step: K(tile 0, half 1), V("tile -1")
        sfor<kAhead>([&](auto fc) { read_frag(fc, 0u, 1, kRingMask * kSlotBytes, 1); });

        // phase_c: j & 3 when the caller knows it at compile time (the unrolled steady state: ring slot offsets become
        // immediates of the LDS instructions instead of one v_add per fragment read), -1 otherwise
        // req_c: request tile j+2 at the top (not in iteration 0 of the non-DMA path: the prologue already has it in flight)
        auto tile_barrier = [&]() __attribute__((always_inline)) {
            if constexpr ((FA_RP16_ABL & 16) != 0 || kFlagBar) {
            } else if constexpr (!kDma && kLdsAfterLand <= 15) {
                // The barrier publishes this wave's ds_writes of the landed tile (first read at least one iteration later) and orders
                // the ring's reuse; it does not need the fragment reads issued since (LDS operations of a wave complete in order: once
                // at most kLdsAfterLand are outstanding, the writes are done).  __syncthreads() would wait for all of them
                // (s_waitcnt lgkmcnt(0)): the latency of the last read, exposed once per tile (DESIGN.md 3.6 (4)).
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(kLdsAfterLand) : "memory");
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            } else {   // (LDS-DMA: the barrier also has to wait for the tile's loads, vmcnt; beyond 15 the counter's field ends)
                __syncthreads();
            }
        };
        auto tile_iter = [&](int j, auto masked_c, auto phase_c, auto req_c) __attribute__((always_inline)) {
            constexpr int ph = decltype(phase_c)::value;
            const unsigned jj = ph >= 0 ? (unsigned)ph : (unsigned)j;
            const unsigned so_m1 = ((jj + kRingMask) & kRingMask) * kSlotBytes, so_0 = (jj & kRingMask) * kSlotBytes;
            const unsigned so_p1 = ((jj + 1u) & kRingMask) * kSlotBytes, so_ld = ((jj + (unsigned)kLook) & kRingMask) * kSlotBytes;
            // tile j + kLook: tiles past the end read zeros through the buffer bounds into a free slot
            if constexpr ((FA_RP16_ABL & 8) != 0 || !decltype(req_c)::value || kSpread) {   // (kSpread: inside the first step)
            } else if constexpr (kDma) {
                dma_tile(rk, rv, (unsigned)(j + 2) * kTile, so_ld);   // the barrier below waits for it (vmcnt) and publishes it
            } else {
#pragma unroll
                for (int p = 0; p < kLoads; ++p) {
                    kst[p] = buf_load16(rk, (unsigned)(j + kLook) * kTile + st_goff[p]);
                    vst[p] = buf_load16(rv, (unsigned)(j + kLook) * kTile + sv_goff[p]);
                }
            }
            //   h 0: softmax (j,0);  QK^T (j,1);    PV (j-1,1);  next step: QK^T (j+1,0), PV (j,0)
            //   h 1: softmax (j,1);  QK^T (j+1,0);  PV (j,0);    next step: QK^T (j+1,1), PV (j,1)
            step(c0{}, masked_c, fast_c, track_c, j, sA, sB, pkB, pkA, so_0, so_m1, so_p1, so_0, so_ld, c0{}, req_c);
            step(c1{}, masked_c, fast_c, track_c, j, sB, sA, pkA, pkB, so_p1, so_0, so_p1, so_0, so_ld, c0{}, req_c);
            tile_barrier();
        };
        // kPair: tiles j and j+1 in one iteration: tiles j+3 and j+4 requested at the top and landed in the second step of each tile,
        // one barrier behind both (the iteration starts with the tiles up to j+2 in LDS: the last step reads K of tile j+2)
        auto pair_iter = [&](int j) __attribute__((always_inline)) {
            const unsigned jj = (unsigned)j;
            const unsigned so_m1 = ((jj + kRingMask) & kRingMask) * kSlotBytes, so_0 = (jj & kRingMask) * kSlotBytes;
            const unsigned so_p1 = ((jj + 1u) & kRingMask) * kSlotBytes, so_p2 = ((jj + 2u) & kRingMask) * kSlotBytes;
            const unsigned so_p3 = ((jj + 3u) & kRingMask) * kSlotBytes, so_p4 = ((jj + 4u) & kRingMask) * kSlotBytes;
            if constexpr ((FA_RP16_ABL & 8) == 0) {
#pragma unroll
                for (int p = 0; p < kLoads; ++p) {
                    kst[p] = buf_load16(rk, (unsigned)(j + 3) * kTile + st_goff[p]);
                    vst[p] = buf_load16(rv, (unsigned)(j + 3) * kTile + sv_goff[p]);
                    kst2[p] = buf_load16(rk, (unsigned)(j + 4) * kTile + st_goff[p]);
                    vst2[p] = buf_load16(rv, (unsigned)(j + 4) * kTile + sv_goff[p]);
                }
            }
            step(c0{}, no, fast_c, track_c, j, sA, sB, pkB, pkA, so_0, so_m1, so_p1, so_0, so_p3, c0{}, no);
            step(c1{}, no, fast_c, track_c, j, sB, sA, pkA, pkB, so_p1, so_0, so_p1, so_0, so_p3, c0{}, no);
            step(c0{}, no, fast_c, track_c, j + 1, sA, sB, pkB, pkA, so_p1, so_0, so_p2, so_p1, so_p4, c1{}, no);
            step(c1{}, no, fast_c, track_c, j + 1, sB, sA, pkA, pkB, so_p2, so_p1, so_p2, so_p1, so_p4, c1{}, no);
            tile_barrier();
        };
        if constexpr (kMode == (kFold ? 0 : 1)) FA_STAMP(3);
        using dyn = std::integral_constant<int, -1>;
        // iteration 0 of the one-tile-per-iteration form requests nothing unless staging is by DMA: the prologue has tile 2 in flight
        const std::integral_constant<bool, kDma || kPair> req0{};
        // returns true when the pass was given up on a workgroup vote: fp16 weights of the exact optimistic pass overflowed (the
        // matrix-pipe row sums are complete in every lane, so the look costs a compare per block and a vote every kCheckEvery tiles)
        auto full_tiles = [&](int nfull) __attribute__((always_inline)) -> bool {
            constexpr bool kLook4Overflow = kMode == 1 && T::id == 0 && FA_RP16_ABL == 0;
            auto overflowed = [&]() -> bool {
                bool over = false;
#pragma unroll
                for (int x = 0; x < X; ++x) over = over || !(lacc[x][0] < lim);
                return __syncthreads_or(over ? 1 : 0) != 0;
            };
            int j = 0;
            if constexpr (kPair) {
                for (; j + 1 < nfull; j += 2) {
                    pair_iter(j);
                    if constexpr (kLook4Overflow) { if (((j + 2) % kCheckEvery) == 0 && j + 2 < nfull && overflowed()) return true; }
                }
                if (j < nfull) tile_iter(j, no, dyn{}, yes);
                return false;
            }
            if (nfull > 0) { tile_iter(0, no, dyn{}, req0); j = 1; }
            if constexpr (kLook4Overflow) {
                while (j < nfull) {
                    const int je = min(nfull, j + kCheckEvery);
                    for (; j < je; ++j) tile_iter(j, no, dyn{}, yes);
                    if (j < nfull && overflowed()) return true;
                }
            } else {
                for (; j < nfull; ++j) tile_iter(j, no, dyn{}, yes);
            }
            return false;
        };
        // (a masked iteration 0 requests tile 2 once more: the same data into the same registers)
        if constexpr (kCausal) {
            if (full_tiles(jc)) return true;
            for (int j = jc; j < nt; ++j) tile_iter(j, yes, dyn{}, yes);
        } else {
            if (full_tiles(partial ? ntiles - 1 : ntiles)) return true;
            if (partial) tile_iter(ntiles - 1, yes, dyn{}, yes);
        }
        if constexpr (kMode == (kFold ? 0 : 1)) FA_STAMP(4);
        // ---- epilogue: O^T += V(last tile, half 1)^T.P^T ----
        {
            const unsigned so = ((unsigned)(nt - 1) & kRingMask) * kSlotBytes;
#pragma unroll
            for (int db = 0; db < kDB; ++db) {
                const u32x4 vf = read_vf(so, 1, db);
#pragma unroll
                for (int x = 0; x < X; ++x) o[x][db] = M::mfma(vf, pkB[x], o[x][db]);
            }
#pragma unroll
            for (int x = 0; x < X; ++x) lacc[x] = M::mfma(ones, pkB[x], lacc[x]);
        }
        return false;
    };

    float l_row[X];
    bool bad = false, second_vote = false, direct = false;   // (second_vote, direct: workgroup-uniform)
    // a pass' row sum: complete in every lane (it comes from the matrix pipe)
    auto row_sum = [&](int x) -> float { return lacc[x][0]; };
    if constexpr (!kPrefetch) q_issue(Qg + bh * head_elems, q_row0 - c16);   // else: requested by the item before (next_in)
    else {
        if constexpr (kScan) { if (!q_pending) q_issue(Qg + bh * head_elems, q_row0 - c16); }   // (first block of a later list batch)
        kv_issue(rk, rv);   // tiles 0..2 on their way before Q is waited for
    }
    const std::integral_constant<bool, kPrefetch> pre_c{};
    // qf, pfk/pfv, kst/vst <- the next item's raw Q rows and K/V tiles 0..2 (called between the last pass and the stores)
    auto next_in = [&]() __attribute__((always_inline)) {
        if constexpr (kPrefetch) {
#if FA_RP16_DEVICE_BODY
            const unsigned nbid = kTail ? tail_from(bid + 1u) : kScan ? scan_peek() : bid + gridDim.x;
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
            const unsigned nbid = kScan ? scan_peek() : bid + gridDim.x;
#endif
            if constexpr (kScan) q_pending = nbid < nwg;
            if (nbid < nwg) {
                unsigned bh_n, qb_n;
                FA_RP16_ITEM_OF(nbid, bh_n, qb_n);
                bh_n = __builtin_amdgcn_readfirstlane(bh_n);   // (uniform anyway: spares the descriptors a waterfall loop)
                qb_n = __builtin_amdgcn_readfirstlane(qb_n);
                q_issue(Qg + bh_n * head_elems, qb_n * kRows + wave * (16u * X));
            }
        }
    };
    bool redo = false;   // (workgroup-uniform) full-width waves: this block is left to the redo kernel
    [[maybe_unused]] unsigned pass_id = kFold ? 0u : 1u;
    if constexpr (kScan) {
        q_finish(no);
        direct = true;
    } else if constexpr (kFold) {
        k_amax = 0.0f;
        q_finish(yes);
        FA_STAMP(1);
        const bool gave_up = run(std::integral_constant<int, 0>{}, pre_c);
        // fp16 weights: each subnormal one is off by at most 2^-25, N of them by N * 2^-25 in the worst case (2^-13 * sqrt(N)
        // typically), which stays below 2^-9 of the row sum; bf16 weights only must not vanish in fp32 (a row more than ~100
        // log2 units below its wave's reference: p = 0, l = 0)
        int n_here = Nkv;
        asm volatile("" : "+s"(n_here));   // as above: no spilled constant behind the Q prefetch
        const float lo = T::id == 0 ? (float)n_here * 0x1p-16f : 0x1p-100f;
#pragma unroll
        for (int x = 0; x < X; ++x) {
            l_row[x] = row_sum(x);
            // causal: a row only has row+1 keys to add up
            const float lo_x = (kCausal && T::id == 0) ? (float)min((unsigned)n_here, q_row0 + 16u * x + 1u) * 0x1p-16f : lo;
            // upper gate: 60000 for BOTH input types.  For bf16 the weights themselves would hold far more (lim = 2^96), but a row
            // sum beyond 2^16 means logits more than 16 above a reference that is itself up to kFoldMax in magnitude, and the
            // rounding of Q' (|logit| 2^-11 per logit) then moves the ratio of two comparable dominant weights by up to ~0.5 %
            bad = bad || ((FA_RP16_GATES & 1) && !(l_row[x] < 60000.0f)) || ((FA_RP16_GATES & 2) && !(l_row[x] >= lo_x)) ||
                  ((FA_RP16_GATES & 4) && !(fabsf(m_ref[x]) <= kFoldMax));
        }
        bad = bad || gave_up || ((FA_RP16_GATES & 8) && q_bad != 0) || !(k_amax <= 65504.0f);
        if constexpr ((FA_RP16_ABL & 255) != 0) bad = false;
        // folded pass refused: the exact optimistic pass first (same pipeline, per-row reference, one v_fma per score --
        // it is what large logits need; bf16 weights cannot overflow in it), the tracked pass only if that overflows too
        if (__syncthreads_or(bad ? 1 : 0)) {
            if (T::id == 0 && gave_up) {
                // fp16, refused before anything was computed (reference beyond kFoldMax, Q' out of range): logits this large overflow
                // fixed-reference fp16 weights more often than not (profiles/r02_gate_cliff.txt) -- the running-max pass at once
                direct = true;
                if constexpr (!kSplitTrack) load_q(no);
            } else {
                load_q(no);
                pass_id = 1u;
                direct = run(std::integral_constant<int, 1>{}, no);   // (true: given up on an overflow vote)
                bad = false;
#pragma unroll
                for (int x = 0; x < X; ++x) {
                    l_row[x] = row_sum(x);
                    bad = bad || !(l_row[x] < lim);
                }
                second_vote = !direct;
            }
        }
    } else {
        q_finish(no);
        direct = run(std::integral_constant<int, 1>{}, pre_c);
#pragma unroll
        for (int x = 0; x < X; ++x) {
            l_row[x] = row_sum(x);
            bad = bad || !(l_row[x] < lim);
        }
        second_vote = !direct;
    }
#if FA_RP16_DEVICE_BODY
    bool to_tracked = direct || (second_vote && __syncthreads_or(bad ? 1 : 0));
    // (The vote's result is a per-lane value to the compiler.  An appending body counts its list and leaves its loop under this
    // branch, so the count and the loop's cursor would live in vector registers across the whole item loop -- in the fp16 exact
    // pipeline, which has none to spare, the allocator then spilled all 64 accumulators around every item's votes: 90 spills,
    // 7 %.  Said to be wave-uniform, they are scalars.  Not in the folded-first kernels: they fit as they are, and their
    // measured code stays what it was.)
    if constexpr (kAppend && !kFold) to_tracked = __builtin_amdgcn_readfirstlane((int)to_tracked) != 0;
    if (to_tracked) {   // (both flags are uniform: workgroup votes decided them)
#else   // the kernel-body form keeps the statement as it was: another form = another register allocation = a kernel nobody has timed
    if (direct || (second_vote && __syncthreads_or(bad ? 1 : 0))) {   // (both flags are uniform: workgroup votes decided them)
#endif
        pass_id = kSplitTrack ? 3u : 2u;
        if constexpr (kSplitTrack) {
            redo = true;
        } else {
            if constexpr (kScan) run(std::integral_constant<int, 2>{}, pre_c);   // (its K/V tiles 0..2 are on their way already)
            else run(std::integral_constant<int, 2>{}, no);
#pragma unroll
            for (int x = 0; x < X; ++x) l_row[x] = row_sum(x);
            __syncthreads();   // the next item's prologue writes the ring: every wave is past this pass' last LDS read
        }
    }
#ifdef FA_EXPERIMENTS
    if constexpr (!kScan) {
        unsigned* ids = g_rp16_pass_ids;
        if (ids != nullptr && tid == 0u) ids[bh * (unsigned)nqb + qb] = pass_id;
    }
#endif
    constexpr unsigned es = kOutF32 ? 4u : 2u;
    const __amdgpu_buffer_rsrc_t ro =
        make_rsrc(reinterpret_cast<char*>(Og) + (size_t)bh * head_elems * es, (unsigned)(head_elems * es));
    if constexpr (kSplitTrack) {
        if (redo) {
#if FA_RP16_DEVICE_BODY   // (only in the device-function form; the kernel-body form must stay statement for statement what it was, see the top)
            if constexpr (kAppend) {
                // onto the list (tid 0; the wrapper's barrier in front of the half-width body publishes it).  Nothing is stored
                // to the block here: the half-width body stores all of it.  n_listed is workgroup-uniform (redo is a vote's result).
                if (tid == 0u) {
                    tail_list[2u * n_listed] = bh;
                    tail_list[2u * n_listed + 1u] = qb * (unsigned)kRows;
                }
                ++n_listed;
                if (n_listed == (unsigned)kTailCap) return bid + gridDim.x;   // full: the wrapper empties it and comes back
                next_in();
                continue;
            }
#endif
            // the marker goes where the redo kernel's two half-width blocks of this block begin: the first rows of waves 0 and
            // kW/2, written by those waves (their stand-in stores to the same addresses precede it in program order)
            next_in();
            if (lane == 0u && (wave == 0u || wave == (unsigned)(kW / 2))) buf_store4(ro, (q_row0 - c16) * D * es, kMarker);
            continue;
        }
    }

    if constexpr (kKeySplit == 2) {
        // group 1 -> group 0: (O^T unnormalised, l, m) per lane through group 1's ring (both rings are idle: every wave is past
        // its last fragment read once it is past this barrier); weights 2^(m_s - M)
        float* const xch = reinterpret_cast<float*>(smem_all + kRingSlots * kSlotBytes) + tid;
        constexpr unsigned kStride = 64u * kW;
        __syncthreads();
        if (grp == 1u) {
#pragma unroll
            for (int x = 0; x < X; ++x) {
#pragma unroll
                for (int db = 0; db < kDB; ++db)
#pragma unroll
                    for (int i = 0; i < 4; ++i) xch[((x * kDB + db) * 4 + i) * kStride] = o[x][db][i];
                xch[(X * kDB * 4 + 2 * x) * kStride] = l_row[x];
                xch[(X * kDB * 4 + 2 * x + 1) * kStride] = m_ref[x];
            }
        }
        __syncthreads();
        if (grp == 0u) {
#pragma unroll
            for (int x = 0; x < X; ++x) {
                const float l1 = xch[(X * kDB * 4 + 2 * x) * kStride], m1 = xch[(X * kDB * 4 + 2 * x + 1) * kStride];
                const float mm = fmaxf(m_ref[x], m1);
                const float a0 = fast_exp2(m_ref[x] - mm), a1 = fast_exp2(m1 - mm);
#pragma unroll
                for (int db = 0; db < kDB; ++db)
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[x][db][i] = o[x][db][i] * a0 + xch[((x * kDB + db) * 4 + i) * kStride] * a1;
                l_row[x] = l_row[x] * a0 + l1 * a1;
            }
        }
        __syncthreads();   // (group 1's next prologue writes the ring group 0 has just read)
        if (grp == 1u) {
            next_in();
            continue;
        }
    }
    // normalise in place FIRST (no temporaries alive when the prefetch takes its registers), then the next item's loads, then
    // the stores straight from the accumulators
#pragma unroll
    for (int x = 0; x < X; ++x) {
        const float inv = 1.0f / l_row[x];
#pragma unroll
        for (int db = 0; db < kDB; ++db)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[x][db][i] *= inv;
    }
    FA_STAMP(5);
    if constexpr (kPrefetch) {
#pragma unroll
        for (int x = 0; x < X; ++x)
#pragma unroll
            for (int db = 0; db < kDB; ++db) asm volatile("" : "+v"(o[x][db]));   // the multiplies stay in front of the loads
    }
    next_in();
    // o[x][db][i] = O[q_row0 + 16x][16 db + 4 g + i]
    // (sixteen 64-B pieces of sixteen rows per instruction: whole rows through LDS gained nothing, DESIGN.md 3.6 (4b))
    // (A local constant on purpose: with no declaration at this point two independent scalar moves of the FA_EXPERIMENTS build
    // swap places, and the device code is no longer instruction for instruction the one the records were measured on.)
    constexpr bool kStoreF32 = (FA_RP16_ABL & 32) == 0;
#pragma unroll
    for (int x = 0; x < X; ++x) {
        const unsigned row = q_row0 + 16u * x;
#pragma unroll
        for (int db = 0; db < kDB; ++db) {
            const unsigned col = 16u * db + 4u * g;
            if constexpr (kOutF32) {
                if constexpr (!kStoreF32) asm volatile("" :: "v"(o[x][db]));
                else buf_store16(ro, (row * D + col) * 4u, __builtin_bit_cast(u32x4, o[x][db]));
            } else {
                buf_store8(ro, (row * D + col) * 2u, u32x2{T::pack2(o[x][db][0], o[x][db][1]), T::pack2(o[x][db][2], o[x][db][3])});
            }
        }
    }
#ifdef FA_RP16_STAMPS
    FA_STAMP(6);
    if constexpr (kOutF32) {
        if (tid == 0) {
            float* orow = reinterpret_cast<float*>(Og) + ((size_t)bh * N + (size_t)qb * kRows) * D;
            orow[0] = (float)(ts[0] & 0xFFFFFFull);
            for (int i = 1; i < 7; ++i) orow[i] = (float)(long long)(ts[i] - ts[0]);
            orow[7] = (float)blockIdx.x;
        }
    }
#endif
#undef FA_STAMP
    }   // persistent loop over work items
#if FA_RP16_DEVICE_BODY   // (only in the device-function form; the kernel-body form must stay statement for statement what it was, see the top)
    return bid;
#endif
#undef FA_RP16_ITEM_OF

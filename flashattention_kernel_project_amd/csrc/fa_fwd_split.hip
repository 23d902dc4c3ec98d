// fa_fwd_split.hip -- attention forward with Nq != Nk and a split over the keys ("flash-decoding").
//
// SURVEY.md 8(f) rank 1, third part; not a reference entry point (the reference's kernels are
// self-attention, Nq == Nk; its single-query experiment is
// flashattn_warp_spc/../flashattn_streaming_16x16_mw_v7_5*.cu).  Use: few query rows against a long
// K/V (decode), where one workgroup per (head, query block) cannot fill 256 CUs and the job is to
// stream K and V once at HBM rate.
//
//   pass 1  fa_fwd_split_kernel: grid = BH x query blocks x S.  Workgroup (bh, qb, s) runs the tiled
//           stream of fa_fwd_kernels.hip (same LDS images, MFMA orientation, lazy running max) over
//           the keys [s*chunk, (s+1)*chunk) and writes the UNNORMALISED O^T (fp32), the reference max
//           m (log2 units) and the row sum l of its split to the caller's workspace
//           [BH][S][Nq][D + 2] fp32 (m and l in the two trailing slots of a row).
//   pass 2  fa_split_combine_kernel: per (bh, row): M = max_s m_s, L = sum_s l_s 2^(m_s - M),
//           O = sum_s O_s 2^(m_s - M) / L, written in the output dtype.
//   S == 1  pass 1 normalises and writes O directly; no workspace, no pass 2.
//
// 128-row workgroups (4 waves x 32 rows): query rows >= Nq read zeros and are not stored, so for a
// handful of query rows most MFMA work is idle lanes -- irrelevant here, the path is HBM-bound.
#include "fa_fwd_split_kernel.hpp"
#include "fa_dispatch.hpp"

#include <cstdlib>

namespace fa {

// ---- host side -------------------------------------------------------------------------------------
// Number of key splits: enough workgroups for about four per CU, at least 4 tiles per split.
int split_count(int BH, int Nq, int Nk)
{
    const long long base = (long long)BH * ((Nq + split::kRows - 1) / split::kRows);
    const int tiles = (Nk + kBlockN - 1) / kBlockN;
    constexpr int target = 1024, min_tiles = 4;   // workgroups in total, fewest tiles per split
    long long s = (target + base - 1) / base;   // about four workgroups per CU
    if (s > tiles / min_tiles) s = tiles / min_tiles;
    if (s < 1) s = 1;
    // every split must hold at least one key: chunk = ceil(tiles / s) tiles, recompute s from the chunk
    const int chunk_tiles = (int)((tiles + s - 1) / s);
    return (tiles + chunk_tiles - 1) / chunk_tiles;
}

size_t split_workspace_bytes(int BH, int Nq, int Nk, int D)
{
    const int S = split_count(BH, Nq, Nk);
    return S <= 1 ? 0 : (size_t)BH * S * Nq * (D + 2) * sizeof(float);
}

template <typename T, int D, bool kOutF32>
static hipError_t launch_split(const void* Q, const void* K, const void* V, void* O, void* ws, size_t ws_bytes,
                               int BH, int Nq, int Nk, float scale, hipStream_t stream)
{
    using G = TileGeom<D>;
    const int S = split_count(BH, Nq, Nk);
    const int tiles = (Nk + kBlockN - 1) / kBlockN;
    const int chunk = ((tiles + S - 1) / S) * kBlockN;
    const int nqb = (Nq + split::kRows - 1) / split::kRows;
    const long long nwg = (long long)BH * nqb * S;
    if (nwg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (S > 1 && (!ws || ws_bytes < split_workspace_bytes(BH, Nq, Nk, D))) return hipErrorInvalidValue;
    const uint16_t *q = static_cast<const uint16_t*>(Q), *k = static_cast<const uint16_t*>(K), *v = static_cast<const uint16_t*>(V);
    hipError_t attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, false>), G::kLdsBytes);
    if (attr == hipSuccess) attr = ensure_dyn_lds(reinterpret_cast<const void*>(&fa_fwd_split_kernel<T, D, kOutF32, true>), G::kLdsBytes);
    if (attr != hipSuccess) return attr;
    if (S == 1) {
        FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, false>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                           stream, q, k, v, O, static_cast<float*>(nullptr), Nq, Nk, nqb, S, chunk, host_scale_log2e(scale));
        return launch_status();
    }
    FA_LAUNCH((fa_fwd_split_kernel<T, D, kOutF32, true>), dim3((unsigned)nwg), dim3(64 * split::kW), G::kLdsBytes,
                       stream, q, k, v, O, static_cast<float*>(ws), Nq, Nk, nqb, S, chunk, host_scale_log2e(scale));
    hipError_t e = launch_status();
    if (e != hipSuccess) return e;
    const long long rows = (long long)BH * Nq;   // one wave per output row
    if (rows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    FA_LAUNCH((fa_split_combine_kernel<T, kOutF32>), dim3((unsigned)rows), dim3(64), 0, stream,
                       static_cast<const float*>(ws), O, BH, Nq, D, S);
    return launch_status();
}

hipError_t split_dispatch(const void* Q, const void* K, const void* V, void* O, void* ws, size_t ws_bytes,
                          int BH, int Nq, int Nk, int D, float scale, int in_dtype, int out_dtype, hipStream_t stream)
{
    if (!Q || !K || !V || !O) return hipErrorInvalidValue;
    if (BH <= 0 || Nq <= 0 || Nk <= 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
    if (in_dtype != 0 && in_dtype != 1) return hipErrorInvalidValue;
    if (out_dtype != 0 && out_dtype != 1) return hipErrorInvalidValue;
    // per-head byte offsets are 32 bit (fp32 output / workspace rows of D+2 floats)
    if ((unsigned long long)(Nq + split::kRows) * (unsigned)(D + 2) * 4ull >= (1ull << 32)) return hipErrorInvalidValue;
    if ((unsigned long long)(Nk + kBlockN) * (unsigned)D * 2ull >= (1ull << 32)) return hipErrorInvalidValue;
    if (D == 64)
        return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
            return launch_split<decltype(t), 64, decltype(f32)::value>(Q, K, V, O, ws, ws_bytes, BH, Nq, Nk, scale, stream);
        });
    return with_types(in_dtype, out_dtype, [&](auto t, auto f32) {
        return launch_split<decltype(t), 128, decltype(f32)::value>(Q, K, V, O, ws, ws_bytes, BH, Nq, Nk, scale, stream);
    });
}

}  // namespace fa

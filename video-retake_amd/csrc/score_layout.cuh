// score_layout.cuh — host side: the layout of a unit's score workspace and the split geometry of the two passes, i.e.
// what the score entry points (pivotkv_score.hip) and the kernels that fill the workspace (pivotkv_prepare.hip) have to
// agree on.  Everything here depends on the shape and the dtype code only, so results are deterministic.
#pragma once
#include <algorithm>

#include "score_mfma.cuh"

namespace rtk {

// Work decomposition.  Both passes are cut into >= ~3000 workgroups (about 4 rounds over 256 CUs x 3
// resident workgroups) so the last round's tail stays small; the splits depend on the shape only,
// so results are deterministic.
constexpr int TARGET_WGS = 3072;
inline int pick_splits(int tiles_fixed, int heads, int stream_tiles, int cap, int Hkv) {
    int s = (TARGET_WGS + tiles_fixed * heads - 1) / (tiles_fixed * heads);
    s = std::max(1, std::min(std::min(s, cap), stream_tiles));
    // prefer a split count whose NON-EMPTY splits make Hkv*splits a multiple of the XCD count (balanced
    // XCD-aware mapping); splits are whole 64-row tiles, so check the effective count
    for (int t = s; t <= std::min(cap, stream_tiles) && t <= s + 8; ++t) {
        const int per = (((stream_tiles + t - 1) / t));          // tiles per split
        const int eff = (stream_tiles + per - 1) / per;
        if ((Hkv * eff) % NXCD == 0) return t;
    }
    return s;
}

struct ScoreWs {
    size_t q_off, k_off, lse_off, part_off, total;
    int RS, KS;            // split counts the buffers are sized for
    int kps, rps;          // keys per key split (pass 1) / query rows per row split (pass 2): whole 64-row tiles
    int ks_n, rs_n;        // the non-empty splits: what is launched, and what the partials hold
    bool f32;   // RTK_F32: fp32 payloads (everything else is 16-bit)
    bool ref;   // RTK_BF16_REFROUND / RTK_F16_REFROUND: the reference's rounding chain; column partials are per head
    bool fast;  // RTK_BF16_FAST: q~ (pre-scaled) and a second copy of k~ (at k_off) are fp16
    bool h16;   // RTK_F16 / RTK_F16_REFROUND: fp16 payloads (un-rotation rounds to fp16, the passes use the fp16 matrix instruction)
};
inline ScoreWs score_ws(int Hq, int Hkv, int L, int D, int dtype) {
    const bool many = (dtype & RTK_SCORE_MANY_UNITS) != 0;   // the caller batches many units per launch
    dtype &= ~RTK_SCORE_MANY_UNITS;
    const size_t es = dtype == RTK_F32 ? 4 : 2;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    ScoreWs w;
    w.f32 = dtype == RTK_F32;
    w.ref = dtype == RTK_BF16_REFROUND || dtype == RTK_F16_REFROUND;
    w.fast = dtype == RTK_BF16_FAST;
    w.h16 = dtype == RTK_F16 || dtype == RTK_F16_REFROUND;
    const int fixed_tiles = (L + REG_ROWS - 1) / REG_ROWS, stream_tiles = (L + TILE_ROWS - 1) / TILE_ROWS;
    w.RS = (D == HD) ? pick_splits(fixed_tiles, Hkv, stream_tiles, 32, Hkv) : 1;
    w.KS = (D == HD) ? pick_splits(fixed_tiles, Hq, stream_tiles, 8, Hkv) : 1;
    // bf16 production path: the chunk-batched launches bring their own parallelism (28 layers), so pass 1 prefers
    // longer key streams per workgroup (measured: 2 splits -1.7 % over 4) and half the lse partials
    if (D == HD && dtype != RTK_F32) w.KS = std::min(w.KS, 2);
    if (many && D == HD && dtype != RTK_F32) {
        // Launches of many units bring their own parallelism, so the splits are chosen for the length of a workgroup's
        // stream instead of for the workgroup count of ONE unit (same-box A/Bs at L = 2304 and 6272,
        // profiles/r06_ab_splits.txt): one key split (pass 1 -1.6 % / -0.4 %, no lse_combine launch), about eight row
        // tiles per row split (pass 2 -2 % at L = 2304; 14 splits of 7 tiles at L = 6272, what pick_splits gave already).
        w.KS = 1;
        const int s0 = std::max(1, (stream_tiles + 7) / 8);
        w.RS = s0;
        for (int t = s0; t <= std::min(stream_tiles, s0 + 8); ++t) {
            const int per = (stream_tiles + t - 1) / t, eff = (stream_tiles + per - 1) / per;
            if ((Hkv * eff) % NXCD == 0) { w.RS = t; break; }
        }
    }
    auto per_split = [](int n, int parts) { return (((n + parts - 1) / parts + TILE_ROWS - 1) / TILE_ROWS) * TILE_ROWS; };
    w.kps = per_split(L, w.KS);
    w.rps = per_split(L, w.RS);
    w.ks_n = (L + w.kps - 1) / w.kps;
    w.rs_n = (L + w.rps - 1) / w.rps;
    w.q_off = 0;
    w.k_off = al((size_t)Hq * L * D * es);
    w.lse_off = w.k_off + al((size_t)Hkv * L * D * es);
    w.part_off = w.lse_off + al((size_t)w.KS * Hq * L * 4);
    w.total = w.part_off + al((size_t)(w.ref ? Hq : Hkv) * w.RS * L * 4);
    return w;
}
// workgroups along the register operand: tiles of 128 rows x nb register blocks per wave
inline int reg_tiles(int L, int nb) { return (L + REG_ROWS * nb - 1) / (REG_ROWS * nb); }

}  // namespace rtk

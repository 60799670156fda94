// pivotkv_score.hip — PivotKV token scoring on gfx950: host dispatch and C ABI.  Replaces longvideo_cache.py:248-270:
//   un-rotate q,k (pos_embed_reforge) -> softmax(q k^T / sqrt(D)) over the CURRENT chunk's keys, no
//   mask -> column sums over queries -> mean over the G heads of a KV group -> mean over groups.
//
// The [Hq,L,L] probability tensor (4.4 GB fp32 at L = 6272) is never materialised.  The row
// normaliser has to be known before a column sum can be accumulated, so the contraction runs twice:
//   prepare  un-rotated, packed copies q~ [Hq,L,D], k~ [Hkv,L,D]          (pivotkv_prepare.hip: score_unrotate)
//   pass 1   per (head, query tile, key split): stream key tiles, row log-sum-exp     -> lse_part[ks,h,i]
//   combine  lse[h,i] over the key splits (lse_combine_kernel, only if there are several)
//   pass 2   per (kv group, key tile, row split): stream query tiles of the group's G heads,
//            p = exp(s - lse[h,i]), accumulate per-key column sums                    -> partial[g,split,j]
//   finalize fixed-order reduction of the partials (deterministic, no float atomics)  -> score[j]
// Roofline: MFMA-bound (2*Hq*L^2*D flop per pass, operands are a few MB and L2-resident).
// Kernels of the passes, by dtype code: score_dma.cuh (bf16 / fp16 payloads / RTK_BF16_FAST, head_dim 128: production),
// score_f32.cuh (fp32 parity path; any head_dim: generic), score_refround.cuh (the reference's 16-bit rounding chain).
// Workspace layout and split geometry: score_layout.cuh.
#include <atomic>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "score_dma.cuh"
#include "score_f32.cuh"
#include "score_layout.cuh"
#include "score_refround.cuh"

namespace rtk {

// lse[h,i] = log sum_ks exp(lse_part[ks,h,i]), written over split 0 (one thread per row: no hazard)
template <int DT>
__global__ __launch_bounds__(256) void lse_combine_kernel(float* __restrict__ lse_part, size_t n, int KS,
                                                          size_t unit_floats, int negate = 0) {
    lse_part += blockIdx.y * unit_floats;   // blockIdx.y = unit of a batched launch
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float v[8];
    float mx = -INFINITY;
    for (int s = 0; s < KS; ++s) {
        v[s] = lse_part[(size_t)s * n + idx];
        mx = fmaxf(mx, v[s]);
    }
    float tot = 0.f;
    for (int s = 0; s < KS; ++s) tot += (DT == RTK_BF16) ? __builtin_amdgcn_exp2f(v[s] - mx) : expf(v[s] - mx);
    const float out = mx + ((DT == RTK_BF16) ? __builtin_amdgcn_logf(tot) : logf(tot));
    lse_part[idx] = negate ? -out : out;   // RTK_BF16_FAST: pass 2 starts its accumulators from -lse
}

// finalize: score[j] = mean_g( (sum_split partial[g,split,j]) / G )      (longvideo_cache.py:269-270)
// Fixed summation order (bit-reproducible).  A workgroup owns 64 keys; its four waves take the KV groups
// g = wave, wave + 4, ... so that up to 4 x 8 loads per key are in flight, then wave 0 adds the per-group means
// in group order.
__global__ __launch_bounds__(256) void score_finalize_kernel(const float* __restrict__ partial, int Hkv, int RS, int G,
                                                             int L, float* __restrict__ score) {
    extern __shared__ float fin_gs[];  // [Hkv][64]
    const int jl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + jl;
    const int jc = min(j, L - 1);
    for (int g = part; g < Hkv; g += 4) {
        const float* p = partial + (size_t)g * RS * L + jc;
        float gs = 0.f;
        int r = 0;
        for (; r + 8 <= RS; r += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u) * L];
#pragma unroll
            for (int u = 0; u < 8; ++u) gs += v[u];
        }
        for (; r < RS; ++r) gs += p[(size_t)r * L];
        fin_gs[g * 64 + jl] = gs / (float)G;
    }
    __syncthreads();
    if (part == 0 && j < L) {
        float tot = 0.f;
        for (int g = 0; g < Hkv; ++g) tot += fin_gs[g * 64 + jl];
        score[j] = tot / (float)Hkv;
    }
}

}  // namespace rtk

using namespace rtk;

template <int V> using IC = std::integral_constant<int, V>;   // a compile-time int as a lambda argument

extern "C" size_t rtk_pivotkv_score_workspace_bytes(int Hq, int Hkv, int L, int D, int dtype) {
    if (Hq < 1 || Hkv < 1 || L < 1 || D < 1) return 0;
    return score_ws(Hq, Hkv, L, D, dtype).total;
}

extern "C" size_t rtk_pivotkv_score_partials(int Hq, int Hkv, int L, int D, int dtype, int* rs_out) {
    if (Hq < 1 || Hkv < 1 || L < 1 || D < 1) return 0;
    const ScoreWs w = score_ws(Hq, Hkv, L, D, dtype);
    if (rs_out) *rs_out = w.rs_n;   // the non-empty row splits score_impl launches
    return (size_t)(w.ref ? Hq : Hkv) * w.rs_n * L;
}

// The stages of one scoring call.  n_units > 1 (RTK_SCORE_PASSES of the 16-bit head_dim-128 kernels only): the same
// passes for n_units units whose workspaces / k~ / partials lie ws_stride / k_stride bytes and part_stride floats apart -
// one launch per kernel, blockIdx.y = unit.  q_view (LDS-DMA passes only, n_units <= MAX_Q_UNITS): the units' queries are
// read where the caller keeps them (per-unit pointers, head stride, row pitch) instead of from the packed copies inside
// the workspaces.
static int score_impl(const void* q, int64_t qsh, int64_t qsl, const void* k, int64_t ksh, int64_t ksl, int Hq,
                      int Hkv, int L, int D, const float* cosv, const float* sinv, float a, float* score,
                      void* k_unrot, char* ws, const ScoreWs& w, int stages, float* partial_out, hipStream_t st,
                      int n_units = 1, size_t ws_stride = 0, size_t k_stride = 0, size_t part_stride = 0,
                      const int* key_index = nullptr, const QView* q_view = nullptr) {
    QView qv;
    memset(&qv, 0, sizeof(qv));
    if (q_view) qv = *q_view;
    const char* qt = ws + w.q_off;
    const char* kt = (k_unrot && !w.fast) ? (char*)k_unrot : ws + w.k_off;   // FAST scores on the fp16 copy inside the workspace
    if (w.fast) k_stride = ws_stride;
    float* lse = (float*)(ws + w.lse_off);
    float* part = partial_out ? partial_out : (float*)(ws + w.part_off);
    if (stages & RTK_SCORE_PREPARE) {   // q~ -> the workspace; k~ -> k_unrot or the workspace (FAST: bf16 to k_unrot if given, fp16 to the workspace)
        const int rc = score_unrotate(w.f32 ? RTK_F32 : (w.h16 ? RTK_F16 : RTK_BF16), q, qsh, qsl, k, ksh, ksl, Hq, Hkv, L, D, cosv,
                                      sinv, a, ws + w.q_off, w.fast ? (char*)k_unrot : (char*)kt,
                                      w.fast ? ws + w.k_off : nullptr, st);
        if (rc) return rc;
    }
    if ((w.ref || w.fast) && D != HD) {
        set_error(w.ref ? "rtk_pivotkv_score: the reference-rounding modes need head_dim %d"
                        : "rtk_pivotkv_score: RTK_BF16_FAST needs head_dim %d", HD);
        return RTK_EUNSUPPORTED;
    }
    const int G = Hq / Hkv;
    const int ks_n = w.ks_n, rs_n = w.rs_n;
    const size_t su = ws_stride / sizeof(float);   // floats between the units' lse buffers
    const int x1 = (int)((Hkv * ks_n) % NXCD == 0), x2 = (int)((Hkv * rs_n) % NXCD == 0);   // balanced XCD-aware decode
    // dynamic LDS: two tiles, + two tiles' worth of row normalisers in pass 2
    constexpr int LDS16 = 2 * Tile<RTK_BF16>::BYTES, LDS32 = 2 * Tile<RTK_F32>::BYTES;
    constexpr int LDS_LSE = 2 * TILE_ROWS * (int)sizeof(float);
    auto combine = [&] {   // lse over the key splits, written over split 0
        const size_t n = (size_t)Hq * L;
        auto launch = [&](auto kern) {
            RTK_LAUNCH(KID_FINALIZE, kern, dim3((unsigned)((n + 255) / 256), n_units), dim3(256), 0, st, lse, n, ks_n, su, (int)w.fast);
        };
        if (ks_n <= 1) return;
        if (w.f32) launch(lse_combine_kernel<RTK_F32>);
        else launch(lse_combine_kernel<RTK_BF16>);
    };
    const bool passes = (stages & RTK_SCORE_PASSES) != 0;
    if (passes && w.ref) {
        // raw row sums + the fix-up launch for rows whose sum left fp32's range, lse combine over key splits, then the
        // column sums of the 16-bit probabilities per head
        const int jt = reg_tiles(L, REF_NB), jt2 = reg_tiles(L, REF_NB2), n_tiles = Hkv * ks_n * jt * G;
        const dim3 g1(n_tiles, n_units), gf((n_tiles + FIX_TILES - 1) / FIX_TILES, n_units), g2(Hkv * rs_n * jt2, n_units);
        const float sqrt_d = (float)sqrt((double)HD);   // python: math.sqrt(self.head_dim), then an fp32 opmath scalar
        const float rcp_sd = 1.0f / sqrt_d;
        auto ref_passes = [&](auto div, auto f16) {
            constexpr int DIV = decltype(div)::value;
            constexpr bool F16 = decltype(f16)::value != 0;
            RTK_LAUNCH(KID_PASS1, (score_pass1_ref_kernel<DIV, F16>), g1, dim3(SC_BLOCK), LDS16, st, qt, kt, Hq, Hkv, L, w.kps, jt,
                       x1, lse, ws_stride, k_stride, su, sqrt_d, rcp_sd);
            RTK_LAUNCH(KID_FINALIZE, (score_pass1_ref_fixup_kernel<DIV, F16>), gf, dim3(SC_BLOCK), LDS16, st, qt, kt, Hq, Hkv, L,
                       w.kps, jt, n_tiles, lse, ws_stride, k_stride, su, sqrt_d, rcp_sd);
            combine();
            RTK_LAUNCH(KID_PASS2, (score_pass2_ref_kernel<DIV, F16>), g2, dim3(SC_BLOCK), LDS16 + LDS_LSE, st, qt, kt,
                       (const float*)lse, Hq, Hkv, L, w.rps, jt2, rs_n, x2, part, ws_stride, k_stride, su, part_stride, sqrt_d,
                       rcp_sd, key_index);
        };
        if (w.h16) ref_passes(IC<2>{}, IC<1>{});   // fp16 payloads: IEEE division
        else if (bf16_rcp_is_exact(sqrt_d)) ref_passes(IC<1>{}, IC<0>{});
        else ref_passes(IC<2>{}, IC<0>{});
        RTK_LAUNCH_CHECK("score_ref_passes");
    } else if (passes && D != HD) {   // any head_dim: plain VALU
        auto generic = [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            RTK_LAUNCH(KID_PASS1, score_pass1_generic<DT>, dim3(L, Hq), dim3(256), D * sizeof(float), st, (const void*)qt,
                       (const void*)kt, Hq, Hkv, L, D, lse);
            RTK_LAUNCH(KID_PASS2, score_pass2_generic<DT>, dim3((L + 255) / 256, Hkv), dim3(256), D * sizeof(float), st,
                       (const void*)qt, (const void*)kt, (const float*)lse, Hq, Hkv, L, D, part);
        };
        if (w.f32) generic(IC<RTK_F32>{});
        else if (w.h16) generic(IC<RTK_F16>{});
        else generic(IC<RTK_BF16>{});
        RTK_LAUNCH_CHECK("score_generic");
    } else if (passes && w.f32) {   // the parity dtype: the register-staged kernels
        // > 64 KiB of dynamic LDS needs an opt-in per kernel AND per device: remembered in one atomic bit per device -
        // racing first calls both opt in, which is harmless
        static std::atomic<uint64_t> opted;
        int dev_id = 0;
        (void)hipGetDevice(&dev_id);
        const uint64_t dev_bit = 1ull << (dev_id & 63);
        if (!(opted.load(std::memory_order_relaxed) & dev_bit)) {
            (void)hipFuncSetAttribute((const void*)score_pass1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS32);
            (void)hipFuncSetAttribute((const void*)score_pass2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS32 + LDS_LSE);
            opted.fetch_or(dev_bit, std::memory_order_relaxed);
        }
        const int jt = reg_tiles(L, F32_NB);
        RTK_LAUNCH(KID_PASS1, score_pass1_kernel, dim3(Hkv * ks_n * jt * G), dim3(SC_BLOCK), LDS32, st, qt, kt, Hq, Hkv, L, w.kps,
                   jt, x1, lse);
        RTK_LAUNCH_CHECK("score_pass1_kernel");
        combine();
        RTK_LAUNCH(KID_PASS2, score_pass2_kernel, dim3(Hkv * rs_n * jt), dim3(SC_BLOCK), LDS32 + LDS_LSE, st, qt, kt,
                   (const float*)lse, Hq, Hkv, L, w.rps, jt, rs_n, x2, part, key_index);
        RTK_LAUNCH_CHECK("score_pass2_kernel");
    } else if (passes) {   // bf16 / fp16 payloads: the LDS-DMA kernels
        // raw row sums + a fix-up launch (1/32 of the grid) for the rows whose sum left fp32's range; the fast mode's
        // pass 2 starts its accumulators from -lse, so whoever writes the final lse negates it
        const int jt1 = reg_tiles(L, P1_NB), jt2 = reg_tiles(L, P2_NB), n_tiles = Hkv * ks_n * jt1 * G;
        const dim3 g1(n_tiles, n_units), gf((n_tiles + FIX_TILES - 1) / FIX_TILES, n_units), g2(Hkv * rs_n * jt2, n_units);
        const int neg = (int)(w.fast && ks_n == 1);
        auto pass1 = [&](auto mode) {   // mode: the P1_* flags of the operands
            constexpr int MODE = decltype(mode)::value;
            RTK_LAUNCH(KID_PASS1, (score_pass1_dma_kernel<P1_NB, MODE | P1_RAW>), g1, dim3(SC_BLOCK), LDS16, st, qt, kt, Hq, Hkv, L,
                       w.kps, jt1, x1, lse, ws_stride, k_stride, su, neg, qv);
            RTK_LAUNCH(KID_FINALIZE, (score_pass1_fixup_kernel<P1_NB, MODE>), gf, dim3(SC_BLOCK), LDS16, st, qt, kt, Hq, Hkv, L,
                       w.kps, jt1, n_tiles, lse, ws_stride, k_stride, su, neg, qv);
        };
        auto pass2 = [&](auto kern) {
            RTK_LAUNCH(KID_PASS2, kern, g2, dim3(SC_BLOCK), LDS16 + LDS_LSE, st, qt, kt, (const float*)lse, Hq, Hkv, L, w.rps, jt2,
                       rs_n, x2, part, ws_stride, k_stride, su, part_stride, key_index, qv);
        };
        if (w.fast) pass1(IC<P1_F16 | P1_SCALED>{});
        else if (w.h16) pass1(IC<P1_F16>{});
        else pass1(IC<0>{});
        RTK_LAUNCH_CHECK("score_pass1_kernel");
        combine();
        if (w.fast) pass2(score_pass2_dma_kernel<P2_NB, true, false>);
        else if (w.h16) pass2(score_pass2_dma_kernel<P2_NB, false, true>);
        else pass2(score_pass2_dma_kernel<P2_NB, false, false>);
        RTK_LAUNCH_CHECK("score_pass2_kernel");
    }
    if (stages & RTK_SCORE_FINALIZE) {
        if (w.ref) {   // the reference's three 16-bit roundings after the per-head sums
            auto launch = [&](auto kern) {
                RTK_LAUNCH(KID_FINALIZE, kern, dim3((L + 255) / 256), dim3(256), 0, st, (const float*)part, Hkv, rs_n, G, L, score);
            };
            if (w.h16) launch(score_finalize_ref_kernel<true>);
            else launch(score_finalize_ref_kernel<false>);
        } else {
            RTK_LAUNCH(KID_FINALIZE, score_finalize_kernel, dim3((L + 63) / 64), dim3(256), (size_t)Hkv * 64 * sizeof(float), st,
                       (const float*)part, Hkv, rs_n, G, L, score);
        }
        RTK_LAUNCH_CHECK("score_finalize_kernel");
    }
    return RTK_OK;
}

// Live keys of pass 2: key_compact_kernel for n units whose key-patch masks (device pointers, NULL = no mask) are listed
// on the host; *key_index = key_index_ws if a list was written, else NULL (no mask anywhere: all columns are computed).
static int compact_keys(const void* const* masks_host, int n, int L, int32_t* key_index_ws, hipStream_t st,
                        const int** key_index) {
    *key_index = nullptr;
    if (!masks_host || !key_index_ws) return RTK_OK;
    bool any = false;
    for (int u = 0; u < n; ++u) any = any || masks_host[u];
    if (!any) return RTK_OK;
    for (int u0 = 0; u0 < n; u0 += MAX_MASK_UNITS) {   // the pointer table travels as a kernel argument
        KeyMasks km;
        const int m = std::min(MAX_MASK_UNITS, n - u0);
        for (int u = 0; u < MAX_MASK_UNITS; ++u) km.m[u] = u < m ? (const uint8_t*)masks_host[u0 + u] : nullptr;
        RTK_LAUNCH(KID_FINALIZE, key_compact_kernel, dim3(m), dim3(1024), 0, st, km, L, key_index_ws + (size_t)u0 * (L + 1));
    }
    RTK_LAUNCH_CHECK("key_compact_kernel");
    *key_index = key_index_ws;
    return RTK_OK;
}

extern "C" int rtk_pivotkv_score_passes_batched_q(void* workspace0, size_t workspace_stride, void* k_unrot0,
                                                  size_t k_unrot_stride, float* partial0, size_t partial_stride_floats,
                                                  int n_units, int Hq, int Hkv, int L, int D, int dtype,
                                                  const void* const* key_masks_host, int32_t* key_index_ws,
                                                  const void* const* q_units_host, int64_t q_stride_h, int64_t q_stride_l,
                                                  rtk_stream_t stream) {
    const int base = dtype & ~RTK_SCORE_MANY_UNITS;   // (the flag: split policy, see score_ws)
    RTK_CHECK_ARG(workspace0 && partial0 && n_units >= 1, "rtk_pivotkv_score_passes_batched: NULL pointer or no units");
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Hq % Hkv == 0 && L >= 1, "rtk_pivotkv_score_passes_batched: bad shape");
    RTK_CHECK_ARG(((uintptr_t)workspace0 & 255) == 0 && workspace_stride % 256 == 0,
                  "rtk_pivotkv_score_passes_batched: workspaces must be 256-byte aligned");
    const ScoreWs w = score_ws(Hq, Hkv, L, D, dtype);
    RTK_CHECK_ARG(n_units == 1 || workspace_stride >= w.total, "rtk_pivotkv_score_passes_batched: workspace stride too small");
    if ((base != RTK_BF16 && base != RTK_BF16_REFROUND && base != RTK_BF16_FAST && base != RTK_F16 && base != RTK_F16_REFROUND) || D != HD) {
        set_error("rtk_pivotkv_score_passes_batched: bf16 / fp16 payloads with head_dim %d only (call RTK_SCORE_PASSES per unit)", HD);
        return RTK_EUNSUPPORTED;
    }
    if (q_units_host) {   // queries read in place: the exact LDS-DMA kernels, k~ outside the workspaces
        RTK_CHECK_ARG(k_unrot0, "rtk_pivotkv_score_passes_batched_q: NULL k_unrot");
        if (base != RTK_BF16 && base != RTK_F16) {
            set_error("rtk_pivotkv_score_passes_batched_q: RTK_BF16 / RTK_F16 only");
            return RTK_EUNSUPPORTED;
        }
        RTK_CHECK_ARG(q_stride_h > 0 && q_stride_l > 0 && (q_stride_h * 2) % 16 == 0 && (q_stride_l * 2) % 16 == 0 &&
                          (Hq - 1) * q_stride_h * 2 + (int64_t)(L - 1) * q_stride_l * 2 < (1ll << 31),
                      "rtk_pivotkv_score_passes_batched_q: bad query strides");
        for (int u = 0; u < n_units; ++u)
            RTK_CHECK_ARG(q_units_host[u] && ((uintptr_t)q_units_host[u] & 15) == 0,
                          "rtk_pivotkv_score_passes_batched_q: unit %d: queries must be 16-byte aligned", u);
    }
    // units whose key-patch mask is known skip the columns the mask override discards anyway
    const int* key_index = nullptr;
    int rc = compact_keys(key_masks_host, n_units, L, key_index_ws, (hipStream_t)stream, &key_index);
    if (rc) return rc;
    if (!k_unrot0) k_unrot_stride = workspace_stride;   // k~ inside the workspaces
    float dummy_score = 0.f;  // not touched by RTK_SCORE_PASSES
    // a query pointer table travels as a kernel argument: MAX_Q_UNITS units per launch
    const int per_call = q_units_host ? MAX_Q_UNITS : n_units;
    for (int u0 = 0; u0 < n_units && !rc; u0 += per_call) {
        const int m = std::min(per_call, n_units - u0);
        QView qv;
        memset(&qv, 0, sizeof(qv));
        if (q_units_host) {
            for (int u = 0; u < m; ++u) qv.unit[u] = (const char*)q_units_host[u0 + u];
            qv.head_stride = (int)(q_stride_h * 2);
            qv.row_pitch = (int)(q_stride_l * 2);
        }
        char* ws_u = (char*)workspace0 + (size_t)u0 * workspace_stride;
        rc = score_impl(ws_u, 0, 0, ws_u, 0, 0, Hq, Hkv, L, D, nullptr, nullptr, 1.0f, &dummy_score,
                        k_unrot0 ? (char*)k_unrot0 + (size_t)u0 * k_unrot_stride : nullptr, ws_u, w, RTK_SCORE_PASSES,
                        partial0 + (size_t)u0 * partial_stride_floats, (hipStream_t)stream, m, workspace_stride, k_unrot_stride,
                        partial_stride_floats, key_index ? key_index + (size_t)u0 * (L + 1) : nullptr, q_units_host ? &qv : nullptr);
    }
    return rc;
}

extern "C" int rtk_pivotkv_score_passes_batched(void* workspace0, size_t workspace_stride, void* k_unrot0,
                                                size_t k_unrot_stride, float* partial0, size_t partial_stride_floats,
                                                int n_units, int Hq, int Hkv, int L, int D, int dtype,
                                                const void* const* key_masks_host, int32_t* key_index_ws,
                                                rtk_stream_t stream) {
    return rtk_pivotkv_score_passes_batched_q(workspace0, workspace_stride, k_unrot0, k_unrot_stride, partial0,
                                              partial_stride_floats, n_units, Hq, Hkv, L, D, dtype, key_masks_host,
                                              key_index_ws, nullptr, 0, 0, stream);
}

extern "C" int rtk_pivotkv_score_stages_masked(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k,
                                               int64_t k_stride_h, int64_t k_stride_l, int Hq, int Hkv, int L, int D,
                                               int dtype, const float* cosv, const float* sinv, float attention_scaling,
                                               float* score, void* k_unrot, void* workspace, size_t workspace_bytes,
                                               int stages, float* partial_out, const void* key_mask,
                                               int32_t* key_index_ws, rtk_stream_t stream) {
    const int dtype_full = dtype;              // may carry RTK_SCORE_MANY_UNITS (split policy, see score_ws)
    dtype &= ~RTK_SCORE_MANY_UNITS;
    RTK_CHECK_ARG(q && k && score && workspace, "rtk_pivotkv_score: NULL pointer");
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Hq % Hkv == 0, "rtk_pivotkv_score: Hq=%d must be a multiple of Hkv=%d", Hq, Hkv);
    RTK_CHECK_ARG(L >= 1 && D >= 2 && D % 2 == 0, "rtk_pivotkv_score: bad shape L=%d D=%d", L, D);
    RTK_CHECK_ARG((cosv == nullptr) == (sinv == nullptr), "rtk_pivotkv_score: cos and sin must both be given or both NULL");
    RTK_CHECK_ARG(dtype == RTK_F32 || dtype == RTK_BF16 || dtype == RTK_BF16_REFROUND || dtype == RTK_BF16_FAST ||
                      dtype == RTK_F16 || dtype == RTK_F16_REFROUND, "rtk_pivotkv_score: unsupported dtype %d", dtype);
    RTK_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "rtk_pivotkv_score: workspace must be 256-byte aligned");
    RTK_CHECK_ARG(stages > 0 && stages <= 7, "rtk_pivotkv_score: stages mask %d out of range", stages);
    const ScoreWs w = score_ws(Hq, Hkv, L, D, dtype_full);
    if (workspace_bytes < w.total) {
        set_error("rtk_pivotkv_score: workspace %zu < required %zu bytes", workspace_bytes, w.total);
        return RTK_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    // live keys of pass 2 (head_dim 128 kernels only): the columns of masked tokens are not computed, the caller's
    // selection overwrites their score with 1.0 anyway (longvideo_cache.py:272-274)
    const int* key_index = nullptr;
    if (D == HD && (stages & RTK_SCORE_PASSES)) {
        const int rc = compact_keys(&key_mask, 1, L, key_index_ws, st, &key_index);
        if (rc) return rc;
    }
    return score_impl(q, q_stride_h, q_stride_l, k, k_stride_h, k_stride_l, Hq, Hkv, L, D, cosv, sinv, attention_scaling, score,
                      k_unrot, (char*)workspace, w, stages, partial_out, st, 1, 0, 0, 0, key_index);
}

extern "C" int rtk_pivotkv_score_stages(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k,
                                        int64_t k_stride_h, int64_t k_stride_l, int Hq, int Hkv, int L, int D, int dtype,
                                        const float* cosv, const float* sinv, float attention_scaling, float* score,
                                        void* k_unrot, void* workspace, size_t workspace_bytes, int stages,
                                        float* partial_out, rtk_stream_t stream) {
    return rtk_pivotkv_score_stages_masked(q, q_stride_h, q_stride_l, k, k_stride_h, k_stride_l, Hq, Hkv, L, D, dtype, cosv,
                                           sinv, attention_scaling, score, k_unrot, workspace, workspace_bytes, stages,
                                           partial_out, nullptr, nullptr, stream);
}

extern "C" int rtk_pivotkv_score(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k,
                                 int64_t k_stride_h, int64_t k_stride_l, int Hq, int Hkv, int L, int D, int dtype,
                                 const float* cosv, const float* sinv, float attention_scaling, float* score,
                                 void* k_unrot, void* workspace, size_t workspace_bytes, rtk_stream_t stream) {
    return rtk_pivotkv_score_stages(q, q_stride_h, q_stride_l, k, k_stride_h, k_stride_l, Hq, Hkv, L, D, dtype, cosv, sinv,
                                    attention_scaling, score, k_unrot, workspace, workspace_bytes,
                                    RTK_SCORE_PREPARE | RTK_SCORE_PASSES | RTK_SCORE_FINALIZE, nullptr, stream);
}

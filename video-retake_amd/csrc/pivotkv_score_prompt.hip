// pivotkv_score_prompt.hip — prompt-guided PivotKV scoring on gfx950 (kvcache_compression_kwargs["prompt_guided_scoring"];
// not in the reference, whose PivotKVCache.before_forward ignores prompt_length).  A chunk of L rows is Lv video rows
// followed by the Lp rows of the appended prompt; the video keys are scored by the prompt's queries alone:
//   score[j] = mean_g mean_{h in g} (1/Lp) sum_{i in [Lv,L)} softmax_{j' in [0,Lv)}(q~[h,i] . k~[g,j'] / sqrt(D))[j],  j < Lv
// No causal mask, prompt keys are never read, entries >= Lv of the output are never written.  The contraction is
// Hq*Lp*Lv*D instead of Hq*L*L*D: a thin problem (few rows, many keys), so the row operand is PACKED - the G*Lp query
// rows of a KV group (all G heads of the group share its keys) are numbered r = hh*Lp + i and cut into 32-row blocks,
// the B operand of v_mfma_f32_32x32x16 (S^T = K Q^T as in attention.hip).  Lp = 1 with G = 7 is one block per group, not a
// 128-row tile per head.  The loads, the block step and the merges are score_thin.cuh's, shared with pivotkv_rescore.hip.
// Two launches, no atomics, every sum in an order that depends on the shape alone:
//   prompt_lse_kernel     grid (row blocks, Hkv, units): the block's 4 waves stream the group's video keys (32-key blocks,
//                         wave w takes blocks w, w+4, ..; straight from L2 into MFMA A fragments, next block in flight), each
//                         lane keeps the online (max, sum) of ONE packed row, base-2; halves, then waves are merged in
//                         order -> lse2[g][r] (+inf for the rows that pad the last block: their probabilities are 0)
//   prompt_colsum_kernel  grid (ceil(Lv/128), units): a wave keeps 32 keys of one group as the B operand, streams the
//                         group's row blocks as A, col += exp2(s*c - lse2[r]); groups in order, /G, /Hkv, /Lp -> score[j]
// Arithmetic of score_rounding="fp32": exact products of the 16-bit operands, fp32 accumulation, softmax and sums.
// fp32 payloads or head_dim != 128: the *_generic kernels (plain FMA, natural exp, dot / sqrt(D)): the parity path.
#include <cstring>

#include "score_thin.cuh"

namespace rtk {

constexpr int PS_MAX_UNITS = 28;   // (layer, chunk) units per call
struct PromptUnits {
    const char* q[PS_MAX_UNITS];   // the units' query tensors (packed q~ inside the workspace, or the caller's)
};

// this lane's fragment of packed row r = rb*32 + (lane & 31) of KV group g: head g*G + r / Lp, prompt row r % Lp (qp: the
// unit's queries from chunk row Lv on)
__device__ __forceinline__ void load_prompt_rows(u32x4* f, const char* qp, int g, int G, int rb, int Lp, int64_t qsh,
                                                 int64_t qpitch, int lane) {
    const u32x4* p;
    const bool ok = packed_row(p, qp, g, G, Lp, rb * 32 + (lane & 31), qsh, qpitch);
    load_frag(f, p, ok, lane >> 5);
}

template <bool F16>
__global__ __launch_bounds__(SC_BLOCK) void prompt_lse_kernel(PromptUnits pu, const char* __restrict__ k0, size_t k_unit_bytes,
                                                              float* __restrict__ lse0, size_t lse_unit_floats, int G, int L,
                                                              int Lv, int Lp, int64_t qsh, int64_t qpitch, int RB, float c2) {
    __shared__ float2 red[4][32];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, hf = lane >> 5, row = lane & 31;
    const int rb = blockIdx.x, g = blockIdx.y, u = blockIdx.z;
    u32x4 qf[8];
    load_prompt_rows(qf, pu.q[u] + (int64_t)Lv * qpitch, g, G, rb, Lp, qsh, qpitch, lane);
    const char* kg = k0 + (size_t)u * k_unit_bytes + (size_t)g * L * (HD * 2);
    const int nkb = (Lv + 31) / 32;
    float m = -INFINITY, sum = 0.f;
    u32x4 a[8], an[8];
    load_key_frag(a, kg, wid * 32, Lv, lane);
    for (int kb = wid; kb < nkb; kb += 4) {
        load_key_frag(an, kg, (kb + 4) * 32, Lv, lane);   // (past the end: nothing is read)
        lse_step<F16, true>(a, qf, c2, kb * 32, Lv, hf, m, sum);   // (every block is masked: only the last needs it)
#pragma unroll
        for (int x = 0; x < 8; ++x) a[x] = an[x];
    }
    // the two halves of the wave, then the four waves, in wave order
    const float2 half = merge_halves(m, sum, hf);
    if (hf == 0) red[wid][row] = half;
    __syncthreads();
    if (tid < 32) {
        const int r = rb * 32 + tid;
        const float2 ms = merge_in_order<true>(4, [&](int w) { return red[w][tid]; });
        lse0[(size_t)u * lse_unit_floats + (size_t)g * RB * 32 + r] = r < G * Lp ? lse_of<true>(ms) : INFINITY;
    }
}

template <bool F16>
__global__ __launch_bounds__(SC_BLOCK) void prompt_colsum_kernel(PromptUnits pu, const char* __restrict__ k0, size_t k_unit_bytes,
                                                                 const float* __restrict__ lse0, size_t lse_unit_floats,
                                                                 float* __restrict__ score0, size_t score_unit_floats, int Hkv,
                                                                 int G, int L, int Lv, int Lp, int64_t qsh, int64_t qpitch,
                                                                 int RB, float c2) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, hf = lane >> 5;
    const int u = blockIdx.y;
    const int j0 = blockIdx.x * REG_ROWS + wid * 32;
    if (j0 >= Lv) return;   // wave-uniform; the kernel has no barrier
    const int j = j0 + (lane & 31);
    const char* qp = pu.q[u] + (int64_t)Lv * qpitch;
    const float* lse = lse0 + (size_t)u * lse_unit_floats;
    float tot = 0.f;
    for (int g = 0; g < Hkv; ++g) {
        u32x4 kf[8];
        load_key_frag(kf, k0 + (size_t)u * k_unit_bytes + (size_t)g * L * (HD * 2), j0, Lv, lane);
        const float* lg = lse + (size_t)g * RB * 32;
        float col = 0.f;
        u32x4 a[8], an[8];
        load_prompt_rows(a, qp, g, G, 0, Lp, qsh, qpitch, lane);
        for (int rb = 0; rb < RB; ++rb) {
            load_prompt_rows(an, qp, g, G, rb + 1, Lp, qsh, qpitch, lane);   // (past the end: nothing is read)
            float ls[16];
            load_ls(ls, lg, rb, hf);
            f32x16 acc = f32x16{0};
#pragma unroll
            for (int x = 0; x < 8; ++x) mma16<F16>(acc, a[x], kf[x], acc);   // acc[r] = q[rb*32 + acc_row(r, hf)] . k[j]
#pragma unroll
            for (int r = 0; r < 16; ++r) col += __builtin_amdgcn_exp2f(__fsub_rn(__fmul_rn(acc[r], c2), ls[r]));
#pragma unroll
            for (int x = 0; x < 8; ++x) a[x] = an[x];
        }
        col += __shfl_xor(col, 32, WAVE);
        tot += __fdiv_rn(col, (float)G);
    }
    if (hf == 0 && j < Lv) score0[(size_t)u * score_unit_floats + j] = __fdiv_rn(__fdiv_rn(tot, (float)Hkv), (float)Lp);
}

// ---- any head_dim, any payload: plain FMA, the reference's operation order (score_thin.cuh) --------------------------------
// lse[h*Lp + i] of prompt row i of head h over the video keys: grid (Hq*Lp, units)
template <int DT>
__global__ __launch_bounds__(256) void prompt_lse_generic(PromptUnits pu, const char* __restrict__ k0, size_t k_unit_bytes,
                                                          float* __restrict__ lse0, size_t lse_unit_floats, int G, int L, int Lv,
                                                          int Lp, int D, int64_t qsh, int64_t qpitch) {
    extern __shared__ float qs[];  // [D]
    const int u = blockIdx.y, h = blockIdx.x / Lp, i = blockIdx.x - h * Lp, g = h / G;
    const char* qrow = pu.q[u] + (int64_t)h * qsh + (int64_t)(Lv + i) * qpitch;
    const float2 ms = range_softmax<DT>(qs, qrow, k0 + (size_t)u * k_unit_bytes, (size_t)g * L, 0, Lv, D);
    if (threadIdx.x == 0) lse0[(size_t)u * lse_unit_floats + blockIdx.x] = lse_of<false>(ms);
}

// score[j]: one thread per video key, every prompt row of every head in turn: grid (ceil(Lv/256), units)
template <int DT>
__global__ __launch_bounds__(256) void prompt_colsum_generic(PromptUnits pu, const char* __restrict__ k0, size_t k_unit_bytes,
                                                             const float* __restrict__ lse0, size_t lse_unit_floats,
                                                             float* __restrict__ score0, size_t score_unit_floats, int Hkv, int G,
                                                             int L, int Lv, int Lp, int D, int64_t qsh, int64_t qpitch) {
    extern __shared__ float qs[];  // [D]
    const int u = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const float* lse = lse0 + (size_t)u * lse_unit_floats;
    float tot = 0.f;
    for (int g = 0; g < Hkv; ++g) {
        const float col = column_sum<DT>(
            qs, k0 + (size_t)u * k_unit_bytes, ((size_t)g * L + j) * D, j < Lv, G, Lp, D,
            [&](int hh, int i) { return pu.q[u] + (int64_t)(g * G + hh) * qsh + (int64_t)(Lv + i) * qpitch; },
            [&](int hh, int i) { return lse[(size_t)(g * G + hh) * Lp + i]; });
        tot += __fdiv_rn(col, (float)G);   // per group /G, then /Hkv, then /Lp: three roundings, in this order
    }
    if (j < Lv) score0[(size_t)u * score_unit_floats + j] = __fdiv_rn(__fdiv_rn(tot, (float)Hkv), (float)Lp);
}

}  // namespace rtk

using namespace rtk;

extern "C" size_t rtk_pivotkv_score_prompt_workspace_bytes(int Hq, int Hkv, int L, int Lp, int D, int dtype) {
    const int base = dtype & ~RTK_SCORE_MANY_UNITS;
    if (Hq < 1 || Hkv < 1 || Hq % Hkv || D < 1 || Lp < 1 || Lp >= L) return 0;
    const size_t floats = thin_mfma_path(base, D) ? (size_t)Hkv * packed_row_blocks(Hq / Hkv, Lp) * 32 : (size_t)Hq * Lp;
    return (floats * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int rtk_pivotkv_score_prompt_batched(void* workspace0, size_t workspace_stride, void* k_unrot0,
                                                size_t k_unrot_stride, float* score0, size_t score_stride_floats,
                                                void* scratch0, size_t scratch_stride, int n_units, int Hq, int Hkv, int L,
                                                int Lp, int D, int dtype, const void* const* q_units_host,
                                                int64_t q_stride_h, int64_t q_stride_l, rtk_stream_t stream) {
    const int base = dtype & ~RTK_SCORE_MANY_UNITS;
    RTK_CHECK_ARG(score0 && scratch0, "rtk_pivotkv_score_prompt_batched: NULL score or scratch");
    RTK_CHECK_ARG(n_units >= 1 && n_units <= PS_MAX_UNITS, "rtk_pivotkv_score_prompt_batched: %d units (1 .. %d per call)",
                  n_units, PS_MAX_UNITS);
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Hq % Hkv == 0 && D >= 1, "rtk_pivotkv_score_prompt_batched: bad shape");
    RTK_CHECK_ARG(Lp >= 1 && Lp < L, "rtk_pivotkv_score_prompt_batched: prompt rows %d must lie in 1 .. L - 1 = %d", Lp, L - 1);
    if (!payload_dtype(base)) {
        set_error("rtk_pivotkv_score_prompt_batched: the fp32 score arithmetic only (RTK_F32 / RTK_BF16 / RTK_F16), got %d", base);
        return RTK_EUNSUPPORTED;
    }
    RTK_CHECK_ARG(workspace0 || (k_unrot0 && q_units_host), "rtk_pivotkv_score_prompt_batched: NULL workspace");
    RTK_CHECK_ARG(!workspace0 || (((uintptr_t)workspace0 & 255) == 0 && workspace_stride % 256 == 0),
                  "rtk_pivotkv_score_prompt_batched: workspaces must be 256-byte aligned");
    const int Lv = L - Lp, G = Hq / Hkv;
    const size_t es = base == RTK_F32 ? 4 : 2;
    const size_t need = rtk_pivotkv_score_prompt_workspace_bytes(Hq, Hkv, L, Lp, D, dtype);
    RTK_CHECK_ARG(((uintptr_t)scratch0 & 255) == 0 && scratch_stride % 256 == 0 && (n_units == 1 || scratch_stride >= need),
                  "rtk_pivotkv_score_prompt_batched: scratch must be 256-byte aligned, %zu bytes per unit", need);
    RTK_CHECK_ARG(n_units == 1 || score_stride_floats >= (size_t)Lv, "rtk_pivotkv_score_prompt_batched: score stride < Lv");
    const ScoreWs w = score_ws(Hq, Hkv, L, D, dtype);
    RTK_CHECK_ARG(!workspace0 || n_units == 1 || workspace_stride >= w.total,
                  "rtk_pivotkv_score_prompt_batched: workspace stride too small");
    const bool mfma = thin_mfma_path(base, D);
    PromptUnits pu;
    memset(&pu, 0, sizeof(pu));
    int64_t qsh, qpitch;   // bytes
    if (q_units_host) {
        RTK_CHECK_ARG(q_stride_h > 0 && q_stride_l >= D, "rtk_pivotkv_score_prompt_batched: bad query strides");
        RTK_CHECK_ARG(!mfma || ((q_stride_h * 2) % 16 == 0 && (q_stride_l * 2) % 16 == 0),
                      "rtk_pivotkv_score_prompt_batched: query rows must be 16-byte aligned");
        for (int u = 0; u < n_units; ++u) {
            RTK_CHECK_ARG(q_units_host[u] && (!mfma || ((uintptr_t)q_units_host[u] & 15) == 0),
                          "rtk_pivotkv_score_prompt_batched: unit %d: queries must be 16-byte aligned", u);
            pu.q[u] = (const char*)q_units_host[u];
        }
        qsh = q_stride_h * (int64_t)es;
        qpitch = q_stride_l * (int64_t)es;
    } else {
        for (int u = 0; u < n_units; ++u) pu.q[u] = (const char*)workspace0 + (size_t)u * workspace_stride + w.q_off;
        qsh = (int64_t)L * D * (int64_t)es;
        qpitch = (int64_t)D * (int64_t)es;
    }
    const char* k0 = k_unrot0 ? (const char*)k_unrot0 : (const char*)workspace0 + w.k_off;
    const size_t k_unit = k_unrot0 ? k_unrot_stride : workspace_stride;
    RTK_CHECK_ARG(((uintptr_t)k0 & 15) == 0 && (n_units == 1 || k_unit >= (size_t)Hkv * L * D * es),
                  "rtk_pivotkv_score_prompt_batched: k~ must be 16-byte aligned, units at least Hkv*L*D elements apart");
    float* lse = (float*)scratch0;
    const size_t lse_unit = scratch_stride / sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (mfma) {
        const int RB = packed_row_blocks(G, Lp);
        const float c2 = logit_scale2(D);
        const dim3 g1(RB, Hkv, n_units), g2((Lv + REG_ROWS - 1) / REG_ROWS, n_units);
        with_f16(base, [&](auto f16) {
            constexpr bool F16 = decltype(f16)::value;
            RTK_LAUNCH(KID_PASS1, prompt_lse_kernel<F16>, g1, dim3(SC_BLOCK), 0, st, pu, k0, k_unit, lse, lse_unit, G, L, Lv, Lp,
                       qsh, qpitch, RB, c2);
            RTK_LAUNCH(KID_PASS2, prompt_colsum_kernel<F16>, g2, dim3(SC_BLOCK), 0, st, pu, k0, k_unit, (const float*)lse, lse_unit,
                       score0, score_stride_floats, Hkv, G, L, Lv, Lp, qsh, qpitch, RB, c2);
        });
    } else {
        RTK_CHECK_ARG((size_t)Hq * Lp < (1u << 31), "rtk_pivotkv_score_prompt_batched: too many prompt rows");
        const dim3 g1(Hq * Lp, n_units), g2((Lv + 255) / 256, n_units);
        with_payload(base, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            RTK_LAUNCH(KID_PASS1, prompt_lse_generic<DT>, g1, dim3(256), D * sizeof(float), st, pu, k0, k_unit, lse, lse_unit, G, L,
                       Lv, Lp, D, qsh, qpitch);
            RTK_LAUNCH(KID_PASS2, prompt_colsum_generic<DT>, g2, dim3(256), D * sizeof(float), st, pu, k0, k_unit, (const float*)lse,
                       lse_unit, score0, score_stride_floats, Hkv, G, L, Lv, Lp, D, qsh, qpitch);
            return 0;
        });
    }
    RTK_LAUNCH_CHECK("rtk_pivotkv_score_prompt_batched");
    return RTK_OK;
}

// score_thin.cuh — the steps of a THIN score contraction on gfx950: a handful of query rows against many keys of a region, no
// mask, which is what prompt-guided scoring (pivotkv_score_prompt.hip) and the budget's re-scoring (pivotkv_rescore.hip, and
// through it the question-focused cache) compute.  The kernels differ - prompt streams keys past resident query rows, the
// re-scoring keeps keys in registers and splits them into ranges - and stay in their files; what they share is written here
// once: the fragment loads (of 16-bit rows, and of e4m3 archive rows dequantised on the way), the packed-row numbering, the
// base-2 online (max, sum) of a 32-key block, the in-order merges with their -inf guards, the generic (parity) path's dot, range softmax and column loop, and the host's path predicates.
// Device and host helpers only, no kernels.  Every sum, product and rounding below is in an order the results are pinned to,
// bit for bit: exp2(fsub(fmul(acc, c2), .)) stays an fmul and an fsub (colsum_block of score_mfma.cuh contracts them to an
// fma; these kernels do not), merges run in index order.
#pragma once
#include <cmath>

#include "fp8kv.cuh"
#include "score_layout.cuh"

namespace rtk {

// element i of a payload array: fp32, or a 16-bit format widened
template <int DT>
__device__ __forceinline__ float ld_any(const void* p, size_t i) {
    if constexpr (DT != RTK_F32) return H16<DT>::ld(p, i);
    else return ((const float*)p)[i];
}

// ---- MFMA path: 16-bit rows of 128 channels; a lane's fragment of a row is its 16-byte chunks 2 x + (lane >> 5), x < 8 -------
// f[x * STRIDE] = chunk x of the fragment of row p, zeros if the row is not there (p is not read then)
template <int STRIDE = 1>
__device__ __forceinline__ void load_frag(u32x4* f, const u32x4* p, bool ok, int hf) {
#pragma unroll
    for (int x = 0; x < 8; ++x) f[x * STRIDE] = ok ? p[2 * x + hf] : u32x4{0, 0, 0, 0};
}
// this lane's fragment of key j0 + (lane & 31) of a group's rows [n, 128]; keys >= n are not read
__device__ __forceinline__ void load_key_frag(u32x4* f, const char* kg, int j0, int n, int lane) {
    const int j = j0 + (lane & 31);
    const bool ok = j < n;
    load_frag(f, (const u32x4*)(kg + (size_t)(ok ? j : 0) * (HD * 2)), ok, lane >> 5);
}
// The same fragment of a group's e4m3 rows (fp8kv.cuh): codes [n, 128] BYTES at kg, one scale per row at sg.  Chunk c of the
// 16-bit row is the 8 codes at byte 8 c, dequantised by rule 5 to DT - the registers load_key_frag fills from the dequantised
// row.  Keys >= n are not read, neither codes nor scales
template <int DT>
__device__ __forceinline__ void load_key_frag_fp8(u32x4* f, const char* kg, const float* sg, int j0, int n, int lane) {
    const int j = j0 + (lane & 31), hf = lane >> 5;
    const bool ok = j < n;
    const uint2* p = (const uint2*)(kg + (size_t)(ok ? j : 0) * HD);
    const float s = ok ? sg[j] : 1.f;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        const uint2 c = ok ? p[2 * x + hf] : uint2{0, 0};   // (code 0 is +0 at any scale: the zeros of load_frag)
        uint32_t w0, w1, w2, w3;
        fp8_dequant4<DT>(c.x, s, w0, w1);
        fp8_dequant4<DT>(c.y, s, w2, w3);
        f[x] = u32x4{w0, w1, w2, w3};
    }
}
// Packed row r = hh * rows + i of kv group g is row i of head g G + hh of q (byte strides qsh, qpitch); the G * rows rows of a
// group are cut into 32-row blocks.  false: r pads the last block (p is then a row that exists, and is not to be read)
__device__ __forceinline__ bool packed_row(const u32x4*& p, const char* q, int g, int G, int rows, int r, int64_t qsh,
                                           int64_t qpitch) {
    const bool ok = r < G * rows;
    const int hh = ok ? r / rows : 0, i = ok ? r - hh * rows : 0;
    p = (const u32x4*)(q + (int64_t)(g * G + hh) * qsh + (int64_t)i * qpitch);
    return ok;
}
inline int packed_row_blocks(int G, int rows) { return (G * rows + 31) / 32; }

// One 32-key block (fragments kf, its first key is key row0 of the caller's count) folded into the online (max, sum), base 2,
// of ONE packed row (this lane's, fragments qf): the lane's 16 logits.  MASKED: only keys < left count; a half-wave whose 16
// keys all lie past it has seen nothing yet
template <bool F16, bool MASKED>
__device__ __forceinline__ void lse_step(const u32x4* kf, const u32x4* qf, float c2, int row0, int left, int hf, float& m,
                                         float& sum) {
    f32x16 acc = f32x16{0};
#pragma unroll
    for (int x = 0; x < 8; ++x) mma16<F16>(acc, kf[x], qf[x], acc);   // acc[r] = k[row0 + acc_row(r, hf)] . q[row]
    float t[16];
    float mn = m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        t[r] = __fmul_rn(acc[r], c2);
        if constexpr (MASKED) t[r] = (row0 + acc_row(r, hf) < left) ? t[r] : -INFINITY;
        mn = fmaxf(mn, t[r]);
    }
    if (!MASKED || mn > -INFINITY) {
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) add += __builtin_amdgcn_exp2f(__fsub_rn(t[r], mn));
        sum = sum * __builtin_amdgcn_exp2f(__fsub_rn(m, mn)) + add;
        m = mn;
    }
}

// n partial (max, sum) of one row over disjoint keys, part(0) .. part(n - 1), merged in index order; a part that saw no key
// (max -inf) adds nothing.  BASE2: the MFMA path's log2 domain, else natural
template <bool BASE2, class Part>
__device__ __forceinline__ float2 merge_in_order(int n, Part&& part) {
    float mm = -INFINITY;
    for (int i = 0; i < n; ++i) mm = fmaxf(mm, part(i).x);
    float tot = 0.f;
    for (int i = 0; i < n; ++i) {
        const float2 v = part(i);
        if (v.x > -INFINITY) tot += v.y * (BASE2 ? __builtin_amdgcn_exp2f(v.x - mm) : expf(v.x - mm));
    }
    return make_float2(mm, tot);
}
// the two halves of a wave saw disjoint keys of the same row: lower half first
__device__ __forceinline__ float2 merge_halves(float m, float sum, int hf) {
    const float m2 = __shfl_xor(m, 32, WAVE), s2 = __shfl_xor(sum, 32, WAVE);
    const float2 lo = make_float2(hf ? m2 : m, hf ? s2 : sum), hi = make_float2(hf ? m : m2, hf ? sum : s2);
    return merge_in_order<true>(2, [&](int i) { return i ? hi : lo; });
}
// the log-sum-exp of a merged (max, sum)
template <bool BASE2>
__device__ __forceinline__ float lse_of(float2 ms) { return ms.x + (BASE2 ? __builtin_amdgcn_logf(ms.y) : logf(ms.y)); }

// ---- any head_dim, any payload: plain FMA, the reference's operation order (dot / sqrt(D), natural exp); 256 threads ----------
// query row `qrow` into LDS (qs [D]), for every thread of the block
template <int DT>
__device__ __forceinline__ void stage_query_row(float* qs, const char* qrow, int D) {
    for (int d = threadIdx.x; d < D; d += blockDim.x) qs[d] = ld_any<DT>(qrow, d);
    __syncthreads();
}
// qs . (the key row whose first element is element e0 of k) / sqrt(D)
template <int DT>
__device__ __forceinline__ float dot_row(const float* qs, const void* k, size_t e0, int D, float sqrt_d) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(qs[d], ld_any<DT>(k, e0 + d), s);
    return __fdiv_rn(s, sqrt_d);
}
// (max, sum), natural, of query row `qrow` over keys [j_begin, j_end) (key j is row row0 + j of k): a thread's keys in order,
// the wave's ladder, the four waves in order.  Thread 0 returns it, the others nothing of use
template <int DT>
__device__ __forceinline__ float2 range_softmax(float* qs, const char* qrow, const void* k, size_t row0, int j_begin, int j_end,
                                                int D) {
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    stage_query_row<DT>(qs, qrow, D);
    const float sqrt_d = sqrtf((float)D);
    float m = -INFINITY, sum = 0.f;
    for (int j = j_begin + tid; j < j_end; j += blockDim.x) {
        const float s = dot_row<DT>(qs, k, (row0 + j) * D, D, sqrt_d);
        const float mn = fmaxf(m, s);
        sum = sum * expf(m - mn) + expf(s - mn);
        m = mn;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, WAVE), s2 = __shfl_xor(sum, o, WAVE);
        const float mm = fmaxf(m, m2);
        if (mm > -INFINITY) sum = (m > -INFINITY ? sum * expf(m - mm) : 0.f) + (m2 > -INFINITY ? s2 * expf(m2 - mm) : 0.f);
        m = mm;
    }
    if ((tid & 63) == 0) red[tid / 64] = make_float2(m, sum);
    __syncthreads();
    return tid == 0 ? merge_in_order<false>(4, [&](int w) { return red[w]; }) : float2{0.f, 0.f};
}
// sum over the G * rows query rows of one kv group of exp(q . key / sqrt(D) - lse), the key row at element e0 of k: heads in
// order, a head's rows in order, two-level, 64 rows at a time (a plain running sum drifts).  qrow(hh, i): the row's address,
// lse(hh, i): its log-sum-exp.  Every thread of the block walks the loop (it stages the rows); `live`: this thread has a key
template <int DT, class QRow, class Lse>
__device__ __forceinline__ float column_sum(float* qs, const void* k, size_t e0, bool live, int G, int rows, int D, QRow&& qrow,
                                            Lse&& lse) {
    const float sqrt_d = sqrtf((float)D);
    float col = 0.f;
    for (int hh = 0; hh < G; ++hh) {
        float blk = 0.f;
        for (int i = 0; i < rows; ++i) {
            __syncthreads();   // the row before this one has been read
            stage_query_row<DT>(qs, qrow(hh, i), D);
            if (live) blk += expf(dot_row<DT>(qs, k, e0, D, sqrt_d) - lse(hh, i));
            if ((i & 63) == 63 || i + 1 == rows) {
                col += blk;
                blk = 0.f;
            }
        }
    }
    return col;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline bool payload_dtype(int dtype) {
    int es, ve;
    return payload_dims(dtype, es, ve);
}
// 16-bit payloads with head_dim 128 take the MFMA kernels, everything else the generic ones
inline bool thin_mfma_path(int dtype, int D) { return dtype != RTK_F32 && D == HD; }
// logits in base 2: s * log2(e) / sqrt(D)
inline float logit_scale2(int D) { return (float)(1.4426950408889634074 / sqrt((double)D)); }

}  // namespace rtk

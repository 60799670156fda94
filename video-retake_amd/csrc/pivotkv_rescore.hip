// pivotkv_rescore.hip — the video budget's re-scoring on gfx950 (retake_hip.h "Budget re-scoring";
// longvideo_kwargs["video_budget_rescore"]; NOT in the reference, which processes a finished video: a rule of this project's
// own).  The n old rows of a layer's video region are scored by the last W rotated query rows of the chunk that has just gone
// through the layer, and the stored fp32 score of each is blended with what they saw:
//   p_h[i, .] = softmax_{j < n}(q[h,i] . k[h / G, j] / sqrt(D))           no mask; keys >= n are never read
//   obs[j]    = (n / (Hq W)) * sum_h sum_{i < W} p_h[i, j]                averages 1 over the n rows
//   score[j]  = fmaf(alpha, obs[j], (1 - alpha) * score[j])               (1 - alpha) rounded once, then one product, one fma
// The contraction is the thin one of score_thin.cuh (its loads, block step and merges are written there) - few query rows
// against many keys, the G W rows of a kv group packed as r = hh W + i into 32-row blocks - but against ~10^5 keys with a head
// stride, so the keys are SPLIT: key range kr of a unit is keys [kr * RS_KEYS, (kr + 1) * RS_KEYS), a function of n alone
// (never of the unit count, the unit's index, the strides or the machine), and every sum below runs in an order fixed by
// (n, W, Hq, Hkv, D, dtype).  No atomics.  Three launches:
//   rescore_lse_kernel    grid (ranges, Hkv, units): a workgroup keeps its range's keys of one group in registers (a wave
//                         holds RS_NKB blocks of 32), puts the group's query blocks into LDS in fragment order (up to RS_QB
//                         blocks = 112 KiB a tile; every wave reads them from there, so a query block leaves L2 once per
//                         RS_KEYS keys and a key row leaves HBM once), and writes per packed row the range's (max, sum),
//                         base 2: the lane's 16 logits per block, blocks in order, the wave's halves, the waves in order
//   rescore_merge_kernel  one thread per packed row: the ranges' (max, sum) merged in range order -> lse2[g][r]
//                         (+inf for the rows that pad the last block: their probabilities are 0)
//   rescore_col_kernel    grid (ranges, units): a workgroup owns ALL kv groups of its range's keys: per group the keys in
//                         registers, the query blocks through LDS as above, col += exp2(s c - lse2[r]) in block order;
//                         groups in order, the blend written straight into score[j]
// Arithmetic: exact products of the 16-bit operands, fp32 accumulation, softmax and sums.  fp32 payloads or head_dim != 128:
// the *_generic kernels (plain FMA, natural exp, dot / sqrt(D)) over the same key ranges and the same merge: the parity path.
// rtk_pivotkv_rescore_fp8k_batched (longvideo_kwargs["archive_rescore"]): the same three launches over the e4m3 archive's
// key rows - the two MFMA kernels take their key source as a template argument (Keys16 / KeysFp8), and the only device code
// that differs is the fragment load, which dequantises the codes (rule 5 of the fp8 rows) into the registers the 16-bit load
// fills from the dequantised row.  Hence: the bits of the 16-bit call on the dequantised rows.
#include <atomic>
#include <cstring>
#include <type_traits>

#include "score_thin.cuh"

namespace rtk {
namespace {

constexpr int RS_MAX_UNITS = 32;                  // units per launch (the array travels as a kernel argument)
constexpr int RS_KEYS = RTK_RESCORE_KEYS;         // keys per range = per workgroup
constexpr int RS_WAVES = 8;                       // waves per workgroup: two per SIMD (a wave's softmax under another's MFMAs; -12 % at W 64)
constexpr int RS_THREADS = RS_WAVES * WAVE;
constexpr int RS_NKB = RS_KEYS / (RS_WAVES * 32); // 32-key blocks a wave keeps in registers
constexpr int RS_QB = 14;                         // 32-row query blocks per LDS tile (G 7 x W 64)
constexpr int RS_BLOCK_BYTES = 32 * HD * 2;       // one query block in fragment order
constexpr int RS_MAX_N = 1 << 24;
static_assert(RS_KEYS == RS_WAVES * RS_NKB * 32, "a range is what one workgroup keeps in registers");

struct RescoreDev {
    const char* q;
    const char* k;     // row 0 of kv head 0
    int64_t ksh;       // BYTES between kv heads
    float* score;
    float* lse;        // [Hkv][rows_pad]
    float2* part;      // [Hkv][ranges(n)][rows_pad]
    int32_t n, pad;
};
struct RescoreUnits {
    RescoreDev u[RS_MAX_UNITS];
};
// the same unit over e4m3 archive rows (rtk_pivotkv_rescore_fp8k_batched): a struct of its own, so that the 16-bit kernels'
// argument - and with it their code - stays what it was
struct RescoreFp8kDev {
    const char* q;
    const char* k8;    // codes of row 0 of kv head 0
    int64_t ksh;       // BYTES between kv heads
    const float* ks;   // scale of row 0 of kv head 0
    int64_t ssh;       // FLOATS between kv heads
    float* score;
    float* lse;
    float2* part;
    int32_t n, pad;
};
struct RescoreFp8kUnits {
    RescoreFp8kDev u[RS_MAX_UNITS];
};

// Where the MFMA kernels' keys come from: the launch's argument and this lane's fragment of key j0 + (lane & 31) of kv group g
struct Keys16 {
    using Units = RescoreUnits;
    template <bool F16>
    static __device__ __forceinline__ void load(u32x4* f, const RescoreDev& un, int g, int j0, int n, int lane) {
        load_key_frag(f, un.k + (int64_t)g * un.ksh, j0, n, lane);
    }
};
struct KeysFp8 {   // dequantised to the queries' dtype (rule 5 of the fp8 rows): the registers Keys16 loads from the dequantised rows
    using Units = RescoreFp8kUnits;
    template <bool F16>
    static __device__ __forceinline__ void load(u32x4* f, const RescoreFp8kDev& un, int g, int j0, int n, int lane) {
        load_key_frag_fp8<F16 ? RTK_F16 : RTK_BF16>(f, un.k8 + (int64_t)g * un.ksh, un.ks + (int64_t)g * un.ssh, j0, n, lane);
    }
};

__device__ __forceinline__ int ranges_of(int n) { return (n + RS_KEYS - 1) / RS_KEYS; }

// query blocks [rb0, rb0 + nb) of kv group g into LDS, fragment order: chunk x of lane l of block b at lq[(b * 8 + x) * 64 + l]
// (what the lane reads back is 16 contiguous bytes next to its neighbours': no bank conflicts).  The rows that pad the last
// block are zeros
__device__ __forceinline__ void fill_query_tile(u32x4* lq, const char* qu, int g, int G, int W, int rb0, int nb, int64_t qsh,
                                                int64_t qpitch, int wid, int lane) {
    for (int b = wid; b < nb; b += RS_WAVES) {
        const u32x4* p;
        const bool ok = packed_row(p, qu, g, G, W, (rb0 + b) * 32 + (lane & 31), qsh, qpitch);
        load_frag<64>(lq + b * 8 * 64 + lane, p, ok, lane >> 5);
    }
}
__device__ __forceinline__ void read_query_block(u32x4* f, const u32x4* lq, int b, int lane) {
#pragma unroll
    for (int x = 0; x < 8; ++x) f[x] = lq[(b * 8 + x) * 64 + lane];
}

// the online (max, sum), base 2, of ONE packed row (this lane's) over the wave's RS_NKB key blocks, blocks in order.  MASKED:
// the wave's keys reach past n - only the first `left` of them count (the last range of a unit; the limit is made opaque
// per call so that the 64 comparisons are redone there instead of living in scalar registers across the row blocks)
template <bool F16, bool MASKED>
__device__ __forceinline__ void lse_block(const u32x4 (&kf)[RS_NKB][8], const u32x4* qf, float c2, int left, float& m, float& sum) {
    const int hf = (threadIdx.x & (WAVE - 1)) >> 5;
    if constexpr (MASKED) asm volatile("" : "+v"(left));
#pragma unroll
    for (int kb = 0; kb < RS_NKB; ++kb) lse_step<F16, MASKED>(kf[kb], qf, c2, kb * 32, left, hf, m, sum);
}

template <bool F16, class KS = Keys16>
__global__ __launch_bounds__(RS_THREADS) void rescore_lse_kernel(typename KS::Units us, int G, int W, int64_t qsh, int64_t qpitch,
                                                               int RB, float c2) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, hf = lane >> 5, row = lane & 31;
    const auto& un = us.u[blockIdx.z];
    const int kr = blockIdx.x, g = blockIdx.y, n = un.n;
    if (kr * RS_KEYS >= n) return;   // (uniform: the grid is sized for the launch's largest unit)
    const int QBn = min(RB, RS_QB);
    u32x4* lq = (u32x4*)rs_smem;
    float2* red = (float2*)(rs_smem + (size_t)QBn * RS_BLOCK_BYTES);   // [RS_WAVES][QBn][32]
    const int j0 = kr * RS_KEYS + wid * (RS_NKB * 32);
    const bool full = j0 + RS_NKB * 32 <= n;   // (wave-uniform)
    u32x4 kf[RS_NKB][8];
#pragma unroll
    for (int kb = 0; kb < RS_NKB; ++kb) KS::template load<F16>(kf[kb], un, g, j0 + kb * 32, n, lane);
    float2* part = un.part + ((size_t)g * ranges_of(n) + kr) * ((size_t)RB * 32);
    for (int rb0 = 0; rb0 < RB; rb0 += RS_QB) {
        const int nb = min(RS_QB, RB - rb0);
        __syncthreads();   // the tile before this one has been read, its partials merged
        fill_query_tile(lq, un.q, g, G, W, rb0, nb, qsh, qpitch, wid, lane);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            u32x4 qf[8];
            read_query_block(qf, lq, b, lane);
            float m = -INFINITY, sum = 0.f;
            if (full) lse_block<F16, false>(kf, qf, c2, 0, m, sum);
            else lse_block<F16, true>(kf, qf, c2, n - j0, m, sum);
            const float2 half = merge_halves(m, sum, hf);
            if (hf == 0) red[(wid * QBn + b) * 32 + row] = half;
        }
        __syncthreads();
        for (int e = tid; e < nb * 32; e += RS_THREADS)   // the waves, in wave order (wave 0 always holds a key < n)
            part[rb0 * 32 + e] = merge_in_order<true>(RS_WAVES, [&](int w) { return red[w * QBn * 32 + e]; });
    }
}

// lse[g][r] of every packed row: the key ranges' (max, sum) in range order.  BASE2: the MFMA path's log2 domain
template <bool BASE2, class Units = RescoreUnits>
__global__ __launch_bounds__(256) void rescore_merge_kernel(Units us, int Hkv, int rows_pad, int nrows) {
    const auto& un = us.u[blockIdx.y];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Hkv * rows_pad) return;
    const int g = e / rows_pad, r = e - g * rows_pad, KR = ranges_of(un.n);
    const float2* p = un.part + (size_t)g * KR * rows_pad + r;
    const float2 ms = merge_in_order<BASE2>(KR, [&](int kr) { return p[(size_t)kr * rows_pad]; });
    un.lse[e] = r < nrows ? lse_of<BASE2>(ms) : INFINITY;
}

// score[j] <- fmaf(alpha, obs[j], (1 - alpha) score[j]), obs[j] = tot[j] * (n / (Hq W))
__device__ __forceinline__ float blend(float old, float tot, float fac, float alpha) {
    return fmaf(alpha, __fmul_rn(tot, fac), __fmul_rn(__fsub_rn(1.f, alpha), old));
}

template <bool F16, class KS = Keys16>
__global__ __launch_bounds__(RS_THREADS) void rescore_col_kernel(typename KS::Units us, int Hkv, int G, int W, int64_t qsh,
                                                               int64_t qpitch, int RB, float c2, float alpha) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, hf = lane >> 5;
    const auto& un = us.u[blockIdx.y];
    const int kr = blockIdx.x, n = un.n;
    if (kr * RS_KEYS >= n) return;   // (uniform)
    u32x4* lq = (u32x4*)rs_smem;
    const int j0 = kr * RS_KEYS + wid * (RS_NKB * 32);
    const bool live = j0 < n;   // (wave-uniform; a wave past n still fills its share of the tiles and meets the barriers)
    float tot[RS_NKB];
#pragma unroll
    for (int kb = 0; kb < RS_NKB; ++kb) tot[kb] = 0.f;
    for (int g = 0; g < Hkv; ++g) {
        u32x4 kf[RS_NKB][8];
#pragma unroll
        for (int kb = 0; kb < RS_NKB; ++kb) KS::template load<F16>(kf[kb], un, g, j0 + kb * 32, n, lane);
        const float* lg = un.lse + (size_t)g * RB * 32;
        float col[RS_NKB];
#pragma unroll
        for (int kb = 0; kb < RS_NKB; ++kb) col[kb] = 0.f;
        for (int rb0 = 0; rb0 < RB; rb0 += RS_QB) {
            const int nb = min(RS_QB, RB - rb0);
            __syncthreads();
            fill_query_tile(lq, un.q, g, G, W, rb0, nb, qsh, qpitch, wid, lane);
            __syncthreads();
            if (live) {
                for (int b = 0; b < nb; ++b) {
                    u32x4 qf[8];
                    read_query_block(qf, lq, b, lane);
                    float ls[16];
                    load_ls(ls, lg, rb0 + b, hf);
#pragma unroll
                    for (int kb = 0; kb < RS_NKB; ++kb) {
                        f32x16 acc = f32x16{0};
#pragma unroll
                        for (int x = 0; x < 8; ++x) mma16<F16>(acc, qf[x], kf[kb][x], acc);   // acc[r] = q[.. + acc_row(r, hf)] . k[j]
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            col[kb] += __builtin_amdgcn_exp2f(__fsub_rn(__fmul_rn(acc[r], c2), ls[r]));
                    }
                }
            }
        }
#pragma unroll
        for (int kb = 0; kb < RS_NKB; ++kb) {
            col[kb] += __shfl_xor(col[kb], 32, WAVE);
            tot[kb] += col[kb];
        }
    }
    const float fac = __fdiv_rn((float)n, (float)(Hkv * G * W));
    if (hf == 0) {
#pragma unroll
        for (int kb = 0; kb < RS_NKB; ++kb) {
            const int j = j0 + kb * 32 + (lane & 31);
            if (j < n) un.score[j] = blend(un.score[j], tot[kb], fac, alpha);
        }
    }
}

// ---- any head_dim, any payload: plain FMA, dot / sqrt(D), natural exp (score_thin.cuh); the same key ranges, the same merge
// (max, sum) of query row i of head h over key range kr: grid (ranges, Hq * W, units)
template <int DT>
__global__ __launch_bounds__(256) void rescore_lse_generic(RescoreUnits us, int G, int W, int D, int64_t qsh, int64_t qpitch) {
    extern __shared__ float rs_qs[];  // [D]
    const RescoreDev& un = us.u[blockIdx.z];
    const int kr = blockIdx.x, n = un.n;
    if (kr * RS_KEYS >= n) return;   // (uniform)
    const int h = blockIdx.y / W, i = blockIdx.y - h * W, g = h / G;
    const float2 ms = range_softmax<DT>(rs_qs, un.q + (int64_t)h * qsh + (int64_t)i * qpitch, un.k + (int64_t)g * un.ksh, 0,
                                        kr * RS_KEYS, min(n, (kr + 1) * RS_KEYS), D);
    if (threadIdx.x == 0) un.part[((size_t)g * ranges_of(n) + kr) * (G * W) + (h - g * G) * W + i] = ms;
}

// the blend of key j: one thread per key, every query row of every head in turn: grid (ceil(n_max / 256), units)
template <int DT>
__global__ __launch_bounds__(256) void rescore_col_generic(RescoreUnits us, int Hkv, int G, int W, int D, int64_t qsh,
                                                           int64_t qpitch, float alpha) {
    extern __shared__ float rs_qs[];  // [D]
    const RescoreDev& un = us.u[blockIdx.y];
    const int n = un.n;
    if (blockIdx.x * 256 >= n) return;   // (uniform)
    const int j = blockIdx.x * 256 + threadIdx.x;
    float tot = 0.f;
    const char* k = un.k;   // (read once, in front of the loop: the key's address is then stepped by ksh; read per group it
    const int64_t ksh = un.ksh;   //  is rebuilt from j D each time, which costs two vector registers)
    for (int g = 0; g < Hkv; ++g)
        tot += column_sum<DT>(
            rs_qs, k + (int64_t)g * ksh, (size_t)j * D, j < n, G, W, D,
            [&](int hh, int i) { return un.q + (int64_t)(g * G + hh) * qsh + (int64_t)i * qpitch; },
            [&](int hh, int i) { return un.lse[(size_t)(g * G + hh) * W + i]; });
    if (j < n) un.score[j] = blend(un.score[j], tot, __fdiv_rn((float)n, (float)(Hkv * G * W)), alpha);
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// a unit's scratch: lse [Hkv][rows_pad] fp32, then the ranges' partials [Hkv][ranges(n)][rows_pad] float2
struct RescorePlan {
    bool mfma;
    int Hkv, G, nrows, RB, rows_pad;
    size_t lse_bytes;
    size_t bytes(int n) const { return lse_bytes + al256((size_t)Hkv * ((n + RS_KEYS - 1) / RS_KEYS) * rows_pad * sizeof(float2)); }
};
inline bool rescore_plan(RescorePlan& p, int Hq, int Hkv, int W, int D, int dtype) {
    if (Hq < 1 || Hkv < 1 || Hq % Hkv || W < 1 || D < 1 || !payload_dtype(dtype)) return false;
    p.mfma = thin_mfma_path(dtype, D);
    p.Hkv = Hkv;
    p.G = Hq / Hkv;
    // (the generic path's grid carries Hq W in its y axis)
    if ((int64_t)p.G * W > (1 << 20) || (!p.mfma && (int64_t)Hq * W > 65535)) return false;
    p.nrows = p.G * W;
    p.RB = packed_row_blocks(p.G, W);
    p.rows_pad = p.mfma ? p.RB * 32 : p.nrows;
    p.lse_bytes = al256((size_t)Hkv * p.rows_pad * 4);
    return true;
}

// What both entries do around their units' keys: the checks in front of every launch (check_keys(u, i, plan, es): the unit's
// own pointers and strides), the scratch, the LDS opt-in and the launches.  KS: where the MFMA kernels' keys come from;
// fill_keys(u, slot) writes a unit's key pointers into its slot.  The generic pair reads 16-bit or fp32 rows only
template <class KS, class Unit, class CheckKeys, class FillKeys>
int rescore_run(const char* who, const Unit* units, int n_units, int Hq, int Hkv, int W, int D, int dtype, float alpha,
                int64_t q_stride_h, int64_t q_stride_l, void* scratch, size_t scratch_stride, hipStream_t st, CheckKeys&& check_keys,
                FillKeys&& fill_keys) {
    using Units = typename KS::Units;
    constexpr bool GENERIC = std::is_same<KS, Keys16>::value;   // (the parity path exists for 16-bit / fp32 rows)
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Hq % Hkv == 0 && D >= 1, "%s: bad shape (Hq %d, Hkv %d, D %d)", who, Hq, Hkv, D);
    RTK_CHECK_ARG(W >= 1, "%s: W %d", who, W);
    RTK_CHECK_ARG(alpha > 0.f && alpha <= 1.f, "%s: alpha %g is not in (0, 1]", who, (double)alpha);   // (a NaN fails too)
    if (!payload_dtype(dtype)) {
        set_error("%s: payloads are RTK_F32 / RTK_BF16 / RTK_F16, got %d", who, dtype);
        return RTK_EUNSUPPORTED;
    }
    if (!GENERIC && !thin_mfma_path(dtype, D)) {
        set_error("%s: e4m3 keys are dequantised to RTK_BF16 / RTK_F16 rows of head_dim %d, got dtype %d, D %d", who, HD, dtype, D);
        return RTK_EUNSUPPORTED;
    }
    RescorePlan p;
    RTK_CHECK_ARG(rescore_plan(p, Hq, Hkv, W, D, dtype), "%s: %d query rows per kv group are beyond the plan", who, (Hq / Hkv) * W);
    const int64_t es = dtype == RTK_F32 ? 4 : 2;
    RTK_CHECK_ARG(q_stride_h >= D && q_stride_l >= D, "%s: query strides (%lld, %lld) below D", who, (long long)q_stride_h,
                  (long long)q_stride_l);
    RTK_CHECK_ARG(!p.mfma || ((q_stride_h * es) % 16 == 0 && (q_stride_l * es) % 16 == 0),
                  "%s: query rows must be 16-byte aligned", who);
    RTK_CHECK_ARG(scratch && ((uintptr_t)scratch & 255) == 0 && scratch_stride % 256 == 0,
                  "%s: scratch must be 256-byte aligned, units a multiple of 256 bytes apart", who);
    int n_max = 0;
    for (int i = 0; i < n_units; ++i) {
        const Unit& u = units[i];
        RTK_CHECK_ARG(u.n >= 0 && u.n <= RS_MAX_N, "%s: unit %d: n %d (0 .. %d)", who, i, u.n, RS_MAX_N);
        if (u.n == 0) continue;
        const int rc = check_keys(u, i, p, es);
        if (rc != RTK_OK) return rc;
        RTK_CHECK_ARG(scratch_stride >= p.bytes(u.n), "%s: unit %d: scratch stride %zu < %zu bytes for n %d", who, i,
                      scratch_stride, p.bytes(u.n), u.n);
        n_max = std::max(n_max, u.n);
    }
    if (n_max == 0) return RTK_OK;
    const int QBn = std::min(p.RB, RS_QB);
    const size_t lds1 = (size_t)QBn * RS_BLOCK_BYTES + (size_t)RS_WAVES * QBn * 32 * sizeof(float2), lds2 = (size_t)QBn * RS_BLOCK_BYTES;
    if (p.mfma && lds1 > 48 * 1024) {   // opt in to the large dynamic LDS window, once per device (and per key source)
        static std::atomic<uint64_t> opted{0};
        int dev_id = 0;
        (void)hipGetDevice(&dev_id);
        const uint64_t bit = 1ull << (dev_id & 63);
        if (!(opted.load(std::memory_order_relaxed) & bit)) {
            constexpr int MOST = RS_QB * RS_BLOCK_BYTES + RS_WAVES * RS_QB * 32 * (int)sizeof(float2);
            (void)hipFuncSetAttribute((const void*)rescore_lse_kernel<false, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, MOST);
            (void)hipFuncSetAttribute((const void*)rescore_lse_kernel<true, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, MOST);
            (void)hipFuncSetAttribute((const void*)rescore_col_kernel<false, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, MOST);
            (void)hipFuncSetAttribute((const void*)rescore_col_kernel<true, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, MOST);
            opted.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    const int64_t qsh = q_stride_h * es, qpitch = q_stride_l * es;
    const float c2 = logit_scale2(D);
    int most = 0;   // of the launch being filled: its largest unit's rows
    return launch_units<Units>(
        n_units,
        [&](int i, auto& dv) {
            const Unit& u = units[i];
            if (u.n == 0) return false;
            char* ws = (char*)scratch + (size_t)i * scratch_stride;
            dv.q = (const char*)u.q;
            fill_keys(u, dv, es);
            dv.score = u.score;
            dv.lse = (float*)ws;
            dv.part = (float2*)(ws + p.lse_bytes);
            dv.n = u.n;
            dv.pad = 0;
            most = std::max(most, u.n);
            return true;
        },
        [&](const Units& ru, int n) -> int {
            const int KR = (most + RS_KEYS - 1) / RS_KEYS;
            const dim3 gm((Hkv * p.rows_pad + 255) / 256, n);
            if (p.mfma) {
                with_f16(dtype, [&](auto f16) {
                    constexpr bool F16 = decltype(f16)::value;
                    RTK_LAUNCH(KID_PASS1, (rescore_lse_kernel<F16, KS>), dim3(KR, Hkv, n), dim3(RS_THREADS), lds1, st, ru, p.G, W,
                               qsh, qpitch, p.RB, c2);
                    RTK_LAUNCH(KID_PASS1, (rescore_merge_kernel<true, Units>), gm, dim3(256), 0, st, ru, Hkv, p.rows_pad, p.nrows);
                    RTK_LAUNCH(KID_PASS2, (rescore_col_kernel<F16, KS>), dim3(KR, n), dim3(RS_THREADS), lds2, st, ru, Hkv, p.G, W,
                               qsh, qpitch, p.RB, c2, alpha);
                });
            } else if constexpr (GENERIC) {
                with_payload(dtype, [&](auto dt) {
                    constexpr int DT = decltype(dt)::value;
                    RTK_LAUNCH(KID_PASS1, rescore_lse_generic<DT>, dim3(KR, Hq * W, n), dim3(256), D * sizeof(float), st, ru, p.G,
                               W, D, qsh, qpitch);
                    RTK_LAUNCH(KID_PASS1, rescore_merge_kernel<false>, gm, dim3(256), 0, st, ru, Hkv, p.rows_pad, p.nrows);
                    RTK_LAUNCH(KID_PASS2, rescore_col_generic<DT>, dim3((most + 255) / 256, n), dim3(256), D * sizeof(float), st,
                               ru, Hkv, p.G, W, D, qsh, qpitch, alpha);
                    return 0;
                });
            }
            RTK_LAUNCH_CHECK(who);
            most = 0;
            return RTK_OK;
        });
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" size_t rtk_pivotkv_rescore_workspace_bytes(int Hq, int Hkv, int W, int n_max, int D, int dtype) {
    RescorePlan p;
    if (n_max < 0 || n_max > RS_MAX_N || !rescore_plan(p, Hq, Hkv, W, D, dtype)) return 0;
    return p.bytes(n_max);
}

extern "C" int rtk_pivotkv_rescore_batched(const rtk_rescore_unit* units, int n_units, int Hq, int Hkv, int W, int D, int dtype,
                                           float alpha, int64_t q_stride_h, int64_t q_stride_l, void* scratch,
                                           size_t scratch_stride, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_rescore_batched";
    const int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    return rescore_run<Keys16>(
        who, units, n_units, Hq, Hkv, W, D, dtype, alpha, q_stride_h, q_stride_l, scratch, scratch_stride, (hipStream_t)stream,
        [&](const rtk_rescore_unit& u, int i, const RescorePlan& p, int64_t es) -> int {
            RTK_CHECK_ARG(u.q && u.k && u.score, "%s: unit %d: NULL q / k / score", who, i);
            RTK_CHECK_ARG(((uintptr_t)u.score & 3) == 0, "%s: unit %d: score is not 4-byte aligned", who, i);
            RTK_CHECK_ARG(u.k_stride_h >= (int64_t)u.n * D, "%s: unit %d: k_stride_h %lld < n D", who, i, (long long)u.k_stride_h);
            RTK_CHECK_ARG(!p.mfma || (((uintptr_t)u.q & 15) == 0 && ((uintptr_t)u.k & 15) == 0 && (u.k_stride_h * es) % 16 == 0),
                          "%s: unit %d: q / k / k_stride_h must be 16-byte aligned", who, i);
            return RTK_OK;
        },
        [](const rtk_rescore_unit& u, RescoreDev& dv, int64_t es) {
            dv.k = (const char*)u.k;
            dv.ksh = u.k_stride_h * es;
        });
}

extern "C" int rtk_pivotkv_rescore_fp8k_batched(const rtk_rescore_fp8k_unit* units, int n_units, int Hq, int Hkv, int W, int D,
                                                int dtype, float alpha, int64_t q_stride_h, int64_t q_stride_l, void* scratch,
                                                size_t scratch_stride, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_rescore_fp8k_batched";
    const int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    return rescore_run<KeysFp8>(
        who, units, n_units, Hq, Hkv, W, D, dtype, alpha, q_stride_h, q_stride_l, scratch, scratch_stride, (hipStream_t)stream,
        [&](const rtk_rescore_fp8k_unit& u, int i, const RescorePlan&, int64_t) -> int {
            RTK_CHECK_ARG(u.q && u.k8 && u.k_scale && u.score, "%s: unit %d: NULL q / k8 / k_scale / score", who, i);
            RTK_CHECK_ARG(((uintptr_t)u.score & 3) == 0, "%s: unit %d: score is not 4-byte aligned", who, i);
            RTK_CHECK_ARG(u.k8_stride_h >= (int64_t)u.n * D, "%s: unit %d: k8_stride_h %lld < n D", who, i, (long long)u.k8_stride_h);
            RTK_CHECK_ARG(u.scale_stride_h >= (int64_t)u.n, "%s: unit %d: scale_stride_h %lld < n", who, i,
                          (long long)u.scale_stride_h);
            RTK_CHECK_ARG(((uintptr_t)u.q & 15) == 0 && ((uintptr_t)u.k8 & 15) == 0 && u.k8_stride_h % 16 == 0,
                          "%s: unit %d: q / k8 / k8_stride_h must be 16-byte aligned", who, i);
            RTK_CHECK_ARG(((uintptr_t)u.k_scale & 3) == 0, "%s: unit %d: k_scale is not 4-byte aligned", who, i);
            return RTK_OK;
        },
        [](const rtk_rescore_fp8k_unit& u, RescoreFp8kDev& dv, int64_t) {
            dv.k8 = (const char*)u.k8;
            dv.ksh = u.k8_stride_h;
            dv.ks = u.k_scale;
            dv.ssh = u.scale_stride_h;
        });
}

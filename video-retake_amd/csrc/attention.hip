// attention.hip — chunk attention over [compressed prefix | current chunk] (retake_hip.h "Chunk attention").
//
//   out[i, h, :] = softmax_j(q[h, i, :] . k[h / G, j, :] * scale) . v[h / G, j, :]      j <= q_offset + i, j < Lk
//
// (q_offset = Lk - Lq: bottom-right causal.)  Batch 1, GQA by index (no repeat_kv), causal by index compare (no mask
// operand), q / k / v read where the caller has them (pointer + head / row strides), softmax statistics and accumulation
// in fp32.
//
// Fast path (bf16 / fp16, head_dim 128) — attn_fwd_d128_kernel, flash-style, one pass over the keys:
//   * a workgroup = 4 waves = 128 query rows of one head, a wave = 32 rows; Q lives in registers as the B operand;
//   * 64-key K and V tiles travel global -> registers -> LDS (two LDS buffers; the next tile's loads are issued before
//     the current tile's MFMAs, its LDS writes after them: one barrier per tile);
//   * S^T = mfma(K, Q): a lane owns ONE query row (column lane & 31) and 32 of the tile's 64 logits, so max / sum are
//     lane-local plus one exchange with lane ^ 32;
//   * O^T = mfma(V^T, P^T): the logits' accumulator registers, converted pairwise to 16 bits, ARE the B operand (the
//     k order inside a step is permuted - key 16s + 8(j>>2) + 4h + (j&3) in element j of lane half h - and the V^T
//     fragments are fetched in that same order with ds_read_b64_tr_b16), so the running rescale of O is lane-local too;
//   * one LDS image serves K's row reads (ds_read_b128) and V's transposed reads: 256-byte rows, 16-byte chunk
//     ch of row r at chunk ch ^ (((r & 3) << 2) | ((r >> 2) & 3));
//   * key tiles above a wave's diagonal are skipped, tiles that straddle it mask by index, the rest take the plain body;
//     rows >= Lq and keys >= Lk are zero-filled by the buffer descriptors' bounds (never read, never padded);
//   * O leaves through LDS as whole 256-byte rows of out[Lq, Hq, D].
// General path (fp32, or any head_dim that is a multiple of 8 up to 256) — attn_fwd_general_kernel: one wave per
// (head, query row), fp32 FMA, 64 keys per step.  No performance claim; it is what the parity fixtures run through.
// Few query rows — both kernels take a key range per blockIdx "split" and leave un-normalised (m, l, acc) partials in
// the caller's workspace; attn_combine_kernel folds them split 0, 1, 2 ... in that fixed order (no atomics).  The
// number of splits is a function of the shape alone.
#include <cmath>

#include "common.cuh"

namespace rtk {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using i16x4 = __attribute__((ext_vector_type(4))) short;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT_QB = 128;            // query rows per workgroup (fast path)
constexpr int AT_KT = 64;             // keys per tile
constexpr int AT_TILE = AT_KT * 256;  // bytes of one K or V tile in LDS (head_dim 128, 16-bit)
constexpr int AT_OPITCH = 272;        // bytes per staged output row (16-byte aligned, off the 256-byte bank period)
constexpr int AT_TARGET_WG = 512;     // workgroups wanted before the keys are split (2 per CU; a constant, not a device query)
constexpr int AT_TARGET_WAVES = 2048; // general path: waves wanted
constexpr int AT_MIN_SPLIT_KEYS = 512;

template <int DT> __device__ __forceinline__ void mma16(f32x16& acc, const u32x4& a, const u32x4& b) {
    if constexpr (DT == RTK_F16)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// descriptor over `bytes` bytes from a wave-uniform base: loads beyond it return zero
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bounded_rsrc(const void* p, uint32_t bytes) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned long long u = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    return __builtin_amdgcn_make_buffer_rsrc((void*)u, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return u32x4{v[0], v[1], v[2], v[3]};
}
// row r of the accumulator register `reg` in lane half `hf` of a 32x32 MFMA result
__device__ __forceinline__ int acc_row(int reg, int hf) { return (reg & 3) + 8 * (reg >> 2) + 4 * hf; }
__device__ __forceinline__ int swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ float safe_max(float m) { return m == -INFINITY ? 0.f : m; }

template <int DT, bool SPLIT>
__global__ __launch_bounds__(256, 2) void attn_fwd_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, uint32_t q_row_bytes, uint32_t q_bytes, const char* __restrict__ k,
    const char* __restrict__ v, int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, char* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq, int G, int Lq, int Lk, int off, float c2,
    int keys_per_split) {
    using Hh = H16<DT>;
    __shared__ __attribute__((aligned(16))) char lds[4 * AT_TILE];   // [buffer][K | V]
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int r = lane & 31, hf = lane >> 5;
    const int nqb = (Lq + AT_QB - 1) / AT_QB;
    const int qb = nqb - 1 - (int)blockIdx.x / Hq;   // heaviest (last) query block first
    const int hq = (int)blockIdx.x % Hq, hkv = hq / G;
    const int row_base = qb * AT_QB, wrow0 = row_base + 32 * wave, qrow = wrow0 + r;
    int k_lo = 0, k_hi = min(Lk, off + min(row_base + AT_QB, Lq));   // exclusive: first key no row of the block sees
    if constexpr (SPLIT) {
        k_lo = (int)blockIdx.y * keys_per_split;
        k_hi = min(k_hi, k_lo + keys_per_split);
    }
    const int ntiles = k_hi > k_lo ? (k_hi - k_lo + AT_KT - 1) / AT_KT : 0;
    const bool wave_rows = wrow0 < Lq;
    const int wave_hi = min(Lk, off + min(wrow0 + 32, Lq));   // first key no row of this wave sees

    const __amdgpu_buffer_rsrc_t rq = bounded_rsrc(q + (int64_t)hq * q_sh * 2, q_bytes);
    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(k + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(v + (int64_t)hkv * kv_sh * 2, kv_bytes);

    // Q fragments: k-step s holds q[qrow][16 s + 8 hf .. + 8]
    u32x4 qf[8];
    {
        const uint32_t qo = (uint32_t)qrow * q_row_bytes + 16u * hf;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = load16(rq, qo + 32u * s);
    }
    // staging: thread -> rows (tid >> 4) + 16 u, chunk tid & 15
    const int srow = tid >> 4, sch = tid & 15;
    const uint32_t g_off = (uint32_t)srow * kv_row_bytes + 16u * sch;
    const int l_off = 256 * srow + 16 * (sch ^ swz(srow));   // + 4096 u (rows 16 apart share the swizzle)
    u32x4 kst[4], vst[4];
    auto issue = [&](int kbase) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t o = g_off + (uint32_t)(kbase + 16 * u) * kv_row_bytes;
            kst[u] = load16(rk, o);
            vst[u] = load16(rv, o);
        }
    };
    auto commit = [&](int buf) {
        char* t = lds + buf * 2 * AT_TILE + l_off;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *(u32x4*)(t + 4096 * u) = kst[u];
            *(u32x4*)(t + AT_TILE + 4096 * u) = vst[u];
        }
    };
    // K row reads: key row r (+32), chunk 2 s + hf
    const int k_rd = 256 * r, k_x = swz(r);
    // V transposed reads: lane 4 q_ + p_ of a 16-lane group supplies row q_ of the 4-key block, columns 4 p_ .. 4 p_ + 3
    const int g16 = lane >> 4, q_ = (lane & 15) >> 2, p_ = lane & 3;
    const int v_rd = 256 * (4 * hf + q_) + 8 * (p_ & 1);
    const int v_cl = 2 * (g16 & 1) + (p_ >> 1);   // low bits of the chunk: which 16 of a d-block's 32 columns, which half

    f32x16 oacc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[db][e] = 0.f;
    float m = -INFINITY, l = 0.f;

    if (ntiles > 0) {
        issue(k_lo);
        commit(0);
    }
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int kbase = k_lo + t * AT_KT;
        const bool more = t + 1 < ntiles;
        if (more) issue(kbase + AT_KT);
        if (wave_rows && kbase < wave_hi) {
            const char* kt = lds + (t & 1) * 2 * AT_TILE;
            const char* vt = kt + AT_TILE;
            f32x16 s0, s1;
#pragma unroll
            for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int co = 16 * ((2 * s + hf) ^ k_x);
                const u32x4 a0 = *(const u32x4*)(kt + k_rd + co);
                const u32x4 a1 = *(const u32x4*)(kt + k_rd + 32 * 256 + co);
                mma16<DT>(s0, a0, qf[s]);
                mma16<DT>(s1, a1, qf[s]);
            }
            if (kbase + AT_KT - 1 > min(off + wrow0, Lk - 1)) {   // the tile straddles this wave's diagonal or the end of the keys
                const int lim = min(off + qrow, Lk - 1) - kbase;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = acc_row(e, hf);
                    if (j > lim) s0[e] = -INFINITY;
                    if (j + 32 > lim) s1[e] = -INFINITY;
                }
            }
            float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmaxf(mx, fmaxf(s0[e], s1[e]));
            mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
            const float mnew = fmaxf(m, mx * c2);
            if (!__all(mnew == m)) {   // some row's maximum grew: bring O and l to the new one (exact, no threshold)
                const float alpha = __builtin_amdgcn_exp2f(m - safe_max(mnew));
#pragma unroll
                for (int db = 0; db < 4; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) oacc[db][e] *= alpha;
                l *= alpha;
                m = mnew;
            }
            const float nm = -safe_max(m);
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s0[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], c2, nm));
                s1[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[e], c2, nm));
                ls += s0[e] + s1[e];
            }
            l += ls;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {   // k-step: keys 16 ks .. 16 ks + 15 of the tile
                const f32x16& p = ks < 2 ? s0 : s1;
                const int e0 = 8 * (ks & 1);
                const u32x4 pf = {Hh::pack2(p[e0], p[e0 + 1]), Hh::pack2(p[e0 + 2], p[e0 + 3]),
                                  Hh::pack2(p[e0 + 4], p[e0 + 5]), Hh::pack2(p[e0 + 6], p[e0 + 7])};
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    u32x2 h2[2];
#pragma unroll
                    for (int jh = 0; jh < 2; ++jh) {
                        // rows 16 ks + 8 jh + 4 hf + q_: (row & 3) = q_, ((row >> 2) & 3) = 2 jh + hf
                        const int x = (q_ << 2) | (2 * jh + hf);
                        const int a = v_rd + 256 * (16 * ks + 8 * jh) + 16 * ((4 * db + v_cl) ^ x);
                        const i16x4 t4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) i16x4*)(vt + a));
                        h2[jh] = __builtin_bit_cast(u32x2, t4);
                    }
                    const u32x4 vf = {h2[0][0], h2[0][1], h2[1][0], h2[1][1]};
                    mma16<DT>(oacc[db], vf, pf);
                }
            }
        }
        if (more) commit((t + 1) & 1);
        __syncthreads();
    }

    const float l_tot = l + __shfl_xor(l, 32, WAVE);
    if constexpr (SPLIT) {
        if (qrow < Lq) {
            const size_t row = ((size_t)blockIdx.y * Hq + hq) * Lq + qrow;
            if (hf == 0) *(float2*)(part_ml + 2 * row) = make_float2(m, l_tot);
            float* pa = part_acc + row * 128;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(f32x4*)(pa + 32 * db + 8 * g4 + 4 * hf) =
                        f32x4{oacc[db][4 * g4], oacc[db][4 * g4 + 1], oacc[db][4 * g4 + 2], oacc[db][4 * g4 + 3]};
        }
    } else {
        // every wave has left the tile loop (the barrier above): stage this wave's 32 rows, store them as whole rows
        const float inv = 1.f / l_tot;
        char* st = lds + wave * (32 * AT_OPITCH);
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(u32x2*)(st + r * AT_OPITCH + 2 * (32 * db + 8 * g4 + 4 * hf)) =
                    u32x2{Hh::pack2(oacc[db][4 * g4] * inv, oacc[db][4 * g4 + 1] * inv),
                          Hh::pack2(oacc[db][4 * g4 + 2] * inv, oacc[db][4 * g4 + 3] * inv)};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int rr = 4 * it + (lane >> 4), ch = lane & 15;
            const u32x4 x = *(const u32x4*)(st + rr * AT_OPITCH + 16 * ch);
            if (wrow0 + rr < Lq) *(u32x4*)(out + ((size_t)(wrow0 + rr) * Hq + hq) * 256 + 16 * ch) = x;
        }
    }
}

template <int DT> __device__ __forceinline__ float ld_elem(const void* p, size_t i) {
    if constexpr (DT == RTK_F32) return ((const float*)p)[i];
    else return H16<DT>::ld(p, i);
}
template <int DT> __device__ __forceinline__ void st_elem(void* p, size_t i, float x) {
    if constexpr (DT == RTK_F32) ((float*)p)[i] = x;
    else H16<DT>::st(p, i, x);
}

// One wave per (query row, head, key split).  Per step of 64 keys: lane j computes the logit of key j0 + j (fp32 FMA
// over d, q from LDS), the wave reduces max / sum, then the lanes own channels d = lane + 64 u and walk the step's keys.
template <int DT>
__global__ __launch_bounds__(256) void attn_fwd_general_kernel(const char* __restrict__ q, int64_t q_sh, int64_t q_sl,
                                                               const char* __restrict__ k, const char* __restrict__ v,
                                                               int64_t kv_sh, int64_t kv_sl, char* __restrict__ out,
                                                               float* __restrict__ part_acc, float* __restrict__ part_ml,
                                                               int Hq, int G, int Lq, int Lk, int off, int D, float c2,
                                                               int keys_per_split, int nsplit) {
    using V16 = Vec16<DT>;
    constexpr int VE = V16::VE;
    constexpr size_t ES = DT == RTK_F32 ? 4 : 2;
    __shared__ float qs[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = (int)blockIdx.x * 4 + wave, hq = blockIdx.y, hkv = hq / G, split = blockIdx.z;
    if (row >= Lq) return;   // whole waves; the kernel has no workgroup barrier
    const char* qr = q + ((int64_t)hq * q_sh + (int64_t)row * q_sl) * (int64_t)ES;
    for (int d = lane; d < D; d += WAVE) qs[wave][d] = ld_elem<DT>(qr, d);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const char* kh = k + (int64_t)hkv * kv_sh * (int64_t)ES;
    const char* vh = v + (int64_t)hkv * kv_sh * (int64_t)ES;
    int k_lo = 0, k_hi = min(Lk, off + row + 1);
    if (nsplit > 1) {
        k_lo = split * keys_per_split;
        k_hi = min(k_hi, k_lo + keys_per_split);
    }
    float m = -INFINITY, l = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = k_lo; j0 < k_hi; j0 += WAVE) {
        const int j = j0 + lane;
        float s = -INFINITY;
        if (j < k_hi) {
            const char* kr = kh + (int64_t)j * kv_sl * (int64_t)ES;
            float dot = 0.f;
            for (int d = 0; d < D; d += VE) {
                float f[VE];
                V16::unpack(*(const u32x4*)(kr + (size_t)d * ES), f);
#pragma unroll
                for (int e = 0; e < VE; ++e) dot = __builtin_fmaf(qs[wave][d + e], f[e], dot);
            }
            s = dot * c2;
        }
        const float mnew = fmaxf(m, wave_max(s));   // finite: lane 0's key is in range
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        const float p = __builtin_amdgcn_exp2f(s - mnew);
        l = l * alpha + wave_sum(p);
        m = mnew;
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] *= alpha;
        const int n = min(WAVE, k_hi - j0);
        for (int jj = 0; jj < n; ++jj) {
            const float pj = __shfl(p, jj, WAVE);
            const char* vr = vh + (int64_t)(j0 + jj) * kv_sl * (int64_t)ES;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = lane + WAVE * u;
                if (d < D) acc[u] = __builtin_fmaf(pj, ld_elem<DT>(vr, d), acc[u]);
            }
        }
    }
    if (nsplit > 1) {
        const size_t prow = ((size_t)split * Hq + hq) * Lq + row;
        if (lane == 0) *(float2*)(part_ml + 2 * prow) = make_float2(m, l);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = lane + WAVE * u;
            if (d < D) part_acc[prow * D + d] = acc[u];
        }
    } else {
        const float inv = 1.f / l;
        char* o = out + ((size_t)row * Hq + hq) * D * ES;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = lane + WAVE * u;
            if (d < D) st_elem<DT>(o, d, acc[u] * inv);
        }
    }
}

// out[row, h, d] from the key splits' (m, l, acc) partials, folded in split order 0, 1, 2, ...
template <int DT>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ part_acc, const float* __restrict__ part_ml,
                                                           char* __restrict__ out, int Hq, int Lq, int D, int nsplit) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)Lq * Hq * D;
    if (idx >= total) return;
    const int d = (int)(idx % D);
    const size_t rh = idx / D;   // row * Hq + h
    const int h = (int)(rh % Hq);
    const size_t row = rh / Hq;
    float mg = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mg = fmaxf(mg, part_ml[2 * (((size_t)s * Hq + h) * Lq + row)]);
    float num = 0.f, den = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const size_t prow = ((size_t)s * Hq + h) * Lq + row;
        const float ms = part_ml[2 * prow];
        if (ms == -INFINITY) continue;   // a split wholly above this row's diagonal
        const float w = __builtin_amdgcn_exp2f(ms - mg);
        num = __builtin_fmaf(w, part_acc[prow * D + d], num);
        den = __builtin_fmaf(w, part_ml[2 * prow + 1], den);
    }
    st_elem<DT>(out, idx, num / den);
}

struct AttnPlan {
    bool fast;
    int nsplit, keys_per_split;
    size_t ws_bytes;
};

// A function of the shape alone: the reduction order, hence the bits of the result, never depends on the device.
AttnPlan attn_plan(int Hq, int Lq, int Lk, int D, int dtype) {
    AttnPlan p;
    p.fast = D == 128 && (dtype == RTK_BF16 || dtype == RTK_F16);
    const long long units = p.fast ? (long long)Hq * ((Lq + AT_QB - 1) / AT_QB) : (long long)Hq * Lq;
    const long long target = p.fast ? AT_TARGET_WG : AT_TARGET_WAVES;
    long long ns = 1;
    if (units * 2 <= target) {
        ns = (target + units - 1) / units;
        const long long by_keys = ((long long)Lk + AT_MIN_SPLIT_KEYS - 1) / AT_MIN_SPLIT_KEYS;
        if (ns > by_keys) ns = by_keys;
        if (ns < 1) ns = 1;
    }
    long long kps = ((long long)Lk + ns - 1) / ns;
    kps = (kps + AT_KT - 1) / AT_KT * AT_KT;
    ns = ((long long)Lk + kps - 1) / kps;
    p.nsplit = (int)ns;
    p.keys_per_split = (int)kps;
    p.ws_bytes = ns > 1 ? (size_t)ns * Hq * Lq * ((size_t)D + 2) * sizeof(float) : 0;
    return p;
}

int attn_check_shape(const char* who, int Hq, int Hkv, int Lq, int Lk, int D, int dtype) {
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Lq >= 1 && Lk >= 1, "%s: Hq, Hkv, Lq and Lk must be positive", who);
    RTK_CHECK_ARG(Hq % Hkv == 0, "%s: Hq %d is not a multiple of Hkv %d", who, Hq, Hkv);
    RTK_CHECK_ARG(Lk >= Lq, "%s: Lk %d < Lq %d (the queries are the last Lq rows of the keys)", who, Lk, Lq);
    if (dtype != RTK_F32 && dtype != RTK_BF16 && dtype != RTK_F16) {
        set_error("%s: unsupported dtype code %d (RTK_F32, RTK_BF16 or RTK_F16)", who, dtype);
        return RTK_EUNSUPPORTED;
    }
    if (D < 8 || D > 256 || D % 8 != 0) {
        set_error("%s: unsupported head_dim %d (a multiple of 8 up to 256)", who, D);
        return RTK_EUNSUPPORTED;
    }
    if (Hq > 65535) {
        set_error("%s: unsupported Hq %d (at most 65535)", who, Hq);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

template <int DT>
int attn_launch(const AttnPlan& pl, const void* q, int64_t q_sh, int64_t q_sl, const void* k, const void* v, int64_t kv_sh,
                int64_t kv_sl, void* out, int Hq, int Hkv, int Lq, int Lk, int off, int D, float c2, void* ws, hipStream_t st) {
    const int G = Hq / Hkv;
    float* part_acc = (float*)ws;
    float* part_ml = part_acc ? part_acc + (size_t)pl.nsplit * Hq * Lq * D : nullptr;
    if constexpr (DT != RTK_F32) {
        if (pl.fast) {
            const size_t es = 2;
            const uint32_t q_bytes = (uint32_t)(((size_t)(Lq - 1) * q_sl + D) * es);
            const uint32_t kv_bytes = (uint32_t)(((size_t)(Lk - 1) * kv_sl + D) * es);
            const dim3 grid((unsigned)(Hq * ((Lq + AT_QB - 1) / AT_QB)), (unsigned)pl.nsplit);
            if (pl.nsplit > 1)
                hipLaunchKernelGGL((attn_fwd_d128_kernel<DT, true>), grid, dim3(256), 0, st, (const char*)q, q_sh,
                                   (uint32_t)(q_sl * es), q_bytes, (const char*)k, (const char*)v, kv_sh,
                                   (uint32_t)(kv_sl * es), kv_bytes, (char*)out, part_acc, part_ml, Hq, G, Lq, Lk, off, c2,
                                   pl.keys_per_split);
            else
                hipLaunchKernelGGL((attn_fwd_d128_kernel<DT, false>), grid, dim3(256), 0, st, (const char*)q, q_sh,
                                   (uint32_t)(q_sl * es), q_bytes, (const char*)k, (const char*)v, kv_sh,
                                   (uint32_t)(kv_sl * es), kv_bytes, (char*)out, part_acc, part_ml, Hq, G, Lq, Lk, off, c2,
                                   pl.keys_per_split);
            RTK_LAUNCH_CHECK("attn_fwd_d128_kernel");
        }
    }
    if (!pl.fast) {
        const dim3 grid((unsigned)((Lq + 3) / 4), (unsigned)Hq, (unsigned)pl.nsplit);
        hipLaunchKernelGGL((attn_fwd_general_kernel<DT>), grid, dim3(256), 0, st, (const char*)q, q_sh, q_sl, (const char*)k,
                           (const char*)v, kv_sh, kv_sl, (char*)out, part_acc, part_ml, Hq, G, Lq, Lk, off, D, c2,
                           pl.keys_per_split, pl.nsplit);
        RTK_LAUNCH_CHECK("attn_fwd_general_kernel");
    }
    if (pl.nsplit > 1) {
        const size_t total = (size_t)Lq * Hq * D;
        hipLaunchKernelGGL((attn_combine_kernel<DT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part_acc,
                           part_ml, (char*)out, Hq, Lq, D, pl.nsplit);
        RTK_LAUNCH_CHECK("attn_combine_kernel");
    }
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" size_t rtk_attention_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype) {
    if (attn_check_shape("rtk_attention_workspace_bytes", Hq, Hkv, Lq, Lk, D, dtype) != RTK_OK) return 0;
    return attn_plan(Hq, Lq, Lk, D, dtype).ws_bytes;
}

extern "C" int rtk_attention_forward(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                     int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                     int q_offset, int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                     rtk_stream_t stream) {
    const char* who = "rtk_attention_forward";
    RTK_CHECK_ARG(q && k && v && out, "%s: NULL q / k / v / out pointer", who);
    const int rc = attn_check_shape(who, Hq, Hkv, Lq, Lk, D, dtype);
    if (rc != RTK_OK) return rc;
    RTK_CHECK_ARG(scale > 0.f && std::isfinite(scale), "%s: scale must be positive and finite", who);
    RTK_CHECK_ARG(q_offset >= Lk - Lq && q_offset <= 0x3fffffff,
                  "%s: q_offset %d < Lk - Lq = %d (the last keys would be visible to no row)", who, q_offset, Lk - Lq);
    const size_t es = dtype == RTK_F32 ? 4 : 2;
    // 16-byte row chunks, and per-head extents (the head offset is folded into the descriptor base) that fit the 31-bit
    // buffer offsets with a tile of slack rows
    const bool aligned = (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0 &&
                         (q_stride_h * (int64_t)es) % 16 == 0 && (q_stride_l * (int64_t)es) % 16 == 0 &&
                         (kv_stride_h * (int64_t)es) % 16 == 0 && (kv_stride_l * (int64_t)es) % 16 == 0;
    if (!aligned || q_stride_l < D || kv_stride_l < D || q_stride_h < 0 || kv_stride_h < 0) {
        set_error("%s: unsupported layout (16-byte aligned pointers and strides, row strides >= head_dim)", who);
        return RTK_EUNSUPPORTED;
    }
    if (!fits_buffer_offsets(1, (int64_t)Lq + AT_QB, D, 0, q_stride_l, es) ||
        !fits_buffer_offsets(1, (int64_t)Lk + AT_KT, D, 0, kv_stride_l, es)) {
        set_error("%s: unsupported extent: one head of q or k / v spans 2 GiB or more", who);
        return RTK_EUNSUPPORTED;
    }
    const AttnPlan pl = attn_plan(Hq, Lq, Lk, D, dtype);
    if (pl.ws_bytes) {
        if (!workspace || workspace_bytes < pl.ws_bytes) {
            set_error("%s: workspace too small (%zu < %zu bytes; query rtk_attention_workspace_bytes)", who,
                      workspace ? workspace_bytes : (size_t)0, pl.ws_bytes);
            return RTK_EWORKSPACE;
        }
        RTK_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    }
    const float c2 = scale * 1.44269504088896340736f;   // the kernels exponentiate in base 2
    hipStream_t st = (hipStream_t)stream;
    void* ws = pl.ws_bytes ? workspace : nullptr;
    switch (dtype) {
        case RTK_F32: return attn_launch<RTK_F32>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, c2, ws, st);
        case RTK_BF16: return attn_launch<RTK_BF16>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, c2, ws, st);
        default: return attn_launch<RTK_F16>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, c2, ws, st);
    }
}

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
// rtk_attention_forward_fp8kv / _shared run the fast path's body (attention_d128_body.inc) over [e4m3 archive | 16-bit
// rows] and [archive | another buffer's 16-bit rows | 16-bit rows]: attn_fwd_d128_fp8kv_kernel, attn_fwd_d128_shared_kernel.
// Host side: each entry point keeps its own checks and its fall-through, then attn_forward (operands, plan, workspace,
// dtype) -> attn_launch -> attn_launch_d128, the one launcher of the three d128 kernels; what the packed decode entry
// points (attention_decode.hip) use as well - descriptors, combine launch, checks - is in attention_shared.cuh.
#include "attention_shared.cuh"

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

// row r of the accumulator register `reg` in lane half `hf` of a 32x32 MFMA result
__device__ __forceinline__ int acc_row(int reg, int hf) { return (reg & 3) + 8 * (reg >> 2) + 4 * hf; }
__device__ __forceinline__ int swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// The body of both kernels is attention_d128_body.inc, included once each with FP8 false / true - a function the two
// kernels share compiles the existing instantiations differently (tools/kernel_diff.py), the same text does not.
// SHARED adds a third kind of tile in the same way: [archive | shared 16-bit rows | 16-bit rows], each segment padded.
// FP8: the keys are [archive | 16-bit rows].  Key tiles are counted in a padded index space - the archive takes
// [0, L8p), L8p = L8 rounded up to a whole tile, the 16-bit row r sits at L8p + r - so a tile is of one kind, the split
// plan and the diagonal arithmetic are those of a 16-bit call over L8p + Lk keys, and with L8 % 64 == 0 every fp32 sum
// is grouped exactly as rtk_attention_forward groups it over the concatenation.
template <int DT, bool SPLIT>
__global__ __launch_bounds__(256, 2) void attn_fwd_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, uint32_t q_row_bytes, uint32_t q_bytes, const char* __restrict__ k,
    const char* __restrict__ v, int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, char* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq, int G, int Lq, int Lk, int off, float c2,
    int keys_per_split) {
    constexpr bool FP8 = false, SHARED = false;
    const Archive8 a8{};
    const Shared16 s16{};
#include "attention_d128_body.inc"
}

// the same body over [e4m3 archive | 16-bit rows]: Lk and off describe the 16-bit segment
template <int DT, bool SPLIT>
__global__ __launch_bounds__(256, 2) void attn_fwd_d128_fp8kv_kernel(
    const char* __restrict__ q, int64_t q_sh, uint32_t q_row_bytes, uint32_t q_bytes, const char* __restrict__ k,
    const char* __restrict__ v, int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, char* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq, int G, int Lq, int Lk, int off, float c2,
    int keys_per_split, Archive8 a8) {
    constexpr bool FP8 = true, SHARED = false;
    const Shared16 s16{};
#include "attention_d128_body.inc"
}

// the same body over [e4m3 archive (may be empty) | shared 16-bit rows | own 16-bit rows]: Lk and off describe the own rows
template <int DT, bool SPLIT>
__global__ __launch_bounds__(256, 2) void attn_fwd_d128_shared_kernel(
    const char* __restrict__ q, int64_t q_sh, uint32_t q_row_bytes, uint32_t q_bytes, const char* __restrict__ k,
    const char* __restrict__ v, int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, char* __restrict__ out,
    float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq, int G, int Lq, int Lk, int off, float c2,
    int keys_per_split, Archive8 a8, Shared16 s16) {
    constexpr bool FP8 = true, SHARED = true;
#include "attention_d128_body.inc"
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

// One launch of a d128 kernel variant: kern_split / kern_whole are its SPLIT = true / false instantiations, `tail` the
// a8 / s16 it takes after the common parameters.
template <class K, class... Tail>
int attn_launch_d128(K kern_split, K kern_whole, const char* name, const AttnPlan& pl, const AttnArgs& a, const Partials& p,
                     const Tail&... tail) {
    const dim3 grid((unsigned)(a.Hq * ((a.Lq + AT_QB - 1) / AT_QB)), (unsigned)pl.nsplit);
    hipLaunchKernelGGL(pl.nsplit > 1 ? kern_split : kern_whole, grid, dim3(256), 0, a.st, (const char*)a.q, a.q_sh,
                       (uint32_t)(a.q_sl * 2), rows_extent(a.Lq, a.q_sl, 128, 2), (const char*)a.k, (const char*)a.v, a.kv_sh,
                       (uint32_t)(a.kv_sl * 2), rows_extent(a.Lk, a.kv_sl, 128, 2), (char*)a.out, p.acc, p.ml, a.Hq, a.Hq / a.Hkv,
                       a.Lq, a.Lk, a.off, base2_scale(a.scale), pl.keys_per_split, tail...);
    RTK_LAUNCH_CHECK(name);
    return RTK_OK;
}

// the kernel of the segments the call has ([archive | shared | own], a8 / s16 empty without), then the combine
template <int DT> int attn_launch(const AttnPlan& pl, const AttnArgs& a, const Archive8& a8, const Shared16& s16) {
    const Partials p = split_partials(pl.ws_bytes ? a.workspace : nullptr, pl.nsplit, a.Hq, a.Lq, a.D);
    int rc = RTK_OK;
    if constexpr (DT != RTK_F32) {
        if (pl.fast) {
            if (s16.Ls > 0)
                rc = attn_launch_d128(attn_fwd_d128_shared_kernel<DT, true>, attn_fwd_d128_shared_kernel<DT, false>,
                                      "attn_fwd_d128_shared_kernel", pl, a, p, a8, s16);
            else if (a8.L8 > 0)
                rc = attn_launch_d128(attn_fwd_d128_fp8kv_kernel<DT, true>, attn_fwd_d128_fp8kv_kernel<DT, false>,
                                      "attn_fwd_d128_fp8kv_kernel", pl, a, p, a8);
            else
                rc = attn_launch_d128(attn_fwd_d128_kernel<DT, true>, attn_fwd_d128_kernel<DT, false>, "attn_fwd_d128_kernel", pl, a, p);
        }
    }
    if (!pl.fast) {
        const dim3 grid((unsigned)((a.Lq + 3) / 4), (unsigned)a.Hq, (unsigned)pl.nsplit);
        hipLaunchKernelGGL((attn_fwd_general_kernel<DT>), grid, dim3(256), 0, a.st, (const char*)a.q, a.q_sh, a.q_sl, (const char*)a.k,
                           (const char*)a.v, a.kv_sh, a.kv_sl, (char*)a.out, p.acc, p.ml, a.Hq, a.Hq / a.Hkv, a.Lq, a.Lk, a.off, a.D,
                           base2_scale(a.scale), pl.keys_per_split, pl.nsplit);
        RTK_LAUNCH_CHECK("attn_fwd_general_kernel");
    }
    if (rc != RTK_OK || pl.nsplit == 1) return rc;
    return attn_combine<DT>(p, a.out, a.Hq, a.Lq, a.D, pl.nsplit, a.st);
}

// What the three entry points share once their own checks are through: the operands, the plan over the padded key count,
// the workspace (`query`: the entry point that sizes it) and the dtype switch.
int attn_forward(const char* who, const char* query, const AttnArgs& a, const Archive8& a8, const Shared16& s16) {
    int rc = attn_check_operands(who, a.q, a.q_sh, a.q_sl, a.k, a.v, a.kv_sh, a.kv_sl, a8.k8, a8.v8, a8.ks, a8.vs, a8.sh8, a8.shs,
                                 a.out, a.Lq, a.Lk, a.off, a.D, a.dtype, a.scale, AT_QB, AT_KT);
    if (rc != RTK_OK) return rc;
    const AttnPlan pl = attn_plan(a.Hq, a.Lq, (int)shared_keys(a.Lk, a8.L8, s16.Ls, AT_KT), a.D, a.dtype);
    rc = attn_check_workspace(who, query, pl.ws_bytes, a.workspace, a.workspace_bytes);
    if (rc != RTK_OK) return rc;
    switch (a.dtype) {
        case RTK_F32: return attn_launch<RTK_F32>(pl, a, a8, s16);
        case RTK_BF16: return attn_launch<RTK_BF16>(pl, a, a8, s16);
        default: return attn_launch<RTK_F16>(pl, a, a8, s16);
    }
}

}  // namespace

// (declared in attention_shared.cuh: the packed decode entry points run the same checks)
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

int fp8kv_check_shape(const char* who, int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype) {
    const int rc = attn_check_shape(who, Hq, Hkv, Lq, Lk, D, dtype);
    if (rc != RTK_OK) return rc;
    RTK_CHECK_ARG(L8 >= 0, "%s: L8 %d is negative", who, L8);
    if ((dtype != RTK_BF16 && dtype != RTK_F16) || D != 128) {
        set_error("%s: unsupported dtype code %d / head_dim %d (RTK_BF16 or RTK_F16 with head_dim 128)", who, dtype, D);
        return RTK_EUNSUPPORTED;
    }
    if (shared_keys(Lk, L8, 0, AT_KT) > 0x3fffffff || (long long)L8 * 128 >= (1ll << 31) - AT_KT * 128) {
        set_error("%s: unsupported extent: %d archive rows + %d keys", who, L8, Lk);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

int shared_check_shape(const char* who, int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype, int tile) {
    const int rc = fp8kv_check_shape(who, Hq, Hkv, Lq, Lk, L8, D, dtype);
    if (rc != RTK_OK) return rc;
    RTK_CHECK_ARG(Ls >= 0, "%s: Ls %d is negative", who, Ls);
    if (shared_keys(Lk, L8, Ls, tile) > 0x3fffffff) {
        set_error("%s: unsupported extent: %d archive rows + %d shared rows + %d keys", who, L8, Ls, Lk);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

int shared_check_operands(const char* who, const void* ks, const void* vs, int Ls, int64_t s_stride_h, int64_t s_stride_l, int D,
                          int slack) {
    RTK_CHECK_ARG(ks && vs, "%s: NULL shared pointer with Ls = %d", who, Ls);
    if ((((uintptr_t)ks | (uintptr_t)vs) & 15) != 0 || (s_stride_h * 2) % 16 != 0 || (s_stride_l * 2) % 16 != 0 ||
        s_stride_l < D || s_stride_h < 0) {
        set_error("%s: unsupported layout of the shared rows (16-byte aligned pointers and strides, row stride >= head_dim)", who);
        return RTK_EUNSUPPORTED;
    }
    if (!fits_buffer_offsets(1, (int64_t)Ls + slack, D, 0, s_stride_l, 2)) {
        set_error("%s: unsupported extent: one head of the shared rows spans 2 GiB or more", who);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

int attn_check_operands(const char* who, const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                        int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8, const float* k_scale,
                        const float* v_scale, int64_t stride8_h, int64_t scale_stride_h, const void* out, int Lq, int Lk,
                        int q_offset, int D, int dtype, float scale, int q_slack, int kv_slack) {
    RTK_CHECK_ARG(scale > 0.f && std::isfinite(scale), "%s: scale must be positive and finite", who);
    RTK_CHECK_ARG(q_offset >= Lk - Lq && q_offset <= 0x3fffffff,
                  "%s: q_offset %d < Lk - Lq = %d (the last keys would be visible to no row)", who, q_offset, Lk - Lq);
    const size_t es = dtype == RTK_F32 ? 4 : 2;
    // 16-byte row chunks, and per-head extents (the head offset is folded into the descriptor base) that fit the 31-bit
    // buffer offsets with a tile of slack rows
    const bool aligned = (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)k8 | (uintptr_t)v8) & 15) == 0 &&
                         (((uintptr_t)k_scale | (uintptr_t)v_scale) & 3) == 0 && stride8_h % 16 == 0 &&
                         (q_stride_h * (int64_t)es) % 16 == 0 && (q_stride_l * (int64_t)es) % 16 == 0 &&
                         (kv_stride_h * (int64_t)es) % 16 == 0 && (kv_stride_l * (int64_t)es) % 16 == 0;
    if (!aligned || q_stride_l < D || kv_stride_l < D || q_stride_h < 0 || kv_stride_h < 0 || stride8_h < 0 || scale_stride_h < 0) {
        set_error("%s: unsupported layout (16-byte aligned pointers and strides, row strides >= head_dim)", who);
        return RTK_EUNSUPPORTED;
    }
    if (!fits_buffer_offsets(1, (int64_t)Lq + q_slack, D, 0, q_stride_l, es) ||
        !fits_buffer_offsets(1, (int64_t)Lk + kv_slack, D, 0, kv_stride_l, es)) {
        set_error("%s: unsupported extent: one head of q or k / v spans 2 GiB or more", who);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

int attn_check_workspace(const char* who, const char* query, size_t need, const void* workspace, size_t workspace_bytes) {
    if (!need) return RTK_OK;
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu bytes; query %s)", who, workspace ? workspace_bytes : (size_t)0, need, query);
        return RTK_EWORKSPACE;
    }
    RTK_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    return RTK_OK;
}

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
    return attn_forward(who, "rtk_attention_workspace_bytes",
                        AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                 scale, workspace, workspace_bytes, (hipStream_t)stream},
                        Archive8{}, Shared16{});
}

extern "C" size_t rtk_attention_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype) {
    if (fp8kv_check_shape("rtk_attention_workspace_bytes_fp8kv", Hq, Hkv, Lq, Lk, L8, D, dtype) != RTK_OK) return 0;
    return attn_plan(Hq, Lq, (int)shared_keys(Lk, L8, 0, AT_KT), D, dtype).ws_bytes;
}

extern "C" int rtk_attention_forward_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                           int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                           const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                           int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                           int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                           rtk_stream_t stream) {
    const char* who = "rtk_attention_forward_fp8kv";
    RTK_CHECK_ARG(q && k && v && out, "%s: NULL q / k / v / out pointer", who);
    int rc = fp8kv_check_shape(who, Hq, Hkv, Lq, Lk, L8, D, dtype);
    if (rc != RTK_OK) return rc;
    if (L8 == 0)   // no archive yet: the 16-bit call itself
        return rtk_attention_forward(q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset,
                                     D, dtype, scale, workspace, workspace_bytes, stream);
    Archive8 a8;
    rc = make_archive8(who, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h, a8);
    if (rc != RTK_OK) return rc;
    return attn_forward(who, "rtk_attention_workspace_bytes_fp8kv",
                        AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                 scale, workspace, workspace_bytes, (hipStream_t)stream},
                        a8, Shared16{});
}

extern "C" size_t rtk_attention_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype) {
    if (shared_check_shape("rtk_attention_workspace_bytes_shared", Hq, Hkv, Lq, Lk, L8, Ls, D, dtype, AT_KT) != RTK_OK) return 0;
    return attn_plan(Hq, Lq, (int)shared_keys(Lk, L8, Ls, AT_KT), D, dtype).ws_bytes;
}

extern "C" int rtk_attention_forward_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                            int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                            int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                            const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                            int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                            int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                            rtk_stream_t stream) {
    const char* who = "rtk_attention_forward_shared";
    RTK_CHECK_ARG(q && k && v && out, "%s: NULL q / k / v / out pointer", who);
    int rc = shared_check_shape(who, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype, AT_KT);
    if (rc != RTK_OK) return rc;
    if (Ls == 0)   // no shared rows: the two-segment call itself
        return rtk_attention_forward_fp8kv(q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, k8, v8, k_scale, v_scale, L8,
                                           stride8_h, scale_stride_h, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype, scale, workspace,
                                           workspace_bytes, stream);
    Shared16 s16;
    rc = make_shared16(who, ks, vs, Ls, s_stride_h, s_stride_l, D, AT_KT, s16);
    if (rc != RTK_OK) return rc;
    Archive8 a8;
    rc = make_archive8(who, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h, a8);
    if (rc != RTK_OK) return rc;
    return attn_forward(who, "rtk_attention_workspace_bytes_shared",
                        AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                 scale, workspace, workspace_bytes, (hipStream_t)stream},
                        a8, s16);
}

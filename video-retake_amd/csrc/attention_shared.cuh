// attention_shared.cuh - what attention.hip (the chunk kernels) and attention_decode.hip (the GQA-packed few-row kernel
// and the group kernel) both use: the bounded buffer loads, the archive / shared-rows descriptors and how an entry point
// binds them, the cross-split combine kernel and its launch, and the host-side argument checks of the entry points.  The
// device parts sit in an unnamed namespace: each file instantiates its own copy under the same name, compiled to the
// same code (tools/kernel_diff.py matches kernels by name over all files).
#pragma once
#include <cmath>

#include "fp8kv.cuh"

namespace rtk {
namespace {

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
__device__ __forceinline__ float safe_max(float m) { return m == -INFINITY ? 0.f : m; }

// The e4m3 archive that precedes the 16-bit keys (retake_hip.h "FP8 rows of the compressed cache"): L8 rows per kv head.
struct Archive8 {
    const char *k8, *v8;        // codes, row (h, r) at h * sh8 + r * 128 bytes
    const float *ks, *vs;       // scales, row (h, r) at h * shs + r
    int64_t sh8, shs;
    int L8;
};

// 16-bit rows of ANOTHER buffer that sit between the archive and k / v in sequence order (rtk_attention_forward_shared: a
// fork reads its parent's rows where they lie).  Ls rows per kv head, every one visible to every query row.
struct Shared16 {
    const char *k, *v;          // element (h, l, d) at (h * sh + d) * 2 + l * row_bytes bytes
    int64_t sh;                 // head stride, elements
    uint32_t row_bytes, bytes;  // row stride; extent of one head: the descriptor's bound
    int Ls;
};

// bytes from a head's first row to the end of its last: the bound of the head's buffer descriptor
inline uint32_t rows_extent(int L, int64_t stride_l, int D, size_t es) { return (uint32_t)(((size_t)(L - 1) * stride_l + D) * es); }

template <int DT> __device__ __forceinline__ float ld_elem(const void* p, size_t i) {
    if constexpr (DT == RTK_F32) return ((const float*)p)[i];
    else return H16<DT>::ld(p, i);
}
template <int DT> __device__ __forceinline__ void st_elem(void* p, size_t i, float x) {
    if constexpr (DT == RTK_F32) ((float*)p)[i] = x;
    else H16<DT>::st(p, i, x);
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

// the workspace of a key-split call: nsplit x heads x Lq un-normalised rows of D floats, then their (m, l) pairs
struct Partials {
    float *acc, *ml;
};
inline Partials split_partials(void* ws, int nsplit, int heads, int Lq, int D) {
    float* acc = (float*)ws;
    return Partials{acc, acc ? acc + (size_t)nsplit * heads * Lq * D : nullptr};
}
// the tail of every key-split launch: out[Lq, heads, D] from the partials
template <int DT> int attn_combine(const Partials& p, void* out, int heads, int Lq, int D, int nsplit, hipStream_t st) {
    const size_t total = (size_t)Lq * heads * D;
    hipLaunchKernelGGL((attn_combine_kernel<DT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p.acc, p.ml, (char*)out,
                       heads, Lq, D, nsplit);
    RTK_LAUNCH_CHECK("attn_combine_kernel");
    return RTK_OK;
}

}  // namespace

// what the three entry points of a kernel family take alike (retake_hip.h "Chunk attention"); off: q_offset
struct AttnArgs {
    const void* q;
    int64_t q_sh, q_sl;
    const void *k, *v;
    int64_t kv_sh, kv_sl;
    void* out;
    int Hq, Hkv, Lq, Lk, off, D, dtype;
    float scale;
    void* workspace;
    size_t workspace_bytes;
    hipStream_t st;
};
// the kernels exponentiate in base 2: a logit is q . k * scale * log2(e)
inline float base2_scale(float scale) { return scale * 1.44269504088896340736f; }

// ---- host-side checks shared by rtk_attention_forward*, rtk_attention_decode* and the group call (defined in attention.hip) ----
int attn_check_shape(const char* who, int Hq, int Hkv, int Lq, int Lk, int D, int dtype);
int fp8kv_check_shape(const char* who, int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype);
// scale, q_offset, 16-byte layout and the 2 GiB head extent with q_slack / kv_slack rows the kernels may address past
// the last one (their descriptors bound what is read); k8 .. scale_stride_h: the archive, all zero without one
int attn_check_operands(const char* who, const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                        int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8, const float* k_scale,
                        const float* v_scale, int64_t stride8_h, int64_t scale_stride_h, const void* out, int Lq, int Lk,
                        int q_offset, int D, int dtype, float scale, int q_slack, int kv_slack);
// the shared rows (rtk_attention_*_shared): fp8kv_check_shape plus Ls and the padded total; `tile`: 64 (chunk) or 32 (decode)
int shared_check_shape(const char* who, int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype, int tile);
// NULL pointers (RTK_EINVAL), 16-byte layout and the 2 GiB head extent of the shared rows, with `slack` rows past the last
int shared_check_operands(const char* who, const void* ks, const void* vs, int Ls, int64_t s_stride_h, int64_t s_stride_l, int D,
                          int slack);
// keys of the padded index space [archive | shared | own]: each of the first two rounded up to whole tiles
inline long long shared_keys(int Lk, int L8, int Ls, int tile) {
    return (long long)Lk + ((long long)L8 + tile - 1) / tile * tile + ((long long)Ls + tile - 1) / tile * tile;
}
// what the MFMA kernels of attention_decode.hip take of dtype and head_dim; `kernel`: "packed" or "group"
inline int d128_check_envelope(const char* who, const char* kernel, int D, int dtype) {
    if (dtype != RTK_BF16 && dtype != RTK_F16) {
        set_error("%s: unsupported dtype code %d (the %s kernel takes RTK_BF16 or RTK_F16)", who, dtype, kernel);
        return RTK_EUNSUPPORTED;
    }
    if (D != 128) {
        set_error("%s: unsupported head_dim %d (the %s kernel takes 128)", who, D, kernel);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}
// RTK_EWORKSPACE unless `workspace` holds `need` bytes (need 0: nothing is checked); `query`: the entry point that sizes it
int attn_check_workspace(const char* who, const char* query, size_t need, const void* workspace, size_t workspace_bytes);

// ---- how an entry point binds its archive and shared rows (after its shape check): a8 / s16 stay empty without rows ----
namespace {
// RTK_EINVAL for a NULL archive pointer with L8 > 0
inline int make_archive8(const char* who, const void* k8, const void* v8, const float* k_scale, const float* v_scale, int L8,
                         int64_t stride8_h, int64_t scale_stride_h, Archive8& a8) {
    a8 = Archive8{};
    if (L8 == 0) return RTK_OK;
    RTK_CHECK_ARG(k8 && v8 && k_scale && v_scale, "%s: NULL archive pointer with L8 = %d", who, L8);
    a8 = Archive8{(const char*)k8, (const char*)v8, k_scale, v_scale, stride8_h, scale_stride_h, L8};
    return RTK_OK;
}
// shared_check_operands with Ls > 0; `tile`: the kernel's key tile, the rows it may address past the last
inline int make_shared16(const char* who, const void* ks, const void* vs, int Ls, int64_t s_stride_h, int64_t s_stride_l, int D,
                         int tile, Shared16& s16) {
    s16 = Shared16{};
    if (Ls == 0) return RTK_OK;
    const int rc = shared_check_operands(who, ks, vs, Ls, s_stride_h, s_stride_l, D, tile);
    if (rc != RTK_OK) return rc;
    s16 = Shared16{(const char*)ks, (const char*)vs, s_stride_h, (uint32_t)(s_stride_l * 2), rows_extent(Ls, s_stride_l, D, 2), Ls};
    return RTK_OK;
}
}  // namespace

}  // namespace rtk

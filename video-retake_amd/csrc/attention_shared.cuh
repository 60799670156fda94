// attention_shared.cuh - what attention.hip (the chunk kernels) and attention_decode.hip (the GQA-packed few-row kernel)
// both use: the bounded buffer loads, the archive descriptor, the cross-split combine kernel and the host-side argument
// checks of the entry points.  The device parts sit in an unnamed namespace: each file instantiates its own copy under
// the same name, compiled to the same code (tools/kernel_diff.py matches kernels by name over all files).
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

}  // namespace

// ---- host-side checks shared by rtk_attention_forward(_fp8kv) and rtk_attention_decode(_fp8kv) (attention.hip) ----
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
// RTK_EWORKSPACE unless `workspace` holds `need` bytes (need 0: nothing is checked); `query`: the entry point that sizes it
int attn_check_workspace(const char* who, const char* query, size_t need, const void* workspace, size_t workspace_bytes);

}  // namespace rtk

// attention_decode.hip — the chunk attention of attention.hip for FEW query rows (decode steps, short trailing text),
// GQA-packed (retake_hip.h "Chunk attention", rtk_attention_decode):
//
//   out[i, h, :] = softmax_j(q[h, i, :] . k[h / G, j, :] * scale) . v[h / G, j, :]      j <= q_offset + i, j < Lk
//
// for bf16 / fp16, head_dim 128 and R = G * Lq <= 16.  attn_decode_d128_kernel:
//   * a workgroup = 4 waves = one kv head x one key range (grid nsplit x Hkv).  The R rows (g, i) of the kv head - packed
//     row g * Lq + i is row i of query head hkv * G + g - are the 16 columns of one 16x16x32 MFMA operand, so a K or V row
//     is fetched from HBM once per call, not once per query head;
//   * the range's 32-key tiles go to the waves round robin (tile u of the range to wave u & 3); a wave's K rows go
//     global -> registers and ARE the A operand of S^T = mfma(K, Q) (lane: key lane & 15, 8 channels per k-step), its V
//     rows global -> registers -> a wave-private LDS image, read back transposed (ds_read_b64_tr_b16) as the A operand of
//     O^T = mfma(V^T, P^T).  No workgroup barrier in the key loop; the next tile's loads are issued as soon as the current
//     tile's registers are consumed and stay in flight under its softmax and PV products;
//   * a lane owns ONE packed row (column lane & 15): 8 of a tile's 32 logits, and 4 channels of each of O's 8 d-blocks, so
//     the running rescale is lane-local and max / sum need the lanes 16 and 32 apart;
//   * causal by index per packed row.  A tile holding keys that only some rows see (j > q_offset) runs its PV products
//     once per query position i with the V rows above i's diagonal zeroed, each lane keeping the pass of its own row: a
//     hidden V row reaches no row that does not see it, whatever it holds;
//   * each wave keeps its own (m, l, acc); the four are folded through LDS in wave order 0, 1, 2, 3 and the workgroup
//     leaves ONE un-normalised partial per packed row in the layout attn_combine_kernel reads, which then runs unchanged.
//     No atomics, no flags; plain vector stores.
// The plan (decode_plan) is a function of the shape alone.
// FP8 = true: the keys are [e4m3 archive | 16-bit rows], counted in a key space where the archive is padded to whole
// 32-key tiles (a tile is of one kind).  Archive tiles are dequantised (fp8_dequant16) into the registers / the LDS image
// a 16-bit tile of the dequantised rows would have left, so with L8 % 32 == 0 every fp32 sum is grouped as in the 16-bit
// call over the concatenation.  (The k-steps of S^T take channels 64 a + 16 g + 8 b + j, step 2 a + b, lane group g: 16
// consecutive codes of a row dequantise into one lane's operands of two steps.)
#include "attention_shared.cuh"

namespace rtk {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using i16x4 = __attribute__((ext_vector_type(4))) short;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

constexpr int DEC_R = 16;                 // packed rows a workgroup serves: the MFMA's columns
constexpr int DEC_T = 32;                 // keys per wave tile: the key tile T of retake_hip.h
constexpr int DEC_STEP = 4 * DEC_T;       // keys the four waves take side by side: the granularity of a split
constexpr int DEC_TARGET_WG = 512;        // workgroups wanted (2 per CU; a constant, not a device query)
constexpr int DEC_VPITCH = 288;           // bytes per V row in LDS: 256 + 32, so the 8 rows a 32-lane half reads tile the banks
constexpr int DEC_WAVE_LDS = DEC_T * DEC_VPITCH;
constexpr int DEC_OPITCH = 132;           // floats per packed row of a wave's O image (the fold)
static_assert(DEC_R * DEC_OPITCH * 4 <= DEC_WAVE_LDS, "a wave's O image reuses its V image");

template <int DT> __device__ __forceinline__ f32x4 mma32(const u32x4& a, const u32x4& b, const f32x4& c) {
    if constexpr (DT == RTK_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// the wave's LDS writes before, its LDS reads after (the image is wave-private: no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int DT, bool FP8>
__global__ __launch_bounds__(256, 2) void attn_decode_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq,
    int G, int Lq, int Lk, int off, float c2, int keys_per_split, Archive8 a8) {
    constexpr bool SHARED = false;
    const Shared16 s16{};
#include "attention_decode_d128_body.inc"
}

// the same body over [e4m3 archive (may be empty) | shared 16-bit rows | own 16-bit rows]: Lk and off describe the own rows
template <int DT>
__global__ __launch_bounds__(256, 2) void attn_decode_d128_shared_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq,
    int G, int Lq, int Lk, int off, float c2, int keys_per_split, Archive8 a8, Shared16 s16) {
    constexpr bool FP8 = true, SHARED = true;
#include "attention_decode_d128_body.inc"
}

struct DecodePlan {
    int nsplit, keys_per_split;
    size_t ws_bytes;
};

// retake_hip.h states this rule; a function of the shape alone.  `keys`: Lk, plus the archive padded to whole tiles.
DecodePlan decode_plan(int Hq, int Hkv, int Lq, long long keys) {
    long long ns = (DEC_TARGET_WG + Hkv - 1) / Hkv;
    const long long by_keys = (keys + DEC_STEP - 1) / DEC_STEP;
    if (ns > by_keys) ns = by_keys;
    if (ns < 1) ns = 1;
    long long kps = (keys + ns - 1) / ns;
    kps = (kps + DEC_STEP - 1) / DEC_STEP * DEC_STEP;
    ns = (keys + kps - 1) / kps;
    return DecodePlan{(int)ns, (int)kps, (size_t)ns * Hq * Lq * (128 + 2) * sizeof(float)};
}

inline long long decode_fp8kv_keys(int Lk, int L8) { return (long long)Lk + ((long long)L8 + DEC_T - 1) / DEC_T * DEC_T; }

// what the packed kernel takes of the shapes attn_check_shape admits
int decode_check_envelope(const char* who, int Hq, int Hkv, int Lq, int D, int dtype) {
    if (dtype != RTK_BF16 && dtype != RTK_F16) {
        set_error("%s: unsupported dtype code %d (the packed kernel takes RTK_BF16 or RTK_F16)", who, dtype);
        return RTK_EUNSUPPORTED;
    }
    if (D != 128) {
        set_error("%s: unsupported head_dim %d (the packed kernel takes 128)", who, D);
        return RTK_EUNSUPPORTED;
    }
    if ((long long)(Hq / Hkv) * Lq > DEC_R) {
        set_error("%s: unsupported shape: (Hq / Hkv) * Lq = %d * %d packed rows (at most %d)", who, Hq / Hkv, Lq, DEC_R);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

template <int DT, bool FP8>
int decode_launch(const DecodePlan& pl, const void* q, int64_t q_sh, int64_t q_sl, const void* k, const void* v, int64_t kv_sh,
                  int64_t kv_sl, const Archive8& a8, void* out, int Hq, int Hkv, int Lq, int Lk, int off, float c2, void* ws,
                  hipStream_t st) {
    constexpr int D = 128;
    float* part_acc = (float*)ws;
    float* part_ml = part_acc + (size_t)pl.nsplit * Hq * Lq * D;
    const uint32_t kv_bytes = (uint32_t)(((size_t)(Lk - 1) * kv_sl + D) * 2);
    hipLaunchKernelGGL((attn_decode_d128_kernel<DT, FP8>), dim3((unsigned)pl.nsplit, (unsigned)Hkv), dim3(256), 0, st,
                       (const char*)q, q_sh, q_sl, (const char*)k, (const char*)v, kv_sh, (uint32_t)(kv_sl * 2), kv_bytes, part_acc,
                       part_ml, Hq, Hq / Hkv, Lq, Lk, off, c2, pl.keys_per_split, a8);
    RTK_LAUNCH_CHECK("attn_decode_d128_kernel");
    const size_t total = (size_t)Lq * Hq * D;
    hipLaunchKernelGGL((attn_combine_kernel<DT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part_acc, part_ml,
                       (char*)out, Hq, Lq, D, pl.nsplit);
    RTK_LAUNCH_CHECK("attn_combine_kernel");
    return RTK_OK;
}

template <int DT>
int decode_launch_shared(const DecodePlan& pl, const void* q, int64_t q_sh, int64_t q_sl, const void* k, const void* v,
                         int64_t kv_sh, int64_t kv_sl, const Archive8& a8, const Shared16& s16, void* out, int Hq, int Hkv, int Lq,
                         int Lk, int off, float c2, void* ws, hipStream_t st) {
    constexpr int D = 128;
    float* part_acc = (float*)ws;
    float* part_ml = part_acc + (size_t)pl.nsplit * Hq * Lq * D;
    const uint32_t kv_bytes = (uint32_t)(((size_t)(Lk - 1) * kv_sl + D) * 2);
    hipLaunchKernelGGL((attn_decode_d128_shared_kernel<DT>), dim3((unsigned)pl.nsplit, (unsigned)Hkv), dim3(256), 0, st,
                       (const char*)q, q_sh, q_sl, (const char*)k, (const char*)v, kv_sh, (uint32_t)(kv_sl * 2), kv_bytes, part_acc,
                       part_ml, Hq, Hq / Hkv, Lq, Lk, off, c2, pl.keys_per_split, a8, s16);
    RTK_LAUNCH_CHECK("attn_decode_d128_shared_kernel");
    const size_t total = (size_t)Lq * Hq * D;
    hipLaunchKernelGGL((attn_combine_kernel<DT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part_acc, part_ml,
                       (char*)out, Hq, Lq, D, pl.nsplit);
    RTK_LAUNCH_CHECK("attn_combine_kernel");
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" size_t rtk_attention_decode_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype) {
    const char* who = "rtk_attention_decode_workspace_bytes";
    if (attn_check_shape(who, Hq, Hkv, Lq, Lk, D, dtype) != RTK_OK) return 0;
    if (decode_check_envelope(who, Hq, Hkv, Lq, D, dtype) != RTK_OK) return 0;
    return decode_plan(Hq, Hkv, Lq, Lk).ws_bytes;
}

extern "C" int rtk_attention_decode(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                    int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                    int q_offset, int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                    rtk_stream_t stream) {
    const char* who = "rtk_attention_decode";
    RTK_CHECK_ARG(q && k && v && out, "%s: NULL q / k / v / out pointer", who);
    int rc = attn_check_shape(who, Hq, Hkv, Lq, Lk, D, dtype);
    if (rc != RTK_OK) return rc;
    rc = decode_check_envelope(who, Hq, Hkv, Lq, D, dtype);
    if (rc != RTK_OK) return rc;
    rc = attn_check_operands(who, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, nullptr, nullptr, nullptr, nullptr,
                             0, 0, out, Lq, Lk, q_offset, D, dtype, scale, 0, DEC_T);
    if (rc != RTK_OK) return rc;
    const DecodePlan pl = decode_plan(Hq, Hkv, Lq, Lk);
    rc = attn_check_workspace(who, "rtk_attention_decode_workspace_bytes", pl.ws_bytes, workspace, workspace_bytes);
    if (rc != RTK_OK) return rc;
    const float c2 = scale * 1.44269504088896340736f;   // the kernels exponentiate in base 2
    if (dtype == RTK_BF16)
        return decode_launch<RTK_BF16, false>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, Archive8{}, out, Hq,
                                              Hkv, Lq, Lk, q_offset, c2, workspace, (hipStream_t)stream);
    return decode_launch<RTK_F16, false>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, Archive8{}, out, Hq, Hkv,
                                         Lq, Lk, q_offset, c2, workspace, (hipStream_t)stream);
}

extern "C" size_t rtk_attention_decode_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype) {
    const char* who = "rtk_attention_decode_workspace_bytes_fp8kv";
    if (fp8kv_check_shape(who, Hq, Hkv, Lq, Lk, L8, D, dtype) != RTK_OK) return 0;
    if (decode_check_envelope(who, Hq, Hkv, Lq, D, dtype) != RTK_OK) return 0;
    return decode_plan(Hq, Hkv, Lq, decode_fp8kv_keys(Lk, L8)).ws_bytes;
}

extern "C" int rtk_attention_decode_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                          int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                          const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                          int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                          int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                          rtk_stream_t stream) {
    const char* who = "rtk_attention_decode_fp8kv";
    RTK_CHECK_ARG(q && k && v && out, "%s: NULL q / k / v / out pointer", who);
    int rc = fp8kv_check_shape(who, Hq, Hkv, Lq, Lk, L8, D, dtype);
    if (rc != RTK_OK) return rc;
    rc = decode_check_envelope(who, Hq, Hkv, Lq, D, dtype);
    if (rc != RTK_OK) return rc;
    if (L8 == 0)   // no archive yet: the 16-bit packed call itself
        return rtk_attention_decode(q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D,
                                    dtype, scale, workspace, workspace_bytes, stream);
    RTK_CHECK_ARG(k8 && v8 && k_scale && v_scale, "%s: NULL archive pointer with L8 = %d", who, L8);
    rc = attn_check_operands(who, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, k8, v8, k_scale, v_scale, stride8_h,
                             scale_stride_h, out, Lq, Lk, q_offset, D, dtype, scale, 0, DEC_T);
    if (rc != RTK_OK) return rc;
    const DecodePlan pl = decode_plan(Hq, Hkv, Lq, decode_fp8kv_keys(Lk, L8));
    rc = attn_check_workspace(who, "rtk_attention_decode_workspace_bytes_fp8kv", pl.ws_bytes, workspace, workspace_bytes);
    if (rc != RTK_OK) return rc;
    const float c2 = scale * 1.44269504088896340736f;
    const Archive8 a8{(const char*)k8, (const char*)v8, k_scale, v_scale, stride8_h, scale_stride_h, L8};
    if (dtype == RTK_BF16)
        return decode_launch<RTK_BF16, true>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, a8, out, Hq, Hkv, Lq,
                                             Lk, q_offset, c2, workspace, (hipStream_t)stream);
    return decode_launch<RTK_F16, true>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, a8, out, Hq, Hkv, Lq, Lk,
                                        q_offset, c2, workspace, (hipStream_t)stream);
}

extern "C" size_t rtk_attention_decode_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype) {
    const char* who = "rtk_attention_decode_workspace_bytes_shared";
    if (shared_check_shape(who, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype, DEC_T) != RTK_OK) return 0;
    if (decode_check_envelope(who, Hq, Hkv, Lq, D, dtype) != RTK_OK) return 0;
    return decode_plan(Hq, Hkv, Lq, shared_keys(Lk, L8, Ls, DEC_T)).ws_bytes;
}

extern "C" int rtk_attention_decode_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                           int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                           int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                           const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                           int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                           int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                           rtk_stream_t stream) {
    const char* who = "rtk_attention_decode_shared";
    RTK_CHECK_ARG(q && k && v && out, "%s: NULL q / k / v / out pointer", who);
    int rc = shared_check_shape(who, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype, DEC_T);
    if (rc != RTK_OK) return rc;
    rc = decode_check_envelope(who, Hq, Hkv, Lq, D, dtype);
    if (rc != RTK_OK) return rc;
    if (Ls == 0)   // no shared rows: the two-segment packed call itself
        return rtk_attention_decode_fp8kv(q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, k8, v8, k_scale, v_scale, L8,
                                          stride8_h, scale_stride_h, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype, scale, workspace,
                                          workspace_bytes, stream);
    rc = shared_check_operands(who, ks, vs, Ls, s_stride_h, s_stride_l, D, DEC_T);
    if (rc != RTK_OK) return rc;
    Archive8 a8{};
    if (L8 > 0) {
        RTK_CHECK_ARG(k8 && v8 && k_scale && v_scale, "%s: NULL archive pointer with L8 = %d", who, L8);
        a8 = Archive8{(const char*)k8, (const char*)v8, k_scale, v_scale, stride8_h, scale_stride_h, L8};
    }
    rc = attn_check_operands(who, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, a8.k8, a8.v8, a8.ks, a8.vs, a8.sh8,
                             a8.shs, out, Lq, Lk, q_offset, D, dtype, scale, 0, DEC_T);
    if (rc != RTK_OK) return rc;
    const DecodePlan pl = decode_plan(Hq, Hkv, Lq, shared_keys(Lk, L8, Ls, DEC_T));
    rc = attn_check_workspace(who, "rtk_attention_decode_workspace_bytes_shared", pl.ws_bytes, workspace, workspace_bytes);
    if (rc != RTK_OK) return rc;
    const float c2 = scale * 1.44269504088896340736f;
    const Shared16 s16{(const char*)ks, (const char*)vs, s_stride_h, (uint32_t)(s_stride_l * 2),
                       (uint32_t)(((size_t)(Ls - 1) * s_stride_l + D) * 2), Ls};
    if (dtype == RTK_BF16)
        return decode_launch_shared<RTK_BF16>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, a8, s16, out, Hq, Hkv,
                                              Lq, Lk, q_offset, c2, workspace, (hipStream_t)stream);
    return decode_launch_shared<RTK_F16>(pl, q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, a8, s16, out, Hq, Hkv, Lq,
                                         Lk, q_offset, c2, workspace, (hipStream_t)stream);
}

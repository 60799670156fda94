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
    using Hh = H16<DT>;
    __shared__ __attribute__((aligned(16))) char lds[4 * DEC_WAVE_LDS];   // [wave]: V tile, then the wave's O
    __shared__ float ml_s[4][DEC_R][2];
    // FP8: from here on Lk and off count in the padded key space
    const int L8 = FP8 ? a8.L8 : 0, L8p = (L8 + DEC_T - 1) / DEC_T * DEC_T;
    if constexpr (FP8) {
        Lk += L8p;
        off += L8p;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // packed row (column) and lane group
    const int split = blockIdx.x, hkv = blockIdx.y, R = G * Lq;
    const int qi = c % Lq, qg = c / Lq;       // query position and head-in-group of packed row c
    const int k_lo = split * keys_per_split;
    const int k_hi = min(min(Lk, off + Lq), k_lo + keys_per_split);   // exclusive: first key no row of the range sees
    const int vis_r = min(off + qi, Lk - 1);                          // last key packed row c sees

    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(k + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(v + (int64_t)hkv * kv_sh * 2, kv_bytes);
    __amdgpu_buffer_rsrc_t rk8 = rk, rv8 = rk, rks = rk, rvs = rk;
    if constexpr (FP8) {
        rk8 = bounded_rsrc(a8.k8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rv8 = bounded_rsrc(a8.v8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rks = bounded_rsrc(a8.ks + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
        rvs = bounded_rsrc(a8.vs + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
    }

    // the byte offset, within a 256-byte row, of the 16-byte chunk this lane feeds to k-step s
    auto step_off = [&](int s) { return 128 * (s >> 1) + 32 * g + 16 * (s & 1); };
    // Q fragments (B operand): packed row c, zero for c >= R
    u32x4 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = u32x4{0u, 0u, 0u, 0u};
    if (c < R) {
        const char* qr = q + ((int64_t)(hkv * G + qg) * q_sh + (int64_t)qi * q_sl) * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const u32x4*)(qr + step_off(s));
    }

    // One tile's operands, in flight from the moment the previous tile's are consumed.  16-bit tile: kr[4 b + s] = the step-s chunk of key row 16 b + c; vr[u] = chunk c of
    // V row 4 u + g.  Archive tile: kr[2 b + a] = codes 16 (4 a + g) .. + 15 of key row 16 b + c, its scale in kr[4][b];
    // vr[u] = codes 16 (lane & 7) .. + 15 of V row 8 u + (lane >> 3), its scale in vr[4][u].
    u32x4 kr[8], vr[8];
    auto load_k = [&](int kb) {
        if constexpr (FP8) {
            if (kb < L8p) {   // rows >= L8 of the last archive tile: zero codes, zero scales
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const uint32_t row = (uint32_t)(kb + 16 * b + c);
#pragma unroll
                    for (int a = 0; a < 2; ++a) kr[2 * b + a] = load16(rk8, row * 128u + 16u * (4 * a + g));
                    kr[4][b] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rks, row * 4u, 0, 0);
                }
                return;
            }
            kb -= L8p;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kr[4 * b + s] = load16(rk, (uint32_t)(kb + 16 * b + c) * kv_row_bytes + (uint32_t)step_off(s));
    };
    auto load_v = [&](int kb) {
        if constexpr (FP8) {
            if (kb < L8p) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t row = (uint32_t)(kb + 8 * u + (lane >> 3));
                    vr[u] = load16(rv8, row * 128u + 16u * (lane & 7));
                    vr[4][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rvs, row * 4u, 0, 0);
                }
                return;
            }
            kb -= L8p;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) vr[u] = load16(rv, (uint32_t)(kb + 4 * u + g) * kv_row_bytes + 16u * c);
    };

    char* vt = lds + wave * DEC_WAVE_LDS;
    // transposed V reads: lane 4 q_ + p_ of a 16-lane group supplies row q_ of a 4-key block, columns 4 p_ .. 4 p_ + 3 of a
    // d-block; it receives column c of the block's 4 rows.  Group g takes the blocks at keys 4 g and 16 + 4 g: the keys of
    // the lane's own logits, in the order they are packed below.
    const int v_rd = DEC_VPITCH * (4 * g + (c >> 2)) + 8 * (c & 3);

    f32x4 oacc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // tile kb; `next`: this wave has a tile at kb + DEC_STEP, whose loads are issued as soon as the registers are free
    auto process = [&](int kb, bool next) {
        bool arch = false;
        if constexpr (FP8) arch = kb < L8p;
        u32x4 ka[8];
        if (arch) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    fp8_dequant16<DT>(kr[2 * b + a], __uint_as_float(kr[4][b]), ka[4 * b + 2 * a], ka[4 * b + 2 * a + 1]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                u32x4 x, y;
                fp8_dequant16<DT>(vr[u], __uint_as_float(vr[4][u]), x, y);
                char* w = vt + DEC_VPITCH * (8 * u + (lane >> 3)) + 32 * (lane & 7);
                *(u32x4*)w = x;
                *(u32x4*)(w + 16) = y;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ka[e] = kr[e];
#pragma unroll
            for (int u = 0; u < 8; ++u) *(u32x4*)(vt + DEC_VPITCH * (4 * u + g) + 16 * c) = vr[u];
        }
        if (next) load_v(kb + DEC_STEP);
        wave_lds_sync();
        // logits: s0[e] = key 4 g + e, s1[e] = key 16 + 4 g + e of the tile, packed row c
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            s0 = mma32<DT>(ka[s], qf[s], s0);
            s1 = mma32<DT>(ka[4 + s], qf[s], s1);
        }
        if (next) load_k(kb + DEC_STEP);
        // the last key this row sees: its diagonal or the end of the keys - of an archive tile, which every row sees
        // whole, the last archive row
        const int lim = (arch ? L8 - 1 : vis_r) - kb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * g + e > lim) s0[e] = -INFINITY;
            if (16 + 4 * g + e > lim) s1[e] = -INFINITY;
        }
        float mx = fmaxf(fmaxf(fmaxf(s0[0], s1[0]), fmaxf(s0[1], s1[1])), fmaxf(fmaxf(s0[2], s1[2]), fmaxf(s0[3], s1[3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
        const float mnew = fmaxf(m, mx * c2);
        const float alpha = __builtin_amdgcn_exp2f(m - safe_max(mnew));
#pragma unroll
        for (int db = 0; db < 8; ++db) oacc[db] *= alpha;
        l *= alpha;
        m = mnew;
        const float nm = -safe_max(m);
        float ls = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s0[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], c2, nm));
            s1[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[e], c2, nm));
            ls += s0[e] + s1[e];
        }
        l += ls;
        const u32x4 pf = {Hh::pack2(s0[0], s0[1]), Hh::pack2(s0[2], s0[3]), Hh::pack2(s1[0], s1[1]), Hh::pack2(s1[2], s1[3])};
        auto v_frag = [&](int db) {
            u32x2 h2[2];
#pragma unroll
            for (int jh = 0; jh < 2; ++jh) {
                const i16x4 t4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) i16x4*)(vt + v_rd + DEC_VPITCH * 16 * jh + 32 * db));
                h2[jh] = __builtin_bit_cast(u32x2, t4);
            }
            return u32x4{h2[0][0], h2[0][1], h2[1][0], h2[1][1]};
        };
        if (arch || kb + DEC_T - 1 <= off) {   // every row sees every key of the tile that exists (keys >= Lk read as zero)
#pragma unroll
            for (int db = 0; db < 8; ++db) oacc[db] = mma32<DT>(v_frag(db), pf, oacc[db]);
        } else {
            // one pass per query position: V rows above its diagonal zeroed, the lanes of its packed rows keep the result
            for (int i = 0; i < Lq; ++i) {
                const int li = min(off + i, Lk - 1) - kb;
                u32x4 keep;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int key = 16 * (w >> 1) + 4 * g + 2 * (w & 1);
                    keep[w] = (key <= li ? 0xffffu : 0u) | (key + 1 <= li ? 0xffff0000u : 0u);
                }
#pragma unroll
                for (int db = 0; db < 8; ++db) {
                    const f32x4 t = mma32<DT>(v_frag(db) & keep, pf, oacc[db]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) oacc[db][e] = qi == i ? t[e] : oacc[db][e];
                }
            }
        }
        wave_lds_sync();   // the reads above before the next tile's writes
    };

    // this wave's tiles: u = wave, wave + 4, ... of the range
    const int kb0 = k_lo + DEC_T * wave;
    if (kb0 < k_hi) {
        load_k(kb0);
        load_v(kb0);
    }
    for (int kb = kb0; kb < k_hi; kb += DEC_STEP) process(kb, kb + DEC_STEP < k_hi);

    // fold the four waves in wave order; the workgroup leaves one partial per packed row
    l += __shfl_xor(l, 16, WAVE);
    l += __shfl_xor(l, 32, WAVE);
    {
        float* ow = (float*)vt;
#pragma unroll
        for (int db = 0; db < 8; ++db) *(f32x4*)(ow + c * DEC_OPITCH + 16 * db + 4 * g) = oacc[db];
        if (g == 0) {
            ml_s[wave][c][0] = m;
            ml_s[wave][c][1] = l;
        }
    }
    __syncthreads();
    const int row = tid >> 4, ch = tid & 15;   // packed row, channels 8 ch .. 8 ch + 7
    if (row >= R) return;
    float mg = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mg = fmaxf(mg, ml_s[w][row][0]);
    f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float mw = ml_s[w][row][0];
        if (mw == -INFINITY) continue;   // the wave had no key this row sees
        const float wt = __builtin_amdgcn_exp2f(mw - mg);
        const float* ow = (const float*)(lds + w * DEC_WAVE_LDS) + row * DEC_OPITCH + 8 * ch;
        const f32x4 a = *(const f32x4*)ow, b = *(const f32x4*)(ow + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            n0[e] = __builtin_fmaf(wt, a[e], n0[e]);
            n1[e] = __builtin_fmaf(wt, b[e], n1[e]);
        }
        den = __builtin_fmaf(wt, ml_s[w][row][1], den);
    }
    const size_t prow = ((size_t)split * Hq + (size_t)(hkv * G + row / Lq)) * Lq + row % Lq;
    float* pa = part_acc + prow * 128 + 8 * ch;
    *(f32x4*)pa = n0;
    *(f32x4*)(pa + 4) = n1;
    if (ch == 0) *(float2*)(part_ml + 2 * prow) = make_float2(mg, den);
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

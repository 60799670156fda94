// pivotkv_archive.hip - the eviction of a chunk's (layer, chunk) units into the e4m3 archive, in ONE launch
// (retake_hip.h "FP8 rows of the compressed cache"): what compact_units_kernel does in place on 16-bit rows, with the
// kept rows quantised into buffers of their own instead.  Source and destination never alias, so there are no tickets
// and no flags: every workgroup loads, (re-rotates K,) reduces max |x| per row, converts and stores.
//
// Roofline: HBM.  Per unit  2 x keep x Hkv x D x 2 bytes read (kept K and V rows)  +  2 x keep x Hkv x (D + 4) written.
//
// A row of one kv head = 8 lanes: lane c holds the 16-byte chunks at channels 8c and 64 + 8c - the pair the rotation
// mixes (rotate_chunk_pair, shared with the compaction kernel) - so max |x| is three DPP steps inside a half row of
// lanes, and the codes leave as two 8-byte stores per lane (64 contiguous bytes per 8 lanes).
#include "fp8kv.cuh"

namespace rtk {
namespace {

struct ArchiveUnits {
    rtk_archive_unit u[RTK_ARCHIVE_MAX_UNITS];
};

constexpr int ARC_BLOCK = 256;
constexpr int ARC_D = 128;
constexpr int ARC_R = ARC_BLOCK / 8;   // rows per workgroup
constexpr int ARC_HU = 4;              // kv heads whose rows are requested together

using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

template <int CTRL> __device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// max over the 8 lanes of a row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
__device__ __forceinline__ float max8(float a) {
    a = fmaxf(a, dpp_f<0xB1>(a));
    a = fmaxf(a, dpp_f<0x4E>(a));
    return fmaxf(a, dpp_f<0x141>(a));
}

template <int DT>
__device__ __forceinline__ void archive_row(const u32x4& lo, const u32x4& hi, char* codes, float* scale, int c, bool active) {
    const float amax = max8(fmaxf(fp8_chunk_amax<DT>(lo), fp8_chunk_amax<DT>(hi)));
    const int e = fp8_row_exp(amax);
    uint32_t a0, a1, b0, b1;
    fp8_quant_chunk<DT>(lo, -e, a0, a1);
    fp8_quant_chunk<DT>(hi, -e, b0, b1);
    if (active) {
        *(u32x2*)(codes + 8 * c) = u32x2{a0, a1};
        *(u32x2*)(codes + 64 + 8 * c) = u32x2{b0, b1};
        if (c == 0) *scale = fp8_exp2i(e);
    }
}

template <int DT, bool ROTATE>
__global__ __launch_bounds__(ARC_BLOCK) void archive_units_kernel(ArchiveUnits units, int Hkv, int keep, int P,
                                                                  const float* __restrict__ inv_freq, float scaling,
                                                                  RowSel rs, int round_mode) {
    constexpr int D = ARC_D, h2 = D / 2, ES = 2, HU = ARC_HU;
    const int tid = threadIdx.x, b = blockIdx.x;
    const rtk_archive_unit& un = units.u[blockIdx.y];
    const int rl = tid >> 3, c = tid & 7, d = 8 * c;
    const int r = b * ARC_R + rl;
    const bool active = r < keep;
    const int rc = min(r, keep - 1);
    long long id[3] = {0, 0, 0};
    if constexpr (ROTATE) {
#pragma unroll
        for (int p = 0; p < 3; ++p) id[p] = un.pos_src[(size_t)min(p, P - 1) * un.pos_src_stride + rc];
    }
    const int64_t l = un.keep_idx ? un.keep_idx[rc] : (int64_t)rc;
    float c1[8], s1[8], c2[8], s2[8];
    if constexpr (ROTATE) {
        const float pid[3] = {(float)id[0], (float)id[1], (float)id[2]};
        rope_chunk<8>(inv_freq, rs, d, h2, pid, scaling, round_mode, c1, s1, c2, s2);
    }
    const char* ks = (const char*)un.k_src;
    const char* vs = (const char*)un.v_src;
    for (int h0 = 0; h0 < Hkv; h0 += HU) {
        u32x4 v_lo[HU], v_hi[HU], k_lo[HU], k_hi[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int h = min(h0 + u, Hkv - 1);
            const char* vr = vs + ((size_t)h * un.v_src_stride_h + (size_t)l * D + d) * ES;
            const char* kr = ks + ((size_t)h * un.k_src_stride_h + (size_t)l * D + d) * ES;
            v_lo[u] = *(const u32x4*)vr;
            v_hi[u] = *(const u32x4*)(vr + h2 * ES);
            k_lo[u] = *(const u32x4*)kr;
            k_hi[u] = *(const u32x4*)(kr + h2 * ES);
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int h = min(h0 + u, Hkv - 1);
            const bool on = active && h0 + u < Hkv;
            const size_t co = (size_t)h * un.dst_stride_h + (size_t)rc * D, so = (size_t)h * un.scale_stride_h + rc;
            if constexpr (ROTATE) {   // kept K = the un-rotated row rotated at its new ids, rounded to the model dtype first
                u32x4 olo, ohi;
                rotate_chunk_pair<DT>(k_lo[u], k_hi[u], c1, s1, c2, s2, olo, ohi);
                archive_row<DT>(olo, ohi, (char*)un.k8 + co, un.k_scale + so, c, on);
            } else {
                archive_row<DT>(k_lo[u], k_hi[u], (char*)un.k8 + co, un.k_scale + so, c, on);
            }
            archive_row<DT>(v_lo[u], v_hi[u], (char*)un.v8 + co, un.v_scale + so, c, on);
        }
    }
    // ids of the kept tokens -> the layer's position cache, once per unit
    if (un.pos_dst) {
        for (int i = tid; i < P * ARC_R; i += ARC_BLOCK) {
            const int p = i / ARC_R, rr = b * ARC_R + (i - p * ARC_R);
            if (rr < keep) un.pos_dst[(size_t)p * un.pos_dst_stride + rr] = un.pos_src[(size_t)p * un.pos_src_stride + rr];
        }
    }
}

// thread -> 16 codes of one row: dense rows of the model dtype
template <int DT>
__global__ __launch_bounds__(256) void fp8kv_dequant_kernel(const char* __restrict__ codes, int64_t codes_sh,
                                                            const float* __restrict__ scales, int64_t scale_sh,
                                                            char* __restrict__ out, int64_t out_sh, int L) {
    const int h = blockIdx.y;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx >> 3;
    const int cc = (int)(idx & 7);
    if (row >= L) return;
    const u32x4 c = *(const u32x4*)(codes + (size_t)h * codes_sh + (size_t)row * ARC_D + 16 * cc);
    const float s = scales[(size_t)h * scale_sh + row];
    u32x4 a, b;
    fp8_dequant16<DT>(c, s, a, b);
    char* o = out + ((size_t)h * out_sh + (size_t)row * ARC_D + 16 * cc) * 2;
    *(u32x4*)o = a;
    *(u32x4*)(o + 16) = b;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_archive_batched(const rtk_archive_unit* units, int n_units, int Hkv, int D, int keep, int P,
                                           int dtype, int k_mode, const float* inv_freq, float attention_scaling,
                                           const int* sections_host, int nsec, int round_mode, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_archive_batched";
    RTK_CHECK_ARG(units && n_units >= 1, "%s: no units", who);
    RTK_CHECK_ARG(Hkv >= 1 && keep >= 1, "%s: bad shape", who);
    RTK_CHECK_ARG(k_mode == RTK_COMPACT_K_ROTATE || k_mode == RTK_COMPACT_K_COPY, "%s: k_mode %d (RTK_COMPACT_K_ROTATE or _COPY)", who, k_mode);
    RTK_CHECK_ARG(P == 0 || P == 1 || P == 3, "%s: P must be 0, 1 or 3, got %d", who, P);
    RTK_CHECK_ARG(k_mode != RTK_COMPACT_K_ROTATE || (inv_freq && P > 0), "%s: the rotation needs inv_freq and the new ids", who);
    if ((dtype != RTK_BF16 && dtype != RTK_F16) || D != ARC_D) {
        set_error("%s: unsupported dtype code %d / head_dim %d (RTK_BF16 or RTK_F16 with head_dim 128)", who, dtype, D);
        return RTK_EUNSUPPORTED;
    }
    for (int i = 0; i < n_units; ++i) {
        const rtk_archive_unit& u = units[i];
        RTK_CHECK_ARG(u.k_src && u.v_src && u.k8 && u.v8 && u.k_scale && u.v_scale, "%s: unit %d: NULL pointer", who, i);
        RTK_CHECK_ARG(k_mode != RTK_COMPACT_K_ROTATE || u.pos_src, "%s: unit %d: the rotation needs pos_src", who, i);
        RTK_CHECK_ARG(!u.pos_dst || (u.pos_src && P > 0), "%s: unit %d: pos_dst needs pos_src and P", who, i);
        RTK_CHECK_ARG(u.k_src_stride_h >= 0 && u.v_src_stride_h >= 0 && u.dst_stride_h >= 0 && u.scale_stride_h >= 0,
                      "%s: unit %d: negative stride", who, i);
        const bool aligned = (u.k_src_stride_h * 2) % 16 == 0 && (u.v_src_stride_h * 2) % 16 == 0 && u.dst_stride_h % 16 == 0 &&
                             (((uintptr_t)u.k_src | (uintptr_t)u.v_src | (uintptr_t)u.k8 | (uintptr_t)u.v8) & 15) == 0 &&
                             (((uintptr_t)u.k_scale | (uintptr_t)u.v_scale) & 3) == 0;
        if (!aligned) {
            set_error("%s: unit %d: row pointers and strides must be 16-byte aligned", who, i);
            return RTK_EUNSUPPORTED;
        }
    }
    RowSel rs;
    if (k_mode == RTK_COMPACT_K_ROTATE) {
        const int rc = make_rowsel(rs, P, D, sections_host, nsec, who);
        if (rc != RTK_OK) return rc;
    } else {
        for (int d = 0; d < 256; ++d) rs.row[d] = 0;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nb = (keep + ARC_R - 1) / ARC_R;
    for (int b = 0; b < n_units; b += RTK_ARCHIVE_MAX_UNITS) {
        const int n = std::min(RTK_ARCHIVE_MAX_UNITS, n_units - b);
        const ArchiveUnits au = pad_units<ArchiveUnits>(units + b, n);
#define RTK_LAUNCH_ARC(DTV, ROT)                                                                                          \
    RTK_LAUNCH(KID_ARCHIVE, (archive_units_kernel<DTV, ROT>), dim3(nb, n), dim3(ARC_BLOCK), 0, st, au, Hkv, keep, P, inv_freq, \
               attention_scaling, rs, round_mode)
        if (k_mode == RTK_COMPACT_K_ROTATE) {
            if (dtype == RTK_BF16) RTK_LAUNCH_ARC(RTK_BF16, true);
            else RTK_LAUNCH_ARC(RTK_F16, true);
        } else {
            if (dtype == RTK_BF16) RTK_LAUNCH_ARC(RTK_BF16, false);
            else RTK_LAUNCH_ARC(RTK_F16, false);
        }
#undef RTK_LAUNCH_ARC
        RTK_LAUNCH_CHECK("archive_units_kernel");
    }
    return RTK_OK;
}

extern "C" int rtk_fp8kv_dequant(const void* codes, int64_t codes_stride_h, const float* scales, int64_t scale_stride_h,
                                 void* out, int64_t out_stride_h, int H, int L, int D, int dtype, rtk_stream_t stream) {
    const char* who = "rtk_fp8kv_dequant";
    RTK_CHECK_ARG(codes && scales && out, "%s: NULL pointer", who);
    RTK_CHECK_ARG(H >= 1 && H <= 65535 && L >= 1, "%s: bad shape", who);
    if ((dtype != RTK_BF16 && dtype != RTK_F16) || D != ARC_D) {
        set_error("%s: unsupported dtype code %d / head_dim %d (RTK_BF16 or RTK_F16 with head_dim 128)", who, dtype, D);
        return RTK_EUNSUPPORTED;
    }
    if (codes_stride_h < 0 || scale_stride_h < 0 || out_stride_h < 0 || codes_stride_h % 16 != 0 || (out_stride_h * 2) % 16 != 0 ||
        (((uintptr_t)codes | (uintptr_t)out) & 15) != 0 || ((uintptr_t)scales & 3) != 0) {
        set_error("%s: unsupported layout (16-byte aligned row pointers and head strides)", who);
        return RTK_EUNSUPPORTED;
    }
    const dim3 grid((unsigned)(((int64_t)L * 8 + 255) / 256), (unsigned)H);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RTK_BF16)
        hipLaunchKernelGGL((fp8kv_dequant_kernel<RTK_BF16>), grid, dim3(256), 0, st, (const char*)codes, codes_stride_h, scales,
                           scale_stride_h, (char*)out, out_stride_h, L);
    else
        hipLaunchKernelGGL((fp8kv_dequant_kernel<RTK_F16>), grid, dim3(256), 0, st, (const char*)codes, codes_stride_h, scales,
                           scale_stride_h, (char*)out, out_stride_h, L);
    RTK_LAUNCH_CHECK("fp8kv_dequant_kernel");
    return RTK_OK;
}

// pivotkv_pages.hip - the page index of the page-sparse decode (retake_hip.h §U "Page-sparse decode"; NOT in the reference,
// a rule of this project's own):
//   page_summary_kernel   per arming: kmax / kmin [Hkv, pages, 2, D] of the stored keys of every layer of a device, one call
//   page_summary_fp8k_kernel   the same over the e4m3 key rows of an fp8 archive (codes + scales), see at the kernel
//   page_bound_kernel     per decode call: ub[g, p], an upper bound on every raw logit of kv head g's packed rows against
//                         every key of page p
// A page is RTK_PAGE_ROWS = 32 region rows: one wave tile of the packed decode kernel.  Host side: the two summary entry
// points are summary_call with their units, kernel, the checks on their own K operand and their device unit's fill.
//
// page_summary_kernel - streaming, reads K once.  One wave per (kv head, page); a row of D = 128 16-bit elements is 256
// bytes = 16 lanes x 16 bytes, so a wave's load instruction takes FOUR whole rows (lane: chunk c = lane & 15 of row
// 4 u + (lane >> 4), u = 0 .. 7) - every lane carries data and each row is one contiguous 256-byte run.  A lane folds its 8
// rows element-wise, the four row groups are folded through the lanes 16 and 32 apart, and the lanes of group 0 / 1 store
// the 256 bytes of kmax / kmin.  Max and min are taken on the order-preserving 16-bit key of the sign-magnitude encoding
// (bf16 and fp16 alike: one kernel), so the result is one of the inputs, bit for bit; of -0 and +0 the max is +0 and the min
// -0.  Rows >= n of the partial last page are not loaded.  No LDS, no atomics, no scratch.
// Roofline: HBM, n x 256 bytes read + pages x 512 written per kv head.
//
// page_bound_kernel - a wave takes 4 pages, lane (page lane >> 4, chunk c): it holds 8 elements of kmax and of kmin in fp32
// and, per packed row r = (hh, i), adds its 8 terms max(q kmax, q kmin) in channel order, folds the 16 chunks through the
// lanes 1, 2, 4, 8 apart and keeps the running max over r in the order r = 0, 1, ...  Both operands are 16-bit, so each
// product is exact in fp32; the order of the additions is a function of the shape alone, and so are the bits.
#include <algorithm>

#include "fp8kv.cuh"

namespace rtk {
namespace {

constexpr int PG_ROWS = RTK_PAGE_ROWS;
constexpr int PG_BLOCK = 256;
constexpr int PG_WAVES = PG_BLOCK / WAVE;

struct PageDev {
    const char* k;        // row 0 of kv head 0
    char* summ;           // [Hkv, pages, 2, 128] 16-bit
    int64_t k_sh, s_sh;   // head strides, bytes
    int32_t first, n;
};
struct PageUnits {
    PageDev u[RTK_PAGE_SUMMARY_MAX_UNITS];
};
static_assert(sizeof(PageUnits) <= 4096, "the units travel as a kernel argument");

// order-preserving key of a sign-magnitude 16-bit float and back
__device__ __forceinline__ uint32_t ord16(uint32_t x) { return x ^ ((x & 0x8000u) ? 0xffffu : 0x8000u); }
__device__ __forceinline__ uint32_t unord16(uint32_t y) { return y ^ ((y & 0x8000u) ? 0x8000u : 0xffffu); }

__global__ __launch_bounds__(PG_BLOCK) void page_summary_kernel(PageUnits units) {
    const PageDev& un = units.u[blockIdx.z];
    const int lane = threadIdx.x & (WAVE - 1), wave = uniform_int(threadIdx.x / WAVE);
    const int c = lane & 15, g = lane >> 4;
    const int n = un.n, pages = (n + PG_ROWS - 1) / PG_ROWS;
    const int p = blockIdx.x * PG_WAVES + wave, h = blockIdx.y;
    if (p >= pages) return;   // (wave-uniform: the grid is sized for the launch's largest unit)
    const char* kp = un.k + (int64_t)h * un.k_sh + ((int64_t)un.first + (int64_t)PG_ROWS * p) * 256 + 16 * c;
    const int rows = min(PG_ROWS, n - PG_ROWS * p);   // of this page: >= 1
    uint32_t hi[8], lo[8];   // keys of the lane's 8 elements: running max, running min
#pragma unroll
    for (int e = 0; e < 8; ++e) hi[e] = 0u, lo[e] = 0xffffu;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int r = 4 * u + g;
        if (r < rows) {
            const u32x4 t = __builtin_nontemporal_load((const u32x4*)(kp + (int64_t)r * 256));
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t a = ord16(t[w] & 0xffffu), b = ord16(t[w] >> 16);
                hi[2 * w] = max(hi[2 * w], a), lo[2 * w] = min(lo[2 * w], a);
                hi[2 * w + 1] = max(hi[2 * w + 1], b), lo[2 * w + 1] = min(lo[2 * w + 1], b);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = max(hi[e], (uint32_t)__shfl_xor((int)hi[e], 16, WAVE));
        hi[e] = max(hi[e], (uint32_t)__shfl_xor((int)hi[e], 32, WAVE));
        lo[e] = min(lo[e], (uint32_t)__shfl_xor((int)lo[e], 16, WAVE));
        lo[e] = min(lo[e], (uint32_t)__shfl_xor((int)lo[e], 32, WAVE));
    }
    if (g < 2) {   // group 0 stores kmax, group 1 kmin: 16 lanes x 16 bytes each
        u32x4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            o[w] = g == 0 ? (unord16(hi[2 * w]) | (unord16(hi[2 * w + 1]) << 16)) : (unord16(lo[2 * w]) | (unord16(lo[2 * w + 1]) << 16));
        *(u32x4*)(un.summ + (int64_t)h * un.s_sh + (int64_t)p * 512 + 256 * g + 16 * c) = o;
    }
}

// page_summary_fp8k_kernel - the same summaries over the e4m3 key rows of an fp8 archive: K[g, j, d] =
// dtype(float(code) * scale), fp8kv.cuh's one dequantisation, so the summaries are 16-bit values of the keys the attention
// really uses.  One wave per (kv head, page); a code row is 128 bytes = 8 lanes x 16 bytes, so a wave's load instruction
// takes EIGHT whole rows (lane: codes 16 c .. 16 c + 15, c = lane & 7, of row 8 u + (lane >> 3), u = 0 .. 3) and the row's
// scale is loaded once per row.  A lane folds its 4 rows element-wise on the ordered 16-bit keys, the eight row groups are
// folded through the lanes 8, 16 and 32 apart, and the lanes of row group 0 / 1 store the 256 bytes of kmax / kmin, 32 each.
// Rows >= n are not loaded, neither codes nor scales.  No LDS, no atomics, no scratch.
// Roofline: HBM, n x 132 bytes read + pages x 512 written per kv head.
struct PageDev8 {
    const char* k8;        // codes of row 0 of kv head 0
    const float* ks;       // scales of row 0 of kv head 0
    char* summ;            // [Hkv, pages, 2, 128] 16-bit
    int64_t k8_sh, s_sh;   // head strides, bytes
    int64_t ks_sh;         // head stride, floats
    int32_t n, pad;
};
struct PageUnits8 {
    PageDev8 u[RTK_PAGE_SUMMARY_MAX_UNITS];
};
static_assert(sizeof(PageUnits8) <= 4096, "the units travel as a kernel argument");

template <int DT> __global__ __launch_bounds__(PG_BLOCK) void page_summary_fp8k_kernel(PageUnits8 units) {
    const PageDev8& un = units.u[blockIdx.z];
    const int lane = threadIdx.x & (WAVE - 1), wave = uniform_int(threadIdx.x / WAVE);
    const int c = lane & 7, g = lane >> 3;
    const int n = un.n, pages = (n + PG_ROWS - 1) / PG_ROWS;
    const int p = blockIdx.x * PG_WAVES + wave, h = blockIdx.y;
    if (p >= pages) return;   // (wave-uniform: the grid is sized for the launch's largest unit)
    const char* kp = un.k8 + (int64_t)h * un.k8_sh + (int64_t)PG_ROWS * p * 128 + 16 * c;
    const float* sp = un.ks + (int64_t)h * un.ks_sh + (int64_t)PG_ROWS * p;
    const int rows = min(PG_ROWS, n - PG_ROWS * p);   // of this page: >= 1
    uint32_t hi[16], lo[16];   // keys of the lane's 16 elements: running max, running min
#pragma unroll
    for (int e = 0; e < 16; ++e) hi[e] = 0u, lo[e] = 0xffffu;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = 8 * u + g;
        if (r < rows) {
            const u32x4 codes = __builtin_nontemporal_load((const u32x4*)(kp + (int64_t)r * 128));
            const float scale = __builtin_nontemporal_load(sp + r);
            u32x4 t[2];
            fp8_dequant16<DT>(codes, scale, t[0], t[1]);
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const uint32_t x = t[w >> 2][w & 3];
                const uint32_t a = ord16(x & 0xffffu), b = ord16(x >> 16);
                hi[2 * w] = max(hi[2 * w], a), lo[2 * w] = min(lo[2 * w], a);
                hi[2 * w + 1] = max(hi[2 * w + 1], b), lo[2 * w + 1] = min(lo[2 * w + 1], b);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int d = 8; d < WAVE; d *= 2) {
            hi[e] = max(hi[e], (uint32_t)__shfl_xor((int)hi[e], d, WAVE));
            lo[e] = min(lo[e], (uint32_t)__shfl_xor((int)lo[e], d, WAVE));
        }
    }
    if (g < 2) {   // row group 0 stores kmax, group 1 kmin: 8 lanes x 32 bytes each
        u32x4 o[2];
#pragma unroll
        for (int w = 0; w < 8; ++w)
            o[w >> 2][w & 3] = g == 0 ? (unord16(hi[2 * w]) | (unord16(hi[2 * w + 1]) << 16))
                                      : (unord16(lo[2 * w]) | (unord16(lo[2 * w + 1]) << 16));
        char* out = un.summ + (int64_t)h * un.s_sh + (int64_t)p * 512 + 256 * g + 32 * c;
        *(u32x4*)out = o[0];
        *(u32x4*)(out + 16) = o[1];
    }
}

template <int DT> __device__ __forceinline__ void unpack8(const u32x4& t, float (&f)[8]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        f[2 * w] = H16<DT>::lo(t[w]);
        f[2 * w + 1] = H16<DT>::hi(t[w]);
    }
}

template <int DT>
__global__ __launch_bounds__(PG_BLOCK) void page_bound_kernel(const char* __restrict__ q, int64_t q_sh, int64_t q_sl,
                                                              const char* __restrict__ summ, int64_t s_sh, int G, int Lq,
                                                              int pages, float* __restrict__ ub) {
    const int lane = threadIdx.x & (WAVE - 1), wave = uniform_int(threadIdx.x / WAVE);
    const int c = lane & 15, j = lane >> 4;
    const int hkv = blockIdx.y;
    const int p = (blockIdx.x * PG_WAVES + wave) * 4 + j;
    const int pc = min(p, pages - 1);   // a page past the end re-reads the last one and stores nothing
    const char* sp = summ + ((int64_t)hkv * s_sh) * 2 + (int64_t)pc * 512 + 16 * c;
    float kx[8], kn[8];
    unpack8<DT>(*(const u32x4*)sp, kx);
    unpack8<DT>(*(const u32x4*)(sp + 256), kn);
    float best = -INFINITY;
    for (int hh = 0; hh < G; ++hh)
        for (int i = 0; i < Lq; ++i) {
            float qv[8];
            unpack8<DT>(*(const u32x4*)(q + ((int64_t)(hkv * G + hh) * q_sh + (int64_t)i * q_sl) * 2 + 16 * c), qv);
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = acc + fmaxf(qv[e] * kx[e], qv[e] * kn[e]);
            acc = acc + __shfl_xor(acc, 1, WAVE);
            acc = acc + __shfl_xor(acc, 2, WAVE);
            acc = acc + __shfl_xor(acc, 4, WAVE);
            acc = acc + __shfl_xor(acc, 8, WAVE);
            best = fmaxf(best, acc);
        }
    if (c == 0 && p < pages) ub[(int64_t)hkv * pages + p] = best;
}

int pages_check_envelope(const char* who, int D, int dtype) {
    if (dtype != RTK_BF16 && dtype != RTK_F16) {
        set_error("%s: unsupported dtype code %d (RTK_BF16 or RTK_F16)", who, dtype);
        return RTK_EUNSUPPORTED;
    }
    if (D != 128) {
        set_error("%s: unsupported head_dim %d (128)", who, D);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

// What the two summary calls share (`Units` / `kern`: the kind's device units and kernel): the call's checks; per unit
// `check_k` - the checks on its own K operand, the first of them on its row counts - and, with rows, the checks on summ;
// then launch_units with `fill`, every launch's grid sized for its largest unit.
template <class Units, class Unit, class CheckK, class Fill>
int summary_call(const char* who, void (*kern)(Units), const char* kern_name, const Unit* units, int n_units, int Hkv, int D, int dtype,
                 rtk_stream_t stream, CheckK&& check_k, Fill&& fill) {
    int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    RTK_CHECK_ARG(Hkv >= 1 && Hkv <= 65535, "%s: Hkv %d", who, Hkv);
    rc = pages_check_envelope(who, D, dtype);
    if (rc != RTK_OK) return rc;
    for (int i = 0; i < n_units; ++i) {
        const Unit& u = units[i];
        rc = check_k(u, i);
        if (rc != RTK_OK) return rc;
        if (u.n == 0) continue;
        const int64_t pages = (u.n + PG_ROWS - 1) / PG_ROWS;
        RTK_CHECK_ARG(u.summ, "%s: unit %d: NULL summ", who, i);
        RTK_CHECK_ARG(((uintptr_t)u.summ & 15) == 0 && (u.summ_stride_h * 2) % 16 == 0,
                      "%s: unit %d: summ / summ_stride_h not 16-byte aligned", who, i);
        RTK_CHECK_ARG(u.summ_stride_h >= 0 && (Hkv == 1 || u.summ_stride_h >= pages * 2 * D),
                      "%s: unit %d: summ_stride_h %lld is smaller than pages * 2 * D = %lld", who, i, (long long)u.summ_stride_h,
                      (long long)(pages * 2 * D));
    }
    unsigned grid_x = 0;   // of the launch being filled: its largest unit's
    return launch_units<Units>(
        n_units,
        [&](int i, auto& dv) {
            const Unit& u = units[i];
            if (u.n == 0) return false;
            dv = fill(u);
            const unsigned pages = (unsigned)((u.n + PG_ROWS - 1) / PG_ROWS);
            grid_x = std::max(grid_x, (pages + PG_WAVES - 1) / PG_WAVES);
            return true;
        },
        [&](const Units& pu, int n) -> int {
            hipLaunchKernelGGL(kern, dim3(grid_x, (unsigned)Hkv, (unsigned)n), dim3(PG_BLOCK), 0, (hipStream_t)stream, pu);
            RTK_LAUNCH_CHECK(kern_name);
            grid_x = 0;
            return RTK_OK;
        });
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_page_summary_batched(const rtk_page_summary_unit* units, int n_units, int Hkv, int D, int dtype,
                                                rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_page_summary_batched";
    return summary_call<PageUnits>(
        who, page_summary_kernel, "page_summary_kernel", units, n_units, Hkv, D, dtype, stream,
        [&](const rtk_page_summary_unit& u, int i) -> int {
            RTK_CHECK_ARG(u.first >= 0 && u.n >= 0 && u.first + u.n <= 0x3fffffff, "%s: unit %d: first %lld / n %lld", who, i,
                          (long long)u.first, (long long)u.n);
            if (u.n == 0) return RTK_OK;
            RTK_CHECK_ARG(u.k, "%s: unit %d: NULL k", who, i);
            RTK_CHECK_ARG(((uintptr_t)u.k & 15) == 0 && (u.k_stride_h * 2) % 16 == 0, "%s: unit %d: k / k_stride_h not 16-byte aligned",
                          who, i);
            RTK_CHECK_ARG(u.k_stride_h >= 0 && (Hkv == 1 || u.k_stride_h >= (u.first + u.n) * D),
                          "%s: unit %d: k_stride_h %lld is smaller than the rows of a head", who, i, (long long)u.k_stride_h);
            return RTK_OK;
        },
        [](const rtk_page_summary_unit& u) {
            return PageDev{(const char*)u.k, (char*)u.summ, u.k_stride_h * 2, u.summ_stride_h * 2, (int32_t)u.first, (int32_t)u.n};
        });
}

extern "C" int rtk_pivotkv_page_summary_fp8k_batched(const rtk_page_summary_fp8k_unit* units, int n_units, int Hkv, int D,
                                                     int dtype, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_page_summary_fp8k_batched";
    return summary_call<PageUnits8>(
        who, dtype == RTK_BF16 ? page_summary_fp8k_kernel<RTK_BF16> : page_summary_fp8k_kernel<RTK_F16>, "page_summary_fp8k_kernel", units,
        n_units, Hkv, D, dtype, stream,
        [&](const rtk_page_summary_fp8k_unit& u, int i) -> int {
            RTK_CHECK_ARG(u.n >= 0 && u.n <= 0x3fffffff, "%s: unit %d: n %lld", who, i, (long long)u.n);
            if (u.n == 0) return RTK_OK;
            RTK_CHECK_ARG(u.k8 && u.k_scale, "%s: unit %d: NULL k8 / k_scale", who, i);
            // the archive's limit (rtk_attention_decode_fp8kv): the codes of one head stay below 2 GiB
            RTK_CHECK_ARG(u.n * D < (1ll << 31) - PG_ROWS * D, "%s: unit %d: n %lld: the codes of one head span 2 GiB or more", who, i,
                          (long long)u.n);
            RTK_CHECK_ARG(((uintptr_t)u.k8 & 15) == 0 && u.k8_stride_h % 16 == 0 && ((uintptr_t)u.k_scale & 3) == 0,
                          "%s: unit %d: k8 / k8_stride_h not 16-byte aligned, or k_scale not 4-byte aligned", who, i);
            RTK_CHECK_ARG(u.k8_stride_h >= 0 && (Hkv == 1 || u.k8_stride_h >= u.n * D),
                          "%s: unit %d: k8_stride_h %lld is smaller than the rows of a head", who, i, (long long)u.k8_stride_h);
            RTK_CHECK_ARG(u.scale_stride_h >= 0 && (Hkv == 1 || u.scale_stride_h >= u.n),
                          "%s: unit %d: scale_stride_h %lld is smaller than the rows of a head", who, i, (long long)u.scale_stride_h);
            return RTK_OK;
        },
        [](const rtk_page_summary_fp8k_unit& u) {
            return PageDev8{(const char*)u.k8, u.k_scale, (char*)u.summ, u.k8_stride_h, u.summ_stride_h * 2, u.scale_stride_h, (int32_t)u.n, 0};
        });
}

extern "C" int rtk_attention_page_bound(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* summ,
                                        int64_t summ_stride_h, int Hq, int Hkv, int Lq, int pages, int D, int dtype, float* ub,
                                        rtk_stream_t stream) {
    const char* who = "rtk_attention_page_bound";
    RTK_CHECK_ARG(q && summ && ub, "%s: NULL q / summ / ub pointer", who);
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Lq >= 1 && pages >= 1, "%s: Hq, Hkv, Lq and pages must be positive", who);
    RTK_CHECK_ARG(Hq % Hkv == 0, "%s: Hq %d is not a multiple of Hkv %d", who, Hq, Hkv);
    RTK_CHECK_ARG(Hkv <= 65535 && pages <= 0x3fffffff / 512, "%s: Hkv %d / pages %d too large", who, Hkv, pages);
    const int rc = pages_check_envelope(who, D, dtype);
    if (rc != RTK_OK) return rc;
    RTK_CHECK_ARG((((uintptr_t)q | (uintptr_t)summ) & 15) == 0 && ((uintptr_t)ub & 3) == 0 && (q_stride_h * 2) % 16 == 0 &&
                      (q_stride_l * 2) % 16 == 0 && (summ_stride_h * 2) % 16 == 0,
                  "%s: q / summ and their strides must be multiples of 16 bytes, ub of 4", who);
    RTK_CHECK_ARG(q_stride_h >= 0 && q_stride_l >= D && (Hkv == 1 || summ_stride_h >= (int64_t)pages * 2 * D),
                  "%s: q_stride_l below head_dim, a negative stride, or summ_stride_h below pages * 2 * D", who);
    const dim3 grid((unsigned)((pages + 4 * PG_WAVES - 1) / (4 * PG_WAVES)), (unsigned)Hkv);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RTK_BF16)
        hipLaunchKernelGGL((page_bound_kernel<RTK_BF16>), grid, dim3(PG_BLOCK), 0, st, (const char*)q, q_stride_h, q_stride_l,
                           (const char*)summ, summ_stride_h, Hq / Hkv, Lq, pages, ub);
    else
        hipLaunchKernelGGL((page_bound_kernel<RTK_F16>), grid, dim3(PG_BLOCK), 0, st, (const char*)q, q_stride_h, q_stride_l,
                           (const char*)summ, summ_stride_h, Hq / Hkv, Lq, pages, ub);
    RTK_LAUNCH_CHECK("page_bound_kernel");
    return RTK_OK;
}

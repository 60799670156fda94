// pivotkv_rebase.hip - re-base the position ids of a bounded video region and re-rotate its keys, in place, for many layers
// in one call (retake_hip.h "Position re-base"; a rule of this project's own, the reference has no counterpart).
//
// Per unit (a layer): t = row 0 of its ids, the region's ids are t[first, end).
//     base  = first > 0 ? t[first - 1] + 1 : 0
//     delta = t[first] - base
//     if delta > 0 and t[end - 1] >= limit:   t[first, end) -= delta;  K[:, first .. first + rows) <- R(-delta) K on the
//                                             temporal channel pairs;  offsets[slot] += delta
// R(a + b) = R(a) R(b): a key rotated at id p and rotated again by -delta is the key rotated at p - delta.
//
// Two launches and no order between workgroups - no flags, no counters, no waiting.  The ids the decision reads are ids
// the call rewrites, so the decision is its own tiny launch: one wave per unit reads three ids and writes delta (0: not
// triggered) into a scratch word per unit; the apply launch decides from that word alone and reads no id in order to
// decide.  Nothing is read back: the host learns neither delta nor whether a unit triggered.
//
// Apply, roofline HBM (one read and one write of the touched bytes): a thread owns ONE 16-byte chunk at channel d and its
// rotation partner at d + D/2, computes the cos / sin of its 8 (fp32: 4) channels once - delta is uniform over a unit -
// and walks rows and heads with them.  A chunk pair without a temporal channel (M-RoPE: the h / w sections) is neither
// loaded nor stored; channels of other id rows inside a loaded pair keep their bits.  A unit with delta == 0 exits at once.
// The grid is sized to the machine (REBASE_WGS workgroups over the launch's units), not to the rows.
#include <algorithm>

#include "common.cuh"

namespace rtk {
namespace {

constexpr int REBASE_BLOCK = 256;
constexpr int REBASE_WGS = 2048;   // workgroups of a full launch: 256 CUs x 8 resident workgroups of 4 waves
constexpr int REBASE_HB = 4;       // heads whose chunk pairs a thread requests together

struct RebaseDev {
    char* k;              // first byte of row `first` of head 0
    int64_t stride_h;     // bytes between heads
    int64_t* t;           // &ids[0][first]
    int64_t n_ids;        // end - first
    int64_t rows;         // K rows of the region
    int32_t H;
    int32_t slot;         // bit 31: first > 0 (t[-1] is the last pinned id)
};
struct RebaseUnits {
    RebaseDev u[RTK_REBASE_MAX_UNITS];
};
constexpr uint32_t REBASE_HAS_PREV = 0x80000000u;

// one wave per unit; lane 0 decides.  delta[unit] is written for every unit of the launch
__global__ __launch_bounds__(WAVE) void rebase_decide_kernel(RebaseUnits units, int64_t limit, int64_t* __restrict__ delta,
                                                             int64_t* __restrict__ offsets) {
    if (threadIdx.x != 0) return;
    const RebaseDev& un = units.u[blockIdx.x];
    long long d = 0;
    if (un.n_ids > 0) {
        const long long base = ((uint32_t)un.slot & REBASE_HAS_PREV) ? (long long)un.t[-1] + 1 : 0ll;
        const long long dl = (long long)un.t[0] - base;
        if (dl > 0 && (long long)un.t[un.n_ids - 1] >= (long long)limit) d = dl;
    }
    delta[blockIdx.x] = d;
    if (d != 0) offsets[(uint32_t)un.slot & ~REBASE_HAS_PREV] += d;   // (slots of one call are distinct: checked on the host)
}

template <int DT>
__global__ __launch_bounds__(REBASE_BLOCK) void rebase_apply_kernel(RebaseUnits units, int D, const float* __restrict__ inv_freq,
                                                                   RowSel rs, const int64_t* __restrict__ delta) {
    using V = Vec16<DT>;
    constexpr int VE = V::VE;
    constexpr int ES = 16 / VE;
    const long long dl = (long long)delta[blockIdx.y];
    if (dl == 0) return;   // (uniform)
    const RebaseDev& un = units.u[blockIdx.y];
    // the ids: t[first, end) -= delta
    for (int64_t i = (int64_t)blockIdx.x * REBASE_BLOCK + threadIdx.x; i < un.n_ids; i += (int64_t)gridDim.x * REBASE_BLOCK)
        un.t[i] -= dl;
    // the keys: chunk pair cp of the rows r0, r0 + stride, ...
    const int h2 = D / 2, lpr = h2 / VE, rpb = REBASE_BLOCK / lpr;
    const int r0 = (int)threadIdx.x / lpr, cp = (int)threadIdx.x - r0 * lpr;
    if (r0 >= rpb) return;
    const int d = cp * VE;
    uint32_t temporal = 0;   // bit e: channel pair (d + e, d + e + h2) follows id row 0
#pragma unroll
    for (int e = 0; e < VE; ++e) temporal |= (rs.row[d + e] == 0 ? 1u : 0u) << e;
    if (temporal == 0) return;
    float c[VE], s[VE];
    const float fd = (float)dl;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        sincos_cr(fd * inv_freq[d + e], s[e], c[e]);
        if (!((temporal >> e) & 1u)) {
            c[e] = 1.f;
            s[e] = 0.f;
        }
    }
    // which 32-bit words of a chunk take the rotated bits (a chunk that mixes id rows keeps the others' bits as they are)
    uint32_t take[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if constexpr (DT != RTK_F32)
            take[w] = (((temporal >> (2 * w)) & 1u) ? 0x0000ffffu : 0u) | (((temporal >> (2 * w + 1)) & 1u) ? 0xffff0000u : 0u);
        else
            take[w] = ((temporal >> w) & 1u) ? 0xffffffffu : 0u;
    }
    const int H = un.H;
    const int64_t row_bytes = (int64_t)D * ES;
    for (int64_t r = (int64_t)blockIdx.x * rpb + r0; r < un.rows; r += (int64_t)gridDim.x * rpb) {
        char* row0 = un.k + r * row_bytes + (int64_t)d * ES;
        for (int hb = 0; hb < H; hb += REBASE_HB) {
            u32x4 lo[REBASE_HB], hi[REBASE_HB];
#pragma unroll
            for (int u = 0; u < REBASE_HB; ++u) {   // (a short last batch repeats its last head: loaded, not stored)
                const char* p = row0 + (int64_t)min(hb + u, H - 1) * un.stride_h;
                lo[u] = *(const u32x4*)p;
                hi[u] = *(const u32x4*)(p + (int64_t)h2 * ES);
            }
#pragma unroll
            for (int u = 0; u < REBASE_HB; ++u) {
                if (hb + u >= H) break;
                float x1[VE], x2[VE], o1[VE], o2[VE];
                V::unpack(lo[u], x1);
                V::unpack(hi[u], x2);
#pragma unroll
                for (int e = 0; e < VE; ++e) {   // R(-delta): fp32, one rounding to the storage dtype in pack()
                    o1[e] = __builtin_fmaf(x1[e], c[e], __fmul_rn(x2[e], s[e]));
                    o2[e] = __builtin_fmaf(x2[e], c[e], -__fmul_rn(x1[e], s[e]));
                }
                u32x4 nlo = V::pack(o1), nhi = V::pack(o2);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    nlo[w] = (nlo[w] & take[w]) | (lo[u][w] & ~take[w]);
                    nhi[w] = (nhi[w] & take[w]) | (hi[u][w] & ~take[w]);
                }
                char* p = row0 + (int64_t)(hb + u) * un.stride_h;
                *(u32x4*)p = nlo;
                *(u32x4*)(p + (int64_t)h2 * ES) = nhi;
            }
        }
    }
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_rebase_batched(const rtk_rebase_unit* units, int n_units, int D, int dtype, int P,
                                          const float* inv_freq, const int* sections_host, int nsec, int64_t limit,
                                          int64_t* offsets, int64_t* delta, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_rebase_batched";
    int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    RTK_CHECK_ARG(inv_freq && offsets && delta, "%s: NULL pointer (inv_freq / offsets / delta)", who);
    RTK_CHECK_ARG(limit >= 0, "%s: negative limit %lld", who, (long long)limit);
    int es, ve;
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "%s: unsupported dtype %d", who, dtype);
    RTK_CHECK_ARG(D >= 2, "%s: head_dim %d", who, D);
    RTK_CHECK_ARG(P == 1 || P == 3, "%s: P must be 1 or 3, got %d", who, P);
    for (int i = 0; i < n_units; ++i) {
        const rtk_rebase_unit& u = units[i];
        RTK_CHECK_ARG(u.k && u.ids, "%s: unit %d: NULL pointer", who, i);
        RTK_CHECK_ARG(u.H >= 1 && u.first >= 0 && u.rows >= 0 && u.end >= 0 && u.k_stride_h >= 0 && u.ids_stride >= 0 && u.slot >= 0,
                      "%s: unit %d: negative H / first / rows / end / stride / slot", who, i);
        RTK_CHECK_ARG(u.first <= u.end, "%s: unit %d: first %lld > end %lld", who, i, (long long)u.first, (long long)u.end);
        RTK_CHECK_ARG(u.first <= (INT64_MAX >> 12) - u.rows, "%s: unit %d: first + rows overflows a byte offset", who, i);
        RTK_CHECK_ARG(u.H == 1 || u.k_stride_h >= (u.first + u.rows) * (int64_t)D * es,
                      "%s: unit %d: the rows [0, %lld) of a head reach into the next head", who, i, (long long)(u.first + u.rows));
        RTK_CHECK_ARG(P == 1 || u.ids_stride >= u.end, "%s: unit %d: ids_stride %lld < end %lld", who, i, (long long)u.ids_stride,
                      (long long)u.end);
        for (int j = 0; j < i; ++j)
            RTK_CHECK_ARG(units[j].slot != u.slot, "%s: units %d and %d share offset slot %d", who, j, i, u.slot);
    }
    bool aligned = D % (2 * ve) == 0 && D <= 256;
    for (int i = 0; i < n_units; ++i)
        aligned = aligned && ((uintptr_t)units[i].k & 15) == 0 && units[i].k_stride_h % 16 == 0 && ((uintptr_t)units[i].ids & 7) == 0;
    if (!aligned) {
        set_error("%s: needs 16-byte aligned rows and head strides and head_dim a multiple of %d (<= 256)", who, 2 * ve);
        return RTK_EUNSUPPORTED;
    }
    RowSel rs;
    if ((rc = make_rowsel(rs, P, D, sections_host, nsec, who)) != RTK_OK) return rc;
    for (int d = 0; d < D / 2; ++d)
        if ((rs.row[d] == 0) != (rs.row[d + D / 2] == 0)) {
            set_error("%s: channel %d and its rotation partner follow different id rows", who, d);
            return RTK_EUNSUPPORTED;
        }
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_units; b += RTK_REBASE_MAX_UNITS) {
        const int n = std::min(n_units - b, RTK_REBASE_MAX_UNITS);
        RebaseUnits ru;
        int64_t most = 1;
        for (int j = 0; j < RTK_REBASE_MAX_UNITS; ++j) {
            const rtk_rebase_unit& u = units[b + std::min(j, n - 1)];   // (slots past n repeat the last unit and are never read)
            RebaseDev& dv = ru.u[j];
            dv.k = (char*)u.k + u.first * (int64_t)D * es;
            dv.stride_h = u.k_stride_h;
            dv.t = u.ids + u.first;
            dv.n_ids = u.end - u.first;
            dv.rows = u.rows;
            dv.H = u.H;
            dv.slot = (int32_t)((uint32_t)u.slot | (u.first > 0 ? REBASE_HAS_PREV : 0u));
            most = std::max(most, std::max(u.rows, (dv.n_ids + REBASE_BLOCK - 1) / REBASE_BLOCK));
        }
        RTK_LAUNCH(KID_REBASE_DECIDE, rebase_decide_kernel, dim3(n), dim3(WAVE), 0, st, ru, limit, delta + b, offsets);
        RTK_LAUNCH_CHECK("rebase_decide_kernel");
        // workgroups per unit: the machine's share, and no more than the largest unit has steps for
        const int rpb = REBASE_BLOCK / (D / 2 / ve);
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((REBASE_WGS + n - 1) / n, (most + rpb - 1) / rpb));
        const int64_t* dl = delta + b;
        with_payload(dtype, [&](auto dt) {
            RTK_LAUNCH(KID_REBASE, rebase_apply_kernel<decltype(dt)::value>, dim3(gx, n), dim3(REBASE_BLOCK), 0, st, ru, D, inv_freq, rs, dl);
            return 0;
        });
        RTK_LAUNCH_CHECK("rebase_apply_kernel");
    }
    return RTK_OK;
}

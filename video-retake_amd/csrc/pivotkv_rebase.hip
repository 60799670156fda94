// pivotkv_rebase.hip - re-base (one delta per unit) or renumber (one delta per row) the position ids of a bounded video region
// and re-rotate its keys, in place, for many layers in one call (retake_hip.h "Position re-base", §R "Position renumbering";
// rules of this project's own, the reference has no counterpart).
//
// Per unit (a layer): t = row 0 of its ids, the region's ids are t[first, end), prev = first > 0 ? t[first - 1] : -1.
//   re-base:   delta = t[first] - prev - 1
//              if delta > 0 and t[end - 1] >= limit:   t[first, end) -= delta;  K[:, first .. first + rows) <- R(-delta) K on the
//                                                      temporal channel pairs;  offsets[slot] += delta
//   renumber:  e[first] = max(0, t[first] - prev - 1)         the region follows the pinned rows (the re-base's delta)
//              e[i]     = max(0, t[i] - t[i - 1] - gap)       inner gaps above `gap` close to `gap`; gaps <= gap stay
//              d[i]     = e[first] + ... + e[i],   total = d[end - 1]
//              if total > 0 and t[end - 1] >= limit:   t[i] -= d[i];  K row r <- R(-d[first + r]) K row r on the temporal
//                                                      channel pairs;  offsets[slot] += total
// R(a + b) = R(a) R(b): a key rotated at id p and rotated again by -delta is the key rotated at p - delta.
//
// Two launches and no order between workgroups - no flags, no counters, no waiting.  The ids the decision reads are ids the
// call rewrites, so the first launch only READS ids and leaves delta[unit] (0: not triggered) in a scratch word per unit, and
// the apply launch decides from that word alone.  Nothing is read back: the host learns neither delta nor whether a unit
// triggered.  The re-base's first launch is tiny: one wave per unit reads three ids.  The renumbering's is a scan, one
// workgroup per unit: it walks [first, end) in tiles of RTK_RENUMBER_TILE ids - a wave-level inclusive scan, the waves' sums
// through LDS, a running int64 carry - and writes d into the unit's row_delta scratch; a unit whose last id is below the limit
// is not scanned at all.
//
// Apply, roofline HBM (one read and one write of the touched bytes): a thread owns ONE 16-byte chunk at channel d and its
// rotation partner at d + D/2 and walks rows and heads (in batches) with it.  A chunk pair without a temporal channel (M-RoPE:
// the h / w sections) is neither loaded nor stored; channels of other id rows inside a loaded pair keep their bits.  A unit
// with delta == 0 exits at once.  The grid is sized to the machine (REBASE_WGS workgroups over the launch's units), not to the
// rows.  The re-base computes the cos / sin of its 8 (fp32: 4) channels once - delta is uniform over a unit - and strides
// rows across the grid.  In the renumbering they are a function of the row: a workgroup owns a CONTIGUOUS block of rows, a
// thread walks ADJACENT rows of it and keeps its cos / sin while the next row has the same delta - the rows of one id share
// them, and a region with few holes pays the fp64 sin / cos rarely (measured against rows 256 / lanes apart per thread, which
// keeps a wave's requests contiguous: 1 - 2 % slower in every pattern); a row with d = 0 is neither loaded nor
// stored.
#include <algorithm>
#include <type_traits>

#include "common.cuh"

namespace rtk {
namespace {

constexpr int REBASE_BLOCK = 256;
constexpr int REBASE_WGS = 2048;   // workgroups of a full launch: 256 CUs x 8 resident workgroups of 4 waves
constexpr int REBASE_HB = 4;       // heads whose chunk pairs a thread requests together
constexpr int RENUMBER_ITEMS = RTK_RENUMBER_TILE / REBASE_BLOCK;   // consecutive ids of a thread in a tile
static_assert(RENUMBER_ITEMS * REBASE_BLOCK == RTK_RENUMBER_TILE, "a tile is a whole number of ids per thread");

struct RebaseDev {
    char* k;              // first byte of row `first` of head 0
    int64_t stride_h;     // bytes between heads
    int64_t* t;           // &ids[0][first]
    int64_t n_ids;        // end - first
    int64_t rows;         // K rows of the region (renumbering: <= n_ids)
    int64_t* row_delta;   // renumbering: [n_ids] scratch, d of every region id; re-base: NULL
    int32_t H;
    int32_t slot;         // bit 31: first > 0 (t[-1] is the last pinned id)
};
struct RebaseUnits {
    RebaseDev u[RTK_REBASE_MAX_UNITS];
};
constexpr uint32_t REBASE_HAS_PREV = 0x80000000u;

// bit e: channel pair (d + e, d + e + D/2) follows id row 0
template <int VE>
__device__ __forceinline__ uint32_t rebase_temporal(const RowSel& rs, int d) {
    uint32_t temporal = 0;
#pragma unroll
    for (int e = 0; e < VE; ++e) temporal |= (rs.row[d + e] == 0 ? 1u : 0u) << e;
    return temporal;
}

// cos / sin of fl32(fd * inv_freq[d + e]); the identity where the pair is not temporal
template <int VE>
__device__ __forceinline__ void rebase_sincos(float fd, const float* __restrict__ inv_freq, int d, uint32_t temporal, float (&c)[VE],
                                              float (&s)[VE]) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        sincos_cr(fd * inv_freq[d + e], s[e], c[e]);
        if (!((temporal >> e) & 1u)) {
            c[e] = 1.f;
            s[e] = 0.f;
        }
    }
}

// which 32-bit words of a chunk take the rotated bits (a chunk that mixes id rows keeps the others' bits as they are)
template <int DT>
__device__ __forceinline__ void rebase_take(uint32_t temporal, uint32_t (&take)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if constexpr (DT != RTK_F32)
            take[w] = (((temporal >> (2 * w)) & 1u) ? 0x0000ffffu : 0u) | (((temporal >> (2 * w + 1)) & 1u) ? 0xffff0000u : 0u);
        else
            take[w] = ((temporal >> w) & 1u) ? 0xffffffffu : 0u;
    }
}

// one row: the chunk at row0 and its partner `half_bytes` further on, of H heads `stride_h` bytes apart, in batches of
// REBASE_HB heads - R(-delta) in fp32, one rounding to the storage dtype in pack()
template <int DT>
__device__ __forceinline__ void rebase_rotate_row(char* row0, int H, int64_t stride_h, int64_t half_bytes,
                                                  const float (&c)[Vec16<DT>::VE], const float (&s)[Vec16<DT>::VE],
                                                  const uint32_t (&take)[4]) {
    using V = Vec16<DT>;
    constexpr int VE = V::VE;
    for (int hb = 0; hb < H; hb += REBASE_HB) {
        u32x4 lo[REBASE_HB], hi[REBASE_HB];
#pragma unroll
        for (int u = 0; u < REBASE_HB; ++u) {   // (a short last batch repeats its last head: loaded, not stored)
            const char* p = row0 + (int64_t)min(hb + u, H - 1) * stride_h;
            lo[u] = *(const u32x4*)p;
            hi[u] = *(const u32x4*)(p + half_bytes);
        }
#pragma unroll
        for (int u = 0; u < REBASE_HB; ++u) {
            if (hb + u >= H) break;
            float x1[VE], x2[VE], o1[VE], o2[VE];
            V::unpack(lo[u], x1);
            V::unpack(hi[u], x2);
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                o1[e] = __builtin_fmaf(x1[e], c[e], __fmul_rn(x2[e], s[e]));
                o2[e] = __builtin_fmaf(x2[e], c[e], -__fmul_rn(x1[e], s[e]));
            }
            u32x4 nlo = V::pack(o1), nhi = V::pack(o2);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                nlo[w] = (nlo[w] & take[w]) | (lo[u][w] & ~take[w]);
                nhi[w] = (nhi[w] & take[w]) | (hi[u][w] & ~take[w]);
            }
            char* p = row0 + (int64_t)(hb + u) * stride_h;
            *(u32x4*)p = nlo;
            *(u32x4*)(p + half_bytes) = nhi;
        }
    }
}

// re-base: one wave per unit; lane 0 decides.  delta[unit] is written for every unit of the launch
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
    const uint32_t temporal = rebase_temporal<VE>(rs, d);
    if (temporal == 0) return;
    float c[VE], s[VE];
    rebase_sincos<VE>((float)dl, inv_freq, d, temporal, c, s);
    uint32_t take[4];
    rebase_take<DT>(temporal, take);
    const int64_t row_bytes = (int64_t)D * ES;
    for (int64_t r = (int64_t)blockIdx.x * rpb + r0; r < un.rows; r += (int64_t)gridDim.x * rpb)
        rebase_rotate_row<DT>(un.k + r * row_bytes + (int64_t)d * ES, un.H, un.stride_h, (int64_t)h2 * ES, c, s, take);
}

// renumbering: one workgroup per unit.  delta[unit] is written for every unit of the launch; row_delta for every region id of
// a unit whose last id has reached the limit
__global__ __launch_bounds__(REBASE_BLOCK) void renumber_scan_kernel(RebaseUnits units, int64_t limit, int64_t gap,
                                                                    int64_t* __restrict__ delta, int64_t* __restrict__ offsets) {
    constexpr int NW = REBASE_BLOCK / WAVE;
    __shared__ long long wsum[NW];
    const RebaseDev& un = units.u[blockIdx.x];
    const int64_t n = un.n_ids;
    const int lane = (int)threadIdx.x & (WAVE - 1), wv = (int)threadIdx.x / WAVE;
    if (n == 0 || (long long)un.t[n - 1] < (long long)limit) {   // (uniform) not triggered whatever the gaps: nothing is scanned
        if (threadIdx.x == 0) delta[blockIdx.x] = 0;
        return;
    }
    const long long prev = ((uint32_t)un.slot & REBASE_HAS_PREV) ? (long long)un.t[-1] : -1ll;
    long long carry = 0;   // d of the last id before the tile
    for (int64_t base = 0; base < n; base += RTK_RENUMBER_TILE) {
        const int64_t i0 = base + (int64_t)threadIdx.x * RENUMBER_ITEMS;
        long long before = i0 == 0 ? prev : (i0 < n ? (long long)un.t[i0 - 1] : 0ll);
        long long part[RENUMBER_ITEMS], run = 0;   // inclusive sums over the thread's own ids
#pragma unroll
        for (int j = 0; j < RENUMBER_ITEMS; ++j) {
            if (i0 + j < n) {
                const long long cur = (long long)un.t[i0 + j];
                const long long ex = cur - before - (i0 + j == 0 ? 1ll : (long long)gap);
                run += ex > 0 ? ex : 0ll;
                before = cur;
            }
            part[j] = run;
        }
        long long inc = run;   // inclusive over the wave
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long up = __shfl_up(inc, o, WAVE);
            if (lane >= o) inc += up;
        }
        if (lane == WAVE - 1) wsum[wv] = inc;
        __syncthreads();
        long long pre = carry + inc - run, tile = 0;   // pre: d of the id before the thread's first
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const long long s = wsum[w];
            if (w < wv) pre += s;
            tile += s;
        }
#pragma unroll
        for (int j = 0; j < RENUMBER_ITEMS; ++j)
            if (i0 + j < n) un.row_delta[i0 + j] = pre + part[j];
        carry += tile;
        __syncthreads();   // (wsum is written again in the next tile)
    }
    if (threadIdx.x != 0) return;
    const long long d = carry > 0 ? carry : 0ll;
    delta[blockIdx.x] = d;
    if (d != 0) offsets[(uint32_t)un.slot & ~REBASE_HAS_PREV] += d;   // (slots of one call are distinct: checked on the host)
}

template <int DT>
__global__ __launch_bounds__(REBASE_BLOCK) void renumber_apply_kernel(RebaseUnits units, int D, const float* __restrict__ inv_freq,
                                                                     RowSel rs, const int64_t* __restrict__ delta) {
    using V = Vec16<DT>;
    constexpr int VE = V::VE;
    constexpr int ES = 16 / VE;
    if (delta[blockIdx.y] == 0) return;   // (uniform)
    const RebaseDev& un = units.u[blockIdx.y];
    const int64_t* __restrict__ rd = un.row_delta;
    // the ids: t[i] -= d[i]
    for (int64_t i = (int64_t)blockIdx.x * REBASE_BLOCK + threadIdx.x; i < un.n_ids; i += (int64_t)gridDim.x * REBASE_BLOCK) {
        const long long dl = (long long)rd[i];
        if (dl != 0) un.t[i] -= dl;
    }
    // the keys: chunk pair cp of `span` ADJACENT rows - row lane r0's share of the workgroup's own block of `per` rows
    const int h2 = D / 2, lpr = h2 / VE, rpb = REBASE_BLOCK / lpr;
    const int r0 = (int)threadIdx.x / lpr, cp = (int)threadIdx.x - r0 * lpr;
    if (r0 >= rpb) return;
    const int d = cp * VE;
    const uint32_t temporal = rebase_temporal<VE>(rs, d);
    if (temporal == 0) return;
    uint32_t take[4];
    rebase_take<DT>(temporal, take);
    const int64_t steps = (un.rows + rpb - 1) / rpb, per = (steps + gridDim.x - 1) / gridDim.x * rpb;
    const int64_t span = per / rpb, begin = (int64_t)blockIdx.x * per + r0 * span, stop = min(un.rows, begin + span);
    const int64_t row_bytes = (int64_t)D * ES;
    float c[VE], s[VE];
    long long have = 0;   // the delta c / s are the cos / sin of (0: none yet)
    for (int64_t r = begin; r < stop; ++r) {
        const long long dl = (long long)rd[r];
        if (dl == 0) continue;   // the row keeps its bits
        if (dl != have) {
            rebase_sincos<VE>((float)dl, inv_freq, d, temporal, c, s);
            have = dl;
        }
        rebase_rotate_row<DT>(un.k + r * row_bytes + (int64_t)d * ES, un.H, un.stride_h, (int64_t)h2 * ES, c, s, take);
    }
}

// The host's checks of the shared arguments and of every unit's rtk_rebase_unit fields (Unit: rtk_rebase_unit or
// rtk_renumber_unit, which has its fields).  > 0: go on (es and ve are set); else what the entry point returns.
template <typename Unit>
int rebase_check(const Unit* units, int n_units, int D, int dtype, int P, const float* inv_freq, int64_t limit,
                 const int64_t* offsets, const int64_t* delta, int& es, int& ve, const char* who) {
    int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    RTK_CHECK_ARG(inv_freq && offsets && delta, "%s: NULL pointer (inv_freq / offsets / delta)", who);
    RTK_CHECK_ARG(limit >= 0, "%s: negative limit %lld", who, (long long)limit);
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "%s: unsupported dtype %d", who, dtype);
    RTK_CHECK_ARG(D >= 2, "%s: head_dim %d", who, D);
    RTK_CHECK_ARG(P == 1 || P == 3, "%s: P must be 1 or 3, got %d", who, P);
    for (int i = 0; i < n_units; ++i) {
        const Unit& u = units[i];
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
    return 1;
}

// ... and the conditions under which the apply kernels' 16-byte accesses do not serve: RTK_EUNSUPPORTED
template <typename Unit>
int rebase_supported(const Unit* units, int n_units, int D, int P, const int* sections_host, int nsec, int ve, RowSel& rs,
                     const char* who) {
    bool aligned = D % (2 * ve) == 0 && D <= 256;
    for (int i = 0; i < n_units; ++i)
        aligned = aligned && ((uintptr_t)units[i].k & 15) == 0 && units[i].k_stride_h % 16 == 0 && ((uintptr_t)units[i].ids & 7) == 0;
    if (!aligned) {
        set_error("%s: needs 16-byte aligned rows and head strides and head_dim a multiple of %d (<= 256)", who, 2 * ve);
        return RTK_EUNSUPPORTED;
    }
    int rc;
    if ((rc = make_rowsel(rs, P, D, sections_host, nsec, who)) != RTK_OK) return rc;
    for (int d = 0; d < D / 2; ++d)
        if ((rs.row[d] == 0) != (rs.row[d + D / 2] == 0)) {
            set_error("%s: channel %d and its rotation partner follow different id rows", who, d);
            return RTK_EUNSUPPORTED;
        }
    return RTK_OK;
}

// Both entry points: the checks, then per RTK_REBASE_MAX_UNITS units the first launch (decide or scan) and the apply launch.
// `gap` is the renumbering's alone
template <typename Unit>
int rebase_run(const char* who, const Unit* units, int n_units, int D, int dtype, int P, const float* inv_freq,
               const int* sections_host, int nsec, int64_t limit, int64_t gap, int64_t* offsets, int64_t* delta, rtk_stream_t stream) {
    constexpr bool RENUMBER = std::is_same_v<Unit, rtk_renumber_unit>;
    int es, ve;
    int rc = rebase_check(units, n_units, D, dtype, P, inv_freq, limit, offsets, delta, es, ve, who);
    if (rc <= 0) return rc;
    if constexpr (RENUMBER) {
        RTK_CHECK_ARG(gap >= 1, "%s: gap %lld < 1", who, (long long)gap);
        for (int i = 0; i < n_units; ++i) {
            const Unit& u = units[i];
            RTK_CHECK_ARG(u.rows <= u.end - u.first, "%s: unit %d: %lld K rows for %lld ids", who, i, (long long)u.rows,
                          (long long)(u.end - u.first));
            RTK_CHECK_ARG(u.row_delta && ((uintptr_t)u.row_delta & 7) == 0, "%s: unit %d: row_delta is NULL or not 8-byte aligned", who, i);
        }
    }
    RowSel rs;
    if ((rc = rebase_supported(units, n_units, D, P, sections_host, nsec, ve, rs, who)) != RTK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_units; b += RTK_REBASE_MAX_UNITS) {
        const int n = std::min(n_units - b, RTK_REBASE_MAX_UNITS);
        RebaseUnits ru;
        int64_t most = 1;
        for (int j = 0; j < RTK_REBASE_MAX_UNITS; ++j) {
            const Unit& u = units[b + std::min(j, n - 1)];   // (slots past n repeat the last unit and are never read)
            RebaseDev& dv = ru.u[j];
            dv.k = (char*)u.k + u.first * (int64_t)D * es;
            dv.stride_h = u.k_stride_h;
            dv.t = u.ids + u.first;
            dv.n_ids = u.end - u.first;
            dv.rows = u.rows;
            if constexpr (RENUMBER) dv.row_delta = u.row_delta;
            else dv.row_delta = nullptr;
            dv.H = u.H;
            dv.slot = (int32_t)((uint32_t)u.slot | (u.first > 0 ? REBASE_HAS_PREV : 0u));
            most = std::max(most, std::max(u.rows, (dv.n_ids + REBASE_BLOCK - 1) / REBASE_BLOCK));
        }
        if constexpr (RENUMBER) {
            RTK_LAUNCH(KID_RENUMBER_SCAN, renumber_scan_kernel, dim3(n), dim3(REBASE_BLOCK), 0, st, ru, limit, gap, delta + b, offsets);
            RTK_LAUNCH_CHECK("renumber_scan_kernel");
        } else {
            RTK_LAUNCH(KID_REBASE_DECIDE, rebase_decide_kernel, dim3(n), dim3(WAVE), 0, st, ru, limit, delta + b, offsets);
            RTK_LAUNCH_CHECK("rebase_decide_kernel");
        }
        // workgroups per unit: the machine's share, and no more than the largest unit has steps for
        const int rpb = REBASE_BLOCK / (D / 2 / ve);
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((REBASE_WGS + n - 1) / n, (most + rpb - 1) / rpb));
        const int64_t* dl = delta + b;
        with_payload(dtype, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            if constexpr (RENUMBER)
                RTK_LAUNCH(KID_RENUMBER, renumber_apply_kernel<DT>, dim3(gx, n), dim3(REBASE_BLOCK), 0, st, ru, D, inv_freq, rs, dl);
            else
                RTK_LAUNCH(KID_REBASE, rebase_apply_kernel<DT>, dim3(gx, n), dim3(REBASE_BLOCK), 0, st, ru, D, inv_freq, rs, dl);
            return 0;
        });
        RTK_LAUNCH_CHECK(RENUMBER ? "renumber_apply_kernel" : "rebase_apply_kernel");
    }
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

extern "C" int rtk_pivotkv_rebase_batched(const rtk_rebase_unit* units, int n_units, int D, int dtype, int P,
                                          const float* inv_freq, const int* sections_host, int nsec, int64_t limit,
                                          int64_t* offsets, int64_t* delta, rtk_stream_t stream) {
    return rtk::rebase_run("rtk_pivotkv_rebase_batched", units, n_units, D, dtype, P, inv_freq, sections_host, nsec, limit, 0,
                           offsets, delta, stream);
}

extern "C" int rtk_pivotkv_renumber_batched(const rtk_renumber_unit* units, int n_units, int D, int dtype, int P,
                                            const float* inv_freq, const int* sections_host, int nsec, int64_t limit, int64_t gap,
                                            int64_t* offsets, int64_t* delta, rtk_stream_t stream) {
    return rtk::rebase_run("rtk_pivotkv_renumber_batched", units, n_units, D, dtype, P, inv_freq, sections_host, nsec, limit, gap,
                           offsets, delta, stream);
}

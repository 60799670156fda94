// pivotkv_renumber.hip - renumber the position ids of a bounded video region row by row and re-rotate its keys, in place, for
// many layers in one call (retake_hip.h §R "Position renumbering"; a rule of this project's own, the reference has no
// counterpart).  It generalises pivotkv_rebase.hip's one delta per unit to one delta per row.
//
// Per unit (a layer): t = row 0 of its ids, the region's ids are t[first, end), prev = first > 0 ? t[first - 1] : -1.
//     e[first] = max(0, t[first] - prev - 1)                  the region follows the pinned rows (the re-base's delta)
//     e[i]     = max(0, t[i] - t[i - 1] - gap)                inner gaps above `gap` close to `gap`; gaps <= gap stay
//     d[i]     = e[first] + ... + e[i],   total = d[end - 1]
//     if total > 0 and t[end - 1] >= limit:   t[i] -= d[i];  K row r <- R(-d[first + r]) K row r on the temporal channel
//                                             pairs;  offsets[slot] += total
//
// Two launches and no order between workgroups - no flags, no counters, no waiting.  The scan launch (one workgroup per
// unit) only READS ids: it walks [first, end) in tiles of RTK_RENUMBER_TILE ids - a wave-level inclusive scan, the waves'
// sums through LDS, a running int64 carry - and writes d into the unit's row_delta scratch, the total (0: not triggered)
// into delta[unit], and advances offsets[slot]; a unit whose last id is below the limit is not scanned at all.  The apply
// launch decides from delta[unit] alone, rewrites the ids from row_delta and rotates the keys: the rebase apply's layout (a
// thread owns one 16-byte chunk pair d / d + D/2 and walks heads in batches), with the cos / sin now a function of the row.
// A workgroup owns a CONTIGUOUS block of rows, a thread walks ADJACENT rows of it and keeps its cos / sin while the next row
// has the same delta - the rows of one id share them, and a region with few holes pays the fp64 sin / cos rarely (measured
// against rows 256 / lanes apart per thread, which keeps a wave's requests contiguous: 1 - 2 % slower in every pattern,
// DESIGN.md §4); a row with d = 0 is neither loaded nor stored.
#include "rebase_rotate.cuh"

namespace rtk {
namespace {

constexpr int RENUMBER_ITEMS = RTK_RENUMBER_TILE / REBASE_BLOCK;   // consecutive ids of a thread in a tile
static_assert(RENUMBER_ITEMS * REBASE_BLOCK == RTK_RENUMBER_TILE, "a tile is a whole number of ids per thread");

struct RenumberDev {
    char* k;              // first byte of row `first` of head 0
    int64_t stride_h;     // bytes between heads
    int64_t* t;           // &ids[0][first]
    int64_t n_ids;        // end - first
    int64_t rows;         // K rows of the region (<= n_ids)
    int64_t* row_delta;   // [n_ids] scratch: d of every region id
    int32_t H;
    int32_t slot;         // bit 31: first > 0 (t[-1] is the last pinned id)
};
struct RenumberUnits {
    RenumberDev u[RTK_REBASE_MAX_UNITS];
};

// one workgroup per unit.  delta[unit] is written for every unit of the launch; row_delta for every region id of a unit whose
// last id has reached the limit
__global__ __launch_bounds__(REBASE_BLOCK) void renumber_scan_kernel(RenumberUnits units, int64_t limit, int64_t gap,
                                                                    int64_t* __restrict__ delta, int64_t* __restrict__ offsets) {
    constexpr int NW = REBASE_BLOCK / WAVE;
    __shared__ long long wsum[NW];
    const RenumberDev& un = units.u[blockIdx.x];
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
__global__ __launch_bounds__(REBASE_BLOCK) void renumber_apply_kernel(RenumberUnits units, int D, const float* __restrict__ inv_freq,
                                                                     RowSel rs, const int64_t* __restrict__ delta) {
    using V = Vec16<DT>;
    constexpr int VE = V::VE;
    constexpr int ES = 16 / VE;
    if (delta[blockIdx.y] == 0) return;   // (uniform)
    const RenumberDev& un = units.u[blockIdx.y];
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

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_renumber_batched(const rtk_renumber_unit* units, int n_units, int D, int dtype, int P,
                                            const float* inv_freq, const int* sections_host, int nsec, int64_t limit, int64_t gap,
                                            int64_t* offsets, int64_t* delta, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_renumber_batched";
    int es, ve;
    int rc = rebase_check(units, n_units, D, dtype, P, inv_freq, limit, offsets, delta, es, ve, who);
    if (rc <= 0) return rc;
    RTK_CHECK_ARG(gap >= 1, "%s: gap %lld < 1", who, (long long)gap);
    for (int i = 0; i < n_units; ++i) {
        const rtk_renumber_unit& u = units[i];
        RTK_CHECK_ARG(u.rows <= u.end - u.first, "%s: unit %d: %lld K rows for %lld ids", who, i, (long long)u.rows,
                      (long long)(u.end - u.first));
        RTK_CHECK_ARG(u.row_delta && ((uintptr_t)u.row_delta & 7) == 0, "%s: unit %d: row_delta is NULL or not 8-byte aligned", who, i);
    }
    RowSel rs;
    if ((rc = rebase_supported(units, n_units, D, P, sections_host, nsec, ve, rs, who)) != RTK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_units; b += RTK_REBASE_MAX_UNITS) {
        const int n = std::min(n_units - b, RTK_REBASE_MAX_UNITS);
        RenumberUnits ru;
        int64_t most = 1;
        for (int j = 0; j < RTK_REBASE_MAX_UNITS; ++j) {
            const rtk_renumber_unit& u = units[b + std::min(j, n - 1)];   // (slots past n repeat the last unit and are never read)
            RenumberDev& dv = ru.u[j];
            dv.k = (char*)u.k + u.first * (int64_t)D * es;
            dv.stride_h = u.k_stride_h;
            dv.t = u.ids + u.first;
            dv.n_ids = u.end - u.first;
            dv.rows = u.rows;
            dv.row_delta = u.row_delta;
            dv.H = u.H;
            dv.slot = (int32_t)((uint32_t)u.slot | (u.first > 0 ? REBASE_HAS_PREV : 0u));
            most = std::max(most, std::max(u.rows, (dv.n_ids + REBASE_BLOCK - 1) / REBASE_BLOCK));
        }
        RTK_LAUNCH(KID_RENUMBER_SCAN, renumber_scan_kernel, dim3(n), dim3(REBASE_BLOCK), 0, st, ru, limit, gap, delta + b, offsets);
        RTK_LAUNCH_CHECK("renumber_scan_kernel");
        // workgroups per unit: the machine's share, and no more than the largest unit has steps for
        const int rpb = REBASE_BLOCK / (D / 2 / ve);
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((REBASE_WGS + n - 1) / n, (most + rpb - 1) / rpb));
        const int64_t* dl = delta + b;
        with_payload(dtype, [&](auto dt) {
            RTK_LAUNCH(KID_RENUMBER, renumber_apply_kernel<decltype(dt)::value>, dim3(gx, n), dim3(REBASE_BLOCK), 0, st, ru, D, inv_freq,
                       rs, dl);
            return 0;
        });
        RTK_LAUNCH_CHECK("renumber_apply_kernel");
    }
    return RTK_OK;
}

// pivotkv_slide.hip - the sliding video window's move: rows of many independent byte streams moved DOWN in place, one call
// (retake_hip.h "Sliding window").  Per unit and stream it is memmove(dst, dst + drop_bytes, n_bytes) with drop_bytes > 0:
// source and destination overlap almost entirely (a window of ~100 k rows slides by ~1.5 k), and nothing orders workgroups.
//
// Partition: the byte at destination offset x takes the byte at x + drop_bytes, which itself is the destination of
// x + 2 drop_bytes, ...: the dependency chains run along the residues x mod drop_bytes and never cross them.  A workgroup
// therefore owns one stream, or - once drop_bytes exceeds what it moves per step - one SLICE of the residues of one stream,
// and walks its chains from low addresses to high, a tile per step:
//     narrow drop (drop_bytes <  TILE): one workgroup per stream, step k covers offsets [k TILE, (k + 1) TILE);
//     wide drop   (drop_bytes >= TILE): ceil(drop_bytes / TILE) slices per stream, step k of slice [a, a + span) covers
//                                       offsets [k drop_bytes + a, k drop_bytes + a + span).
// Either way every byte is read by the workgroup that overwrites it, and step k's stores end below step k + 1's sources.
// A store of step k can only hit bytes that loads of steps <= k read.  Narrow: those loads may be another thread's, so every
// thread waits for its own loads (vmcnt: a barrier alone does not drain them), then the workgroup barriers, then it stores.
// Wide: a thread's offsets repeat with period drop_bytes, i.e. what it overwrites at step k is what it loaded itself at step
// k - 1 - its own data dependence is the order, no barrier.  Step k + 1 is requested before step k is stored (its
// sources lie above everything stored so far).  Ranges that do not overlap at all (drop >= rows) are the wide case with
// one step: fully parallel.  No flags, no counters, no waiting between workgroups.
//
// Roofline: HBM, 2 x n_bytes per stream.  16-byte accesses where the unit's pointer, stride, drop and length allow, else
// 4-byte ones (the fp32 scale rows of the fp8 archive, ids at an odd row).
#include <algorithm>

#include "common.cuh"

namespace rtk {
namespace {

constexpr int SLIDE_BLOCK = 256;
constexpr int SLIDE_U = 4;   // vectors per thread and step

// a unit as the kernel sees it: every stream is "dst[x] = dst[x + drop_bytes], x < n_bytes" from its own dst
struct SlideDev {
    char* dst;              // first destination byte of stream 0
    int64_t stream_stride;  // bytes
    int64_t drop_bytes;     // > 0
    int64_t n_bytes;        // > 0
    int32_t streams;
    int32_t slices;         // workgroups per stream; bit 30: 16-byte accesses
};
constexpr int SLIDE_WIDE16 = 1 << 30;
struct SlideUnits {
    SlideDev u[RTK_SLIDE_MAX_UNITS];
};

template <class V> __device__ __forceinline__ int64_t slide_tile() { return (int64_t)SLIDE_BLOCK * SLIDE_U * sizeof(V); }

template <class V>
__device__ __forceinline__ void slide_stream(char* __restrict__ d, int64_t db, int64_t n, int slice, int slices) {
    constexpr int64_t VB = sizeof(V);
    const int64_t TILE = slide_tile<V>();
    const bool narrow = db < TILE;
    // the residues [a, a + span) this workgroup owns out of [0, cover), and how far a step advances.  span <= TILE: the
    // launcher cuts ceil(cover / TILE) slices
    const int64_t cover = narrow ? n : min(db, n);    // (a drop beyond the moved rows: one step, residues [0, n))
    const int64_t span = narrow ? TILE : (((cover + slices - 1) / slices + VB - 1) / VB) * VB;
    const int64_t a = (int64_t)slice * span;
    const int64_t step = narrow ? TILE : db;
    const int64_t steps = (n + step - 1) / step;
    int64_t off[SLIDE_U];
    bool own[SLIDE_U];
#pragma unroll
    for (int u = 0; u < SLIDE_U; ++u) {
        const int64_t e = ((int64_t)u * SLIDE_BLOCK + threadIdx.x) * VB;
        off[u] = a + e;
        own[u] = e < span && off[u] < cover;
    }
    // loads are unconditional (a clamped address: a branch around a load costs a wait per element); stores are predicated.
    // Two register tiles take turns, so that no register copy makes a step wait for the one requested after it
    const int64_t last = n - VB;
    auto load = [&](V (&r)[SLIDE_U], int64_t x0) {
#pragma unroll
        for (int u = 0; u < SLIDE_U; ++u) r[u] = __builtin_nontemporal_load((const V*)(d + min(x0 + off[u], last) + db));
    };
    auto store = [&](const V (&r)[SLIDE_U], int64_t x0) {
#pragma unroll
        for (int u = 0; u < SLIDE_U; ++u)
            if (own[u] && x0 + off[u] < n) __builtin_nontemporal_store(r[u], (V*)(d + x0 + off[u]));
    };
    auto sync = [&]() {   // (uniform) narrow: other threads' stores of this step hit what this thread has requested
        if (narrow) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    };
    // (every load is issued, also the ones past the last step - their clamped addresses are in bounds and nothing stores
    // them: a load inside a branch would make the compiler's wait counts assume the worst of both paths)
    V t0[SLIDE_U], t1[SLIDE_U];
    load(t0, 0);
    for (int64_t k = 0; k < steps; k += 2) {
        sync();
        load(t1, (k + 1) * step);
        store(t0, k * step);
        sync();
        load(t0, (k + 2) * step);
        store(t1, (k + 1) * step);   // (an odd count of steps: (k + 1) * step >= n, nothing is stored)
    }
}

__global__ __launch_bounds__(SLIDE_BLOCK) void slide_units_kernel(SlideUnits units) {
    const SlideDev& un = units.u[blockIdx.y];
    const int slices = un.slices & ~SLIDE_WIDE16;
    const int s = blockIdx.x / slices, slice = blockIdx.x - s * slices;
    if (s >= un.streams) return;   // (uniform: the grid is sized for the launch's largest unit)
    char* d = un.dst + (int64_t)s * un.stream_stride;
    if (un.slices & SLIDE_WIDE16) slide_stream<u32x4>(d, un.drop_bytes, un.n_bytes, slice, slices);
    else slide_stream<uint32_t>(d, un.drop_bytes, un.n_bytes, slice, slices);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_slide_batched(const rtk_slide_unit* units, int n_units, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_slide_batched";
    int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    for (int i = 0; i < n_units; ++i) {
        const rtk_slide_unit& u = units[i];
        RTK_CHECK_ARG(u.base, "%s: unit %d: NULL pointer", who, i);
        RTK_CHECK_ARG(u.first >= 0 && u.drop >= 0 && u.rows >= 0, "%s: unit %d: negative first / drop / rows", who, i);
        if ((rc = check_stream_unit(u, who, i)) != RTK_OK) return rc;
        RTK_CHECK_ARG(u.first <= (INT64_MAX >> 2) / u.row_bytes && u.drop <= (INT64_MAX >> 2) / u.row_bytes &&
                          u.rows <= (INT64_MAX >> 2) / u.row_bytes,
                      "%s: unit %d: first / drop / rows overflow a byte offset", who, i);
        // (an upper bound of the unit's workgroups: 4 KB per workgroup and step is the smaller of the two tiles)
        const int64_t cover = std::min(u.drop, u.rows) * u.row_bytes;
        RTK_CHECK_ARG((cover / (SLIDE_BLOCK * SLIDE_U * 4) + 1) <= 0x3fffffff / u.streams,
                      "%s: unit %d: too many workgroups for one launch", who, i);
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned grid_x = 0;   // of the launch being filled: its largest unit's
    return launch_units<SlideUnits>(
        n_units,
        [&](int i, SlideDev& dv) {
            const rtk_slide_unit& u = units[i];
            if (u.drop == 0 || u.rows == 0) return false;
            dv.dst = (char*)u.base + u.first * u.row_bytes;
            dv.stream_stride = u.stream_stride;
            dv.drop_bytes = u.drop * u.row_bytes;
            dv.n_bytes = u.rows * u.row_bytes;
            dv.streams = u.streams;
            const bool wide16 = aligned16(dv.dst, dv.stream_stride, dv.drop_bytes, dv.n_bytes);
            const int64_t tile = (int64_t)SLIDE_BLOCK * SLIDE_U * (wide16 ? 16 : 4);
            // slices of a wide drop; no more of them than there is work for (a drop far beyond the moved rows)
            const int64_t slices = dv.drop_bytes < tile ? 1 : (std::min(dv.drop_bytes, dv.n_bytes) + tile - 1) / tile;
            dv.slices = (int32_t)slices | (wide16 ? SLIDE_WIDE16 : 0);
            grid_x = std::max(grid_x, (unsigned)(slices * u.streams));
            return true;
        },
        [&](const SlideUnits& su, int n) -> int {
            RTK_LAUNCH(KID_SLIDE, slide_units_kernel, dim3(grid_x, n), dim3(SLIDE_BLOCK), 0, st, su);
            RTK_LAUNCH_CHECK("slide_units_kernel");
            grid_x = 0;
            return RTK_OK;
        });
}

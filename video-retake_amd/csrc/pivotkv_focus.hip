// pivotkv_focus.hip - the question-focused cache's move (retake_hip.h §T "Question focus"): rows of many independent byte
// streams gathered OUT OF PLACE into buffers of their own, one call for K, V and ids of every layer of a device.  Per unit
// and stream the destination is three runs of source rows, back to back:
//     dst row r <  head                : src row r                                   the pinned rows
//     head <= r <  head + keep         : src row first + clamp(idx[r - head], 0, n - 1)   the chosen region rows
//     r >= head + keep                 : src row tail_src + (r - head - keep)        the question and what was decoded
//
// Source and destination do not overlap (the launcher refuses units whose byte spans meet) and every destination row is
// written by exactly one wave, so there is NO order between workgroups, waves or steps: no flags, no counters, no barrier,
// no LDS, no scratch - unlike the slide and the squeeze, which move rows inside one buffer and have to order their steps.
//
// Partition: a workgroup owns FG_ROWS contiguous destination rows of one stream, a wave FG_ROWS / 4 of them, FG_U rows in
// flight per thread.  A wave takes whole rows - lane c moves vector c, c + 64, ... of each - so the source row of a
// destination row is one wave-uniform number: idx is read once per destination row, and the clamp is scalar work.  A row of
// 256 bytes (D 128, 16-bit) is 16 vectors of 16 bytes: a quarter of the lanes carry data, and the call takes 1.6 - 1.7 x
// rtk_profile_copy of the same bytes (profiles/focus_bench.json) - 5 % of a focus(), which the re-scoring dominates; packing
// four rows into a wave would give up the wave-uniform idx.  The grid is a function of the units alone.
//
// Roofline: HBM, 2 x (head + keep + tail) x row_bytes per stream + 4 bytes of idx per gathered row.  16-byte accesses where
// both bases, both strides and the row bytes allow, else 4-byte ones; the bytes are the same.
#include <algorithm>

#include "common.cuh"

namespace rtk {
namespace {

constexpr int FG_BLOCK = 256;
constexpr int FG_WAVES = FG_BLOCK / WAVE;
constexpr int FG_ROWS = 64;   // destination rows per workgroup
constexpr int FG_U = 8;       // rows in flight per thread
static_assert(FG_ROWS % (FG_WAVES * FG_U) == 0, "a wave's rows are whole batches");

// a unit as the kernel sees it; the launcher has checked that every row count fits an int32
struct FocusDev {
    const char* src;        // row 0 of source stream 0
    char* dst;              // row 0 of destination stream 0
    const int32_t* idx;     // [keep], region rows
    int64_t src_stride;     // bytes between streams
    int64_t dst_stride;
    int32_t row_bytes;
    int32_t streams;
    int32_t head, keep, tail;
    int32_t first, n;       // the region: source rows [first, first + n)
    int32_t tail_src;
    int32_t blocks;         // workgroups per stream; bit 30: 16-byte accesses
    int32_t pad;
};
constexpr int FG_WIDE16 = 1 << 30;
struct FocusUnits {
    FocusDev u[RTK_FOCUS_MAX_UNITS];
};
static_assert(sizeof(FocusUnits) <= 4096, "the units travel as a kernel argument");

template <class V>
__device__ __forceinline__ void focus_rows(const FocusDev& un, const char* __restrict__ s, char* __restrict__ d, int row0) {
    constexpr int VB = sizeof(V);
    const int lane = threadIdx.x & (WAVE - 1);
    const int head = un.head, keep = un.keep, total = un.head + un.keep + un.tail;
    const int row_bytes = un.row_bytes, vpr = row_bytes / VB;
    const int32_t* __restrict__ idx = un.idx;
    const int last = un.n - 1;
    const int wave0 = row0 + uniform_int(threadIdx.x / WAVE) * (FG_ROWS / FG_WAVES);
    for (int b = 0; b < FG_ROWS / FG_WAVES; b += FG_U) {
        const int r0 = wave0 + b;
        if (r0 >= total) break;   // (uniform)
        // the source rows of this batch: wave-uniform.  A row past the stream's end repeats the last one - its loads are in
        // bounds and nothing stores them
        int64_t so[FG_U];
#pragma unroll
        for (int u = 0; u < FG_U; ++u) {
            const int r = min(r0 + u, total - 1);
            int src;
            if (r < head) {
                src = r;
            } else if (r < head + keep) {
                const int i = uniform_int(idx[r - head]);
                src = un.first + min(max(i, 0), last);   // inside [first, first + n) whatever the list says
            } else {
                src = un.tail_src + (r - head - keep);
            }
            so[u] = (int64_t)src * row_bytes;
        }
        for (int c = lane; c < vpr; c += WAVE) {
            V t[FG_U];
#pragma unroll
            for (int u = 0; u < FG_U; ++u) t[u] = __builtin_nontemporal_load((const V*)(s + so[u] + (int64_t)c * VB));
#pragma unroll
            for (int u = 0; u < FG_U; ++u)
                if (r0 + u < total) __builtin_nontemporal_store(t[u], (V*)(d + (int64_t)(r0 + u) * row_bytes + (int64_t)c * VB));
        }
    }
}

__global__ __launch_bounds__(FG_BLOCK) void focus_gather_kernel(FocusUnits units) {
    const FocusDev& un = units.u[blockIdx.y];
    const int blocks = un.blocks & ~FG_WIDE16;
    const int s = blockIdx.x / blocks, blk = blockIdx.x - s * blocks;
    if (s >= un.streams) return;   // (uniform: the grid is sized for the launch's largest unit)
    const char* src = un.src + (int64_t)s * un.src_stride;
    char* dst = un.dst + (int64_t)s * un.dst_stride;
    if (un.blocks & FG_WIDE16) focus_rows<u32x4>(un, src, dst, blk * FG_ROWS);
    else focus_rows<uint32_t>(un, src, dst, blk * FG_ROWS);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_focus_gather_batched(const rtk_focus_unit* units, int n_units, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_focus_gather_batched";
    const int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    constexpr int64_t MOST = 0x7fff0000;   // rows: every count and source row fits an int32
    for (int i = 0; i < n_units; ++i) {
        const rtk_focus_unit& u = units[i];
        RTK_CHECK_ARG(u.src && u.dst, "%s: unit %d: NULL pointer", who, i);
        RTK_CHECK_ARG(u.head >= 0 && u.first >= 0 && u.n >= 0 && u.keep >= 0 && u.tail_src >= 0 && u.tail >= 0,
                      "%s: unit %d: negative head / first / n / keep / tail_src / tail", who, i);
        RTK_CHECK_ARG(u.keep <= u.n, "%s: unit %d: keep %lld exceeds n %lld", who, i, (long long)u.keep, (long long)u.n);
        RTK_CHECK_ARG(u.keep == 0 || u.idx, "%s: unit %d: NULL idx", who, i);
        RTK_CHECK_ARG(u.streams > 0, "%s: unit %d: streams %d", who, i, u.streams);
        RTK_CHECK_ARG(u.row_bytes > 0 && u.row_bytes % 4 == 0, "%s: unit %d: row_bytes %d is not a positive multiple of 4", who, i,
                      u.row_bytes);
        RTK_CHECK_ARG((((uintptr_t)u.src | (uintptr_t)u.dst) & 3) == 0 && u.src_stride % 4 == 0 && u.dst_stride % 4 == 0,
                      "%s: unit %d: src / dst / stream strides not 4-byte aligned", who, i);
        RTK_CHECK_ARG(u.src_stride >= 0 && u.dst_stride >= 0, "%s: unit %d: negative stream stride", who, i);
        RTK_CHECK_ARG(u.head <= MOST && u.first <= MOST && u.n <= MOST && u.tail_src <= MOST && u.tail <= MOST &&
                          u.first + u.n <= MOST && u.tail_src + u.tail <= MOST && u.head + u.keep + u.tail <= MOST,
                      "%s: unit %d: a row count does not fit an int32", who, i);
        const int64_t total = u.head + u.keep + u.tail;
        if (total == 0) continue;
        // the rows the kernel may read of a source stream, and the byte spans of the whole unit on either side
        const int64_t src_rows = std::max(u.head, std::max(u.keep ? u.first + u.n : 0, u.tail ? u.tail_src + u.tail : 0));
        RTK_CHECK_ARG(u.src_stride <= (INT64_MAX >> 2) / u.streams && u.dst_stride <= (INT64_MAX >> 2) / u.streams,
                      "%s: unit %d: stream strides overflow a byte offset", who, i);
        RTK_CHECK_ARG(u.streams == 1 || u.dst_stride >= total * u.row_bytes,
                      "%s: unit %d: dst_stride %lld is smaller than the %lld rows of a destination stream", who, i,
                      (long long)u.dst_stride, (long long)total);
        const uintptr_t s0 = (uintptr_t)u.src, s1 = s0 + (uintptr_t)((u.streams - 1) * u.src_stride + src_rows * u.row_bytes);
        const uintptr_t d0 = (uintptr_t)u.dst, d1 = d0 + (uintptr_t)((u.streams - 1) * u.dst_stride + total * u.row_bytes);
        RTK_CHECK_ARG(s1 <= d0 || d1 <= s0, "%s: unit %d: source and destination ranges overlap (the move is out of place)", who, i);
        RTK_CHECK_ARG((total + FG_ROWS - 1) / FG_ROWS <= 0x3fffffff / u.streams, "%s: unit %d: too many workgroups for one launch",
                      who, i);
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned grid_x = 0;   // of the launch being filled: its largest unit's
    return launch_units<FocusUnits>(
        n_units,
        [&](int i, FocusDev& dv) {
            const rtk_focus_unit& u = units[i];
            const int64_t total = u.head + u.keep + u.tail;
            if (total == 0) return false;
            dv.src = (const char*)u.src;
            dv.dst = (char*)u.dst;
            dv.idx = u.idx;
            dv.src_stride = u.src_stride;
            dv.dst_stride = u.dst_stride;
            dv.row_bytes = u.row_bytes;
            dv.streams = u.streams;
            dv.head = (int32_t)u.head;
            dv.keep = (int32_t)u.keep;
            dv.tail = (int32_t)u.tail;
            dv.first = (int32_t)u.first;
            dv.n = (int32_t)u.n;
            dv.tail_src = (int32_t)u.tail_src;
            dv.pad = 0;
            const int32_t blocks = (int32_t)((total + FG_ROWS - 1) / FG_ROWS);
            dv.blocks = blocks | (aligned16(dv.src, dv.dst, dv.src_stride, dv.dst_stride, dv.row_bytes) ? FG_WIDE16 : 0);
            grid_x = std::max(grid_x, (unsigned)blocks * (unsigned)u.streams);
            return true;
        },
        [&](const FocusUnits& fu, int n) -> int {
            hipLaunchKernelGGL(focus_gather_kernel, dim3(grid_x, n), dim3(FG_BLOCK), 0, st, fu);
            RTK_LAUNCH_CHECK("focus_gather_kernel");
            grid_x = 0;
            return RTK_OK;
        });
}

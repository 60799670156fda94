// pivotkv_budget.hip - the video budget (retake_hip.h "Video budget"): a bounded cache that keeps its best-scored rows.
//   keep_scores_kernel     per flush: the score the selection saw for every kept row, into the layer's score store
//   budget_select_kernel   per eviction: the newest row + an exact top-(keep - 1) of the others, ascending int32 indices
//   squeeze_units_kernel   per eviction: rows of many independent byte streams gathered DOWN in place, row[r] = row[idx[r]]
//
// The squeeze is the hot path (K, V, ids and scores of every layer; ~11.5 GB at 100 352 bf16 rows x 28 layers).  idx ascends
// and idx[r] >= r, so a row only ever moves down, and source and destination overlap almost entirely - like the slide's
// narrow case (pivotkv_slide.hip), but the distance grows along the stream, so there are no residue classes to own.
// Partition: a workgroup owns one stream, or one COLUMN SLICE (SQZ_SLICE bytes of every row) of one stream, and walks the
// rows upward, R rows per step.  Step k stores rows [k R, (k + 1) R) of its columns; every source of a step > k lies at or
// above row (k + 1) R (idx[r] >= r), so a store can only hit bytes that loads of steps <= k read.  Those may be another
// thread's loads of the same step, so every thread waits for its own loads (vmcnt: a barrier alone does not drain them; on
// CDNA the counter covers the stores of the step before as well), then the workgroup barriers, then it stores.  Step k + 1
// is requested before step k is stored, and the index entries of step k + 2 before that.  No flags, no counters, no waiting
// between workgroups, no scratch buffer.  The kernel clamps idx[r] into [r, rows_in - 1]: with ANY list every load and store
// stays inside the unit's rows and the order argument above still holds (it only needs source >= destination).
//
// Roofline: HBM, 2 x rows_out x row_bytes per stream + 4 bytes of idx per row and slice.  16-byte accesses where the unit's
// pointer, stride and row bytes allow, else 4-byte ones (scales, scores, ids at an odd row).
#include <algorithm>

#include "common.cuh"
#include "select.cuh"

namespace rtk {
namespace {

// ---- keep scores ---------------------------------------------------------------------------------------------------
constexpr int KSC_BLOCK = 256;
struct KeepScoreUnits {
    rtk_keep_scores_unit u[RTK_KEEP_SCORES_MAX_UNITS];
};

__global__ __launch_bounds__(KSC_BLOCK) void keep_scores_kernel(KeepScoreUnits units) {
    const rtk_keep_scores_unit& un = units.u[blockIdx.y];
    const int r = blockIdx.x * KSC_BLOCK + threadIdx.x;
    if (r >= un.keep) return;
    un.dst[r] = un.score[un.keep_idx ? un.keep_idx[r] : (int64_t)r];
}

// ---- budget select -------------------------------------------------------------------------------------------------
constexpr int BSEL_BLOCK = 1024;
struct BudgetSelectUnits {
    rtk_budget_select_unit u[RTK_BUDGET_SELECT_MAX_UNITS];
};

// One workgroup per unit.  The scores stay in memory (n is far beyond what LDS holds) and are re-read on every pass: four
// radix passes for the threshold, one ordered compaction.  Ties at the threshold go to the lowest index (select.cuh).
__global__ __launch_bounds__(BSEL_BLOCK) void budget_select_kernel(BudgetSelectUnits units) {
    __shared__ SelectSmem sm;
    const rtk_budget_select_unit& un = units.u[blockIdx.x];
    const float* __restrict__ score = un.score;
    int32_t* __restrict__ idx = un.idx;
    const int n = un.n, keep = un.keep;
    if (threadIdx.x == 0) idx[keep - 1] = n - 1;   // the newest row always survives
    if (keep == 1) return;                         // (uniform)
    auto key = [&](int i) { return f2key(score[i]); };
    uint32_t thr;
    int need_eq;
    block_radix_threshold<BSEL_BLOCK>(key, n - 1, keep - 1, sm, thr, need_eq);
    block_ordered_compact<BSEL_BLOCK>(key, n - 1, thr, need_eq, sm, [&](int rank, int i) { idx[rank] = i; });
}

// ---- squeeze -------------------------------------------------------------------------------------------------------
constexpr int SQZ_BLOCK = 256;
constexpr int SQZ_U = 4;        // vectors per thread and step
constexpr int SQZ_SLICE = 128;  // bytes of a row one workgroup owns

// a unit as the kernel sees it: every stream is "row[r] = row[clamp(idx[r])], r < rows_out" from its own first row
struct SqueezeDev {
    char* dst;              // row 0 of stream 0
    const int32_t* idx;
    int64_t stream_stride;  // bytes
    int32_t row_bytes;
    int32_t rows_out;       // > 0
    int32_t rows_in;        // >= rows_out
    int32_t streams;
    int32_t slices;         // workgroups per stream; bit 30: 16-byte accesses
    int32_t pad;
};
constexpr int SQZ_WIDE16 = 1 << 30;
struct SqueezeUnits {
    SqueezeDev u[RTK_SQUEEZE_MAX_UNITS];
};

template <class V>
__device__ __forceinline__ void squeeze_stream(char* __restrict__ d, const SqueezeDev& un, int slice) {
    constexpr int VB = sizeof(V);
    constexpr int TILE = SQZ_BLOCK * SQZ_U;                   // vectors per step
    const int row_bytes = un.row_bytes, rows_out = un.rows_out, last_in = un.rows_in - 1;
    const int32_t* __restrict__ idx = un.idx;
    const int col0 = slice * SQZ_SLICE;                       // first byte of this workgroup's columns
    const int vpr = min(row_bytes - col0, SQZ_SLICE) / VB;    // vectors per row here (the last slice may be narrower)
    const int R = TILE / vpr;                                 // rows per step (vpr <= SQZ_SLICE / 4 = 32 <= TILE)
    const int steps = (rows_out + R - 1) / R;
    int rr[SQZ_U], cb[SQZ_U];   // a thread's rows within a step and byte columns: the same every step
    bool own[SQZ_U];
#pragma unroll
    for (int u = 0; u < SQZ_U; ++u) {
        const int e = u * SQZ_BLOCK + threadIdx.x;
        own[u] = e < R * vpr;
        rr[u] = own[u] ? e / vpr : 0;
        cb[u] = col0 + (own[u] ? e % vpr : 0) * VB;
    }
    // loads are unconditional (clamped rows: a branch around a load costs a wait per element); stores are predicated
    auto sources = [&](int (&s)[SQZ_U], int k) {
#pragma unroll
        for (int u = 0; u < SQZ_U; ++u) s[u] = __builtin_nontemporal_load(idx + min(k * R + rr[u], rows_out - 1));
    };
    auto load = [&](V (&t)[SQZ_U], const int (&s)[SQZ_U], int k) {
#pragma unroll
        for (int u = 0; u < SQZ_U; ++u) {
            const int r = min(k * R + rr[u], rows_out - 1);
            const int src = min(max(s[u], r), last_in);   // in [r, rows_in - 1] whatever the list says
            t[u] = __builtin_nontemporal_load((const V*)(d + (int64_t)src * row_bytes + cb[u]));
        }
    };
    auto store = [&](const V (&t)[SQZ_U], int k) {
#pragma unroll
        for (int u = 0; u < SQZ_U; ++u) {
            const int r = k * R + rr[u];
            if (own[u] && r < rows_out) __builtin_nontemporal_store(t[u], (V*)(d + (int64_t)r * row_bytes + cb[u]));
        }
    };
    auto sync = [&]() {   // other threads' stores of this step hit what this thread has requested
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    // (every load is issued, also the ones past the last step - clamped, in bounds, never stored)
    V t0[SQZ_U], t1[SQZ_U];
    int s[SQZ_U];
    sources(s, 0);
    load(t0, s, 0);
    sources(s, 1);
    for (int k = 0; k < steps; k += 2) {
        sync();
        load(t1, s, k + 1);
        sources(s, k + 2);
        store(t0, k);
        sync();
        load(t0, s, k + 2);
        sources(s, k + 3);
        store(t1, k + 1);   // (an odd count of steps: every row of it is >= rows_out, nothing is stored)
    }
}

__global__ __launch_bounds__(SQZ_BLOCK) void squeeze_units_kernel(SqueezeUnits units) {
    const SqueezeDev& un = units.u[blockIdx.y];
    const int slices = un.slices & ~SQZ_WIDE16;
    const int s = blockIdx.x / slices, slice = blockIdx.x - s * slices;
    if (s >= un.streams) return;   // (uniform: the grid is sized for the launch's largest unit)
    char* d = un.dst + (int64_t)s * un.stream_stride;
    if (un.slices & SQZ_WIDE16) squeeze_stream<u32x4>(d, un, slice);
    else squeeze_stream<uint32_t>(d, un, slice);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_keep_scores_batched(const rtk_keep_scores_unit* units, int n_units, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_keep_scores_batched";
    const int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    for (int i = 0; i < n_units; ++i) {
        const rtk_keep_scores_unit& u = units[i];
        RTK_CHECK_ARG(u.keep >= 0, "%s: unit %d: keep %d", who, i, u.keep);
        RTK_CHECK_ARG(u.keep == 0 || (u.score && u.dst), "%s: unit %d: NULL score / dst", who, i);
    }
    hipStream_t st = (hipStream_t)stream;
    int most = 0;   // of the launch being filled: its largest unit's rows
    return launch_units<KeepScoreUnits>(
        n_units,
        [&](int i, rtk_keep_scores_unit& slot) {
            slot = units[i];
            most = std::max(most, slot.keep);
            return slot.keep != 0;
        },
        [&](const KeepScoreUnits& ku, int n) -> int {
            RTK_LAUNCH(KID_KEEPSC, keep_scores_kernel, dim3((most + KSC_BLOCK - 1) / KSC_BLOCK, n), dim3(KSC_BLOCK), 0, st, ku);
            RTK_LAUNCH_CHECK("keep_scores_kernel");
            most = 0;
            return RTK_OK;
        });
}

extern "C" int rtk_pivotkv_budget_select_batched(const rtk_budget_select_unit* units, int n_units, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_budget_select_batched";
    const int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    for (int i = 0; i < n_units; ++i) {
        const rtk_budget_select_unit& u = units[i];
        RTK_CHECK_ARG(u.score && u.idx, "%s: unit %d: NULL score / idx", who, i);
        RTK_CHECK_ARG(u.n >= 1, "%s: unit %d: n %d", who, i, u.n);
        RTK_CHECK_ARG(u.keep >= 1 && u.keep <= u.n, "%s: unit %d: keep %d of n %d", who, i, u.keep, u.n);
    }
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_units; b += RTK_BUDGET_SELECT_MAX_UNITS) {
        const int n = std::min(n_units - b, RTK_BUDGET_SELECT_MAX_UNITS);
        RTK_LAUNCH(KID_BSELECT, budget_select_kernel, dim3(n), dim3(BSEL_BLOCK), 0, st, pad_units<BudgetSelectUnits>(units + b, n));
        RTK_LAUNCH_CHECK("budget_select_kernel");
    }
    return RTK_OK;
}

extern "C" int rtk_pivotkv_squeeze_batched(const rtk_squeeze_unit* units, int n_units, rtk_stream_t stream) {
    const char* who = "rtk_pivotkv_squeeze_batched";
    int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    for (int i = 0; i < n_units; ++i) {
        const rtk_squeeze_unit& u = units[i];
        RTK_CHECK_ARG(u.base, "%s: unit %d: NULL pointer", who, i);
        RTK_CHECK_ARG(u.first >= 0 && u.rows_out >= 0 && u.rows_in >= 0, "%s: unit %d: negative first / rows_out / rows_in", who, i);
        RTK_CHECK_ARG(u.rows_out <= u.rows_in, "%s: unit %d: rows_out %lld exceeds rows_in %lld", who, i, (long long)u.rows_out,
                      (long long)u.rows_in);
        RTK_CHECK_ARG(u.rows_in <= 0x7fff0000, "%s: unit %d: rows_in %lld does not fit the int32 index list", who, i,
                      (long long)u.rows_in);
        RTK_CHECK_ARG(u.rows_out == 0 || u.idx, "%s: unit %d: NULL idx", who, i);
        if ((rc = check_stream_unit(u, who, i)) != RTK_OK) return rc;
        RTK_CHECK_ARG(u.first <= (INT64_MAX >> 2) / u.row_bytes, "%s: unit %d: first overflows a byte offset", who, i);
        // (the slices of a row, written so that a row_bytes near INT32_MAX does not overflow)
        RTK_CHECK_ARG((u.row_bytes - 1) / SQZ_SLICE + 1 <= 0x3fffffff / u.streams,
                      "%s: unit %d: too many workgroups for one launch", who, i);
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned grid_x = 0;   // of the launch being filled: its largest unit's
    return launch_units<SqueezeUnits>(
        n_units,
        [&](int i, SqueezeDev& dv) {
            const rtk_squeeze_unit& u = units[i];
            if (u.rows_out == 0) return false;
            dv.dst = (char*)u.base + u.first * u.row_bytes;
            dv.idx = u.idx;
            dv.stream_stride = u.stream_stride;
            dv.row_bytes = u.row_bytes;
            dv.rows_out = (int32_t)u.rows_out;
            dv.rows_in = (int32_t)u.rows_in;
            dv.streams = u.streams;
            dv.pad = 0;
            const int slices = (u.row_bytes - 1) / SQZ_SLICE + 1;
            dv.slices = slices | (aligned16(dv.dst, dv.stream_stride, dv.row_bytes) ? SQZ_WIDE16 : 0);
            grid_x = std::max(grid_x, (unsigned)(slices * u.streams));
            return true;
        },
        [&](const SqueezeUnits& su, int n) -> int {
            RTK_LAUNCH(KID_SQUEEZE, squeeze_units_kernel, dim3(grid_x, n), dim3(SQZ_BLOCK), 0, st, su);
            RTK_LAUNCH_CHECK("squeeze_units_kernel");
            grid_x = 0;
            return RTK_OK;
        });
}

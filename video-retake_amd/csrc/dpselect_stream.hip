// dpselect_stream.hip — DPSelect on a stream (retake/dpselect_stream.py): frames arrive a few at a time, live in a ring of
// R = 2 S rows (frame g in row g mod R) and leave as compressed segments of S frames.
//
//   rtk_dpselect_ingest       one pass over the new frames: copy them into the ring AND produce their distance rows, the
//                             first against the ring row of the frame before them.  dis_kernel's arithmetic (dprow.cuh), so a
//                             distance carries the bits rtk_dpselect_dis gives the same pair inside a whole video.
//   rtk_dpselect_select_ring  peaks + bonus + exact top-k of one segment whose rows wrap around the ring and whose peak
//                             windows see the neighbouring segments' rows (select.cuh's dpselect_row).
// The kept frames are gathered by rtk_gather_frames on the segment's rows, which are contiguous in the ring.
//
// Roofline: HBM-bound.  The ingest reads every new row once (plus one halo row per strip) and writes it once:
// 2 t N C sizeof(elem) + 4 t N bytes, against 3 t N C sizeof(elem) for a copy followed by rtk_dpselect_dis.
#include "common.cuh"
#include "dprow.cuh"
#include "select.cuh"

namespace rtk {

// dis_kernel's walk (dpselect.hip) over the t rows of a piece: one wave per strip of <= 64 consecutive rows of one patch
// position, lane owns vectors k*64 + lane, two rows in flight, every load unconditional (clamped addresses) so that the
// waits are counted.  The differences: the row in front of row 0 is `prev` (NULL: the stream begins here and row 0 gets the
// constant 1.0, like frame 0 of a video), and every row of the strip is stored to `out` from the registers it was loaded
// into, before it is normalised.  A row belongs to exactly one strip, so it is stored once; halo rows are only read.
template <int DT, int VPL>
__global__ __launch_bounds__(256) void ingest_kernel(const typename Elem<DT>::vec_t* __restrict__ x,
                                                     const typename Elem<DT>::vec_t* __restrict__ prev,
                                                     typename Elem<DT>::vec_t* __restrict__ out, int T, int N, int nvec,
                                                     int strip, float* __restrict__ dis) {
    using E = Elem<DT>;
    using vec_t = typename E::vec_t;
    constexpr int NE = VPL * E::PER_VEC;
    constexpr int KFULL = (VPL <= 6) ? VPL - 1 : VPL - 2;   // (dprow_load: vectors below KFULL are full for every lane)
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nstrips = (T + strip - 1) / strip;
    const int n = wave % N;
    const int s = wave / N;
    if (s >= nstrips) return;
    const int t0 = s * strip;
    const int t1 = min(T, t0 + strip);
    const size_t row_vecs = (size_t)nvec;
    const size_t frame_vecs = (size_t)N * row_vecs;
    const vec_t* xrow = x + (size_t)n * row_vecs;
    const bool first = t0 == 0 && prev == nullptr;   // the stream's frame 0 opens this strip: no pair for it

    vec_t rawA[VPL], rawB[VPL];   // two rows in flight per wave
    float nA[NE], nB[NE];         // normalised rows: odd steps in nA, even steps in nB (no copies between steps)

    // row -1 is the halo in the ring; rows beyond the strip are clamped to its last row
    auto load_row = [&](vec_t* raw, int t) {
        const vec_t* p = t < 0 ? prev + (size_t)n * row_vecs : xrow + (size_t)min(t, t1 - 1) * frame_vecs;
        dprow_load<DT, VPL>(raw, p, nvec, lane);
    };
    auto store_row = [&](const vec_t* raw, int t) {   // t0 <= t < t1
        vec_t* q = out + (size_t)t * frame_vecs + (size_t)n * row_vecs;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            const int v = k * WAVE + lane;
            if (k < KFULL || v < nvec) q[v] = raw[k];
        }
    };
    auto normalise = [&](vec_t* raw, float* cur) { dprow_normalise<DT, VPL>(raw, cur, nvec, lane); };
    const int tb = first ? 1 : t0;   // first row this wave produces a distance for
    float res = 1.0f;                // lane i: result of row tb + i
    auto emit = [&](int t, const float* prevn, const float* cur) {
        const float dot = dprow_dot<DT, VPL>(prevn, cur);
        if (lane == t - tb) res = 1.0f - dot;
    };

    load_row(rawA, first ? 0 : t0 - 1);   // frame 0 itself, or the halo row: the previous strip's last row / the ring's
    load_row(rawB, tb);
    if (first) store_row(rawA, 0);
    normalise(rawA, nA);
    load_row(rawA, tb + 1);
    int t = tb;
    for (; t + 1 < t1; t += 2) {   // whole pairs only: the loads outstanding at the loop head are always B then A
        store_row(rawB, t);
        normalise(rawB, nB);
        load_row(rawB, t + 2);
        emit(t, nA, nB);
        store_row(rawA, t + 1);
        normalise(rawA, nA);
        load_row(rawA, t + 3);
        emit(t + 1, nB, nA);
    }
    if (t < t1) {
        store_row(rawB, t);
        normalise(rawB, nB);
        emit(t, nA, nB);
    }
    const int tr = tb + lane;
    if (tr < t1) dis[(size_t)tr * N + n] = res;
    if (first && lane == 0) dis[n] = 1.0f;
}

// Generic variant: any C (scalar accesses, the row pair read through L2 as dis_kernel_generic does).  One wave per (t, n).
template <int DT>
__global__ __launch_bounds__(256) void ingest_kernel_generic(const void* __restrict__ xv, const void* __restrict__ prev,
                                                             void* __restrict__ outv, int T, int N, int C,
                                                             float* __restrict__ dis) {
    using elem_t = typename std::conditional<DT == RTK_F32, uint32_t, uint16_t>::type;
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (wave >= (size_t)T * N) return;
    const int t = (int)(wave / N), n = (int)(wave % N);
    const size_t b0 = ((size_t)t * N + n) * C;
    for (int c = lane; c < C; c += WAVE) ((elem_t*)outv)[b0 + c] = ((const elem_t*)xv)[b0 + c];
    float d = 1.0f;
    if (t > 0) d = 1.0f - dprow_pair_cos_generic<DT>(xv, b0 - (size_t)N * C, xv, b0, C, lane);
    else if (prev) d = 1.0f - dprow_pair_cos_generic<DT>(prev, (size_t)n * C, xv, b0, C, lane);
    if (lane == 0) dis[(size_t)t * N + n] = d;
}

// One workgroup per row (sync: the patch-mean row; async: one per patch position) of one segment: `len` frames from ring
// row r0 on, rows taken modulo R, with `left` / `right` valid rows around them for the peak windows.
__global__ __launch_bounds__(SEL_BLOCK) void dpselect_select_ring_kernel(const float* __restrict__ dis, int R, int N, int r0,
                                                                         int len, int left, int right, int keep, int window,
                                                                         int sync, int64_t* __restrict__ idx,
                                                                         uint8_t* __restrict__ mask,
                                                                         float* __restrict__ keys) {
    __shared__ SelectSmem sm;
    const int row = blockIdx.x;
    // keys: async [N, len]; sync [len] keys, then the [left + len + right] patch means
    dpselect_row<SEL_BLOCK>([&](int j) { return dis + (size_t)((r0 + j + R) % R) * N; }, N, row, len, left, right, keep,
                            window, sync, idx, mask, keys + (size_t)row * len, keys + (size_t)len, sm);
}

}  // namespace rtk

using namespace rtk;

template <int DT>
static int launch_ingest(const void* x, const void* prev, int T, int N, int C, void* out, float* dis, hipStream_t st) {
    constexpr int PV = Elem<DT>::PER_VEC;
    using vec_t = typename Elem<DT>::vec_t;
    const bool vec_ok = (C % PV == 0) && aligned16(x, prev, out);
    const int nvec = C / PV;
    const int vpl = (nvec + WAVE - 1) / WAVE;
    if (!vec_ok || vpl > 16) {
        const size_t waves = (size_t)T * N;
        const unsigned grid = (unsigned)((waves * WAVE + 255) / 256);
        RTK_LAUNCH(KID_DIS, ingest_kernel_generic<DT>, dim3(grid), dim3(256), 0, st, x, prev, out, T, N, C, dis);
        RTK_LAUNCH_CHECK("ingest_kernel_generic");
        return RTK_OK;
    }
    dprow_with_vpl(vpl, [&](auto vc) {
        constexpr int V = decltype(vc)::value;
        static int resident = 0;   // waves of this instantiation the chip holds at once
        if (!resident) resident = dprow_resident_waves(ingest_kernel<DT, V>);
        const int strip = dprow_strip_rows(T, N, (size_t)resident);
        const size_t waves = (size_t)N * ((T + strip - 1) / strip);
        const unsigned grid = (unsigned)((waves * WAVE + 255) / 256);
        RTK_LAUNCH(KID_DIS, (ingest_kernel<DT, V>), dim3(grid), dim3(256), 0, st, (const vec_t*)x, (const vec_t*)prev,
                   (vec_t*)out, T, N, nvec, strip, dis);
    });
    RTK_LAUNCH_CHECK("ingest_kernel");
    return RTK_OK;
}

extern "C" int rtk_dpselect_ingest(const void* x, const void* prev, int t, int N, int C, int dtype, void* frames_out,
                                   float* dis_out, rtk_stream_t stream) {
    RTK_CHECK_ARG(x && frames_out && dis_out, "rtk_dpselect_ingest: NULL pointer");
    RTK_CHECK_ARG(t >= 1 && N >= 1 && C >= 1, "rtk_dpselect_ingest: bad shape t=%d N=%d C=%d", t, N, C);
    int es, ve;
    if (!payload_dims(dtype, es, ve)) {
        set_error("rtk_dpselect_ingest: unsupported dtype %d", dtype);
        return RTK_EINVAL;
    }
    const size_t row = (size_t)N * C * es, bytes = (size_t)t * row;
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)frames_out, pa = (uintptr_t)prev;
    RTK_CHECK_ARG(xa + bytes <= oa || oa + bytes <= xa, "rtk_dpselect_ingest: frames_out overlaps x");
    RTK_CHECK_ARG(!prev || pa + row <= oa || oa + bytes <= pa, "rtk_dpselect_ingest: prev lies inside the rows being written");
    hipStream_t st = (hipStream_t)stream;
    return with_payload(dtype, [&](auto dt) { return launch_ingest<decltype(dt)::value>(x, prev, t, N, C, frames_out, dis_out, st); });
}

extern "C" int rtk_dpselect_select_ring(const float* dis_ring, int R, int N, int r0, int len, int left, int right, int keep,
                                        int window, int sync, int64_t* idx, uint8_t* mask, float* keys,
                                        rtk_stream_t stream) {
    RTK_CHECK_ARG(dis_ring && idx && mask && keys, "rtk_dpselect_select_ring: NULL pointer");
    RTK_CHECK_ARG(R >= 1 && N >= 1 && window >= 1, "rtk_dpselect_select_ring: bad shape R=%d N=%d window=%d", R, N, window);
    RTK_CHECK_ARG(r0 >= 0 && r0 < R && len >= 1, "rtk_dpselect_select_ring: segment r0=%d len=%d outside a ring of %d rows", r0,
                  len, R);
    RTK_CHECK_ARG(left >= 0 && left <= window / 2 && right >= 0 && right <= window - 1 - window / 2,
                  "rtk_dpselect_select_ring: halo left=%d right=%d outside a window of %d", left, right, window);
    RTK_CHECK_ARG((long long)len + left + right <= R, "rtk_dpselect_select_ring: len + left + right = %lld rows exceed the ring's %d",
                  (long long)len + left + right, R);
    RTK_CHECK_ARG(keep >= 1 && keep <= len, "rtk_dpselect_select_ring: keep %d out of range [1,%d]", keep, len);
    if (!sync && N == 1) {
        set_error("rtk_dpselect_select_ring: async mode with N == 1: the reference raises IndexError (visual_compression.py:153-156)");
        return RTK_EREFCRASH;
    }
    RTK_LAUNCH(KID_DPSEL, dpselect_select_ring_kernel, dim3(sync ? 1 : N), dim3(SEL_BLOCK), 0, (hipStream_t)stream, dis_ring, R, N,
               r0, len, left, right, keep, window, sync, idx, mask, keys);
    RTK_LAUNCH_CHECK("dpselect_select_ring_kernel");
    return RTK_OK;
}

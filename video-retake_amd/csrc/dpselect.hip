// dpselect.hip — DPSelect on gfx950: adjacent-frame cosine distance, peak stencil + exact top-k,
// frame gather.  Replaces retake/visual_compression.py:100-175.
//
// Roofline: HBM-bound.  The distance kernel reads every (frame, patch) embedding row exactly once
// (plus one halo row per strip) — algorithmic bytes T*N*C*sizeof(elem) + 4*T*N — with 16-byte
// coalesced loads, keeps the previous frame's normalised row in registers, and reduces with wave
// shuffles.  The gather moves 2*t*N*C*sizeof(elem).  MFMA is not used: ~1 flop per byte.
#include "common.cuh"
#include "dprow.cuh"
#include "select.cuh"

namespace rtk {

// ------------------------------------------------------------------------------------------------
// K1-K2: distance.  One wave walks `strip` consecutive frames of one patch position.
// ------------------------------------------------------------------------------------------------
// VPL = 16-byte vectors per lane; a row has nvec = C / PER_VEC vectors, lane owns vec k*64+lane.  One wave walks
// `strip` (<= 64) consecutive frames of one patch position; the strip's results stay in a register (lane i holds
// row i) and are stored once at the end, and every load in the loop is unconditional (clamped addresses) so that
// the two rows in flight are tracked with counted waits rather than a full drain.
template <int DT, int VPL>
__global__ __launch_bounds__(256) void dis_kernel(const typename Elem<DT>::vec_t* __restrict__ x, int T, int N,
                                                  int nvec, int strip, int emit_cos, float* __restrict__ dis) {
    using E = Elem<DT>;
    using vec_t = typename E::vec_t;
    constexpr int NE = VPL * E::PER_VEC;
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

    vec_t rawA[VPL], rawB[VPL];   // two rows in flight per wave
    float nA[NE], nB[NE];         // normalised rows: odd steps in nA, even steps in nB (no copies between steps)

    // rows beyond the strip are clamped to its last row (a harmless re-read of a line that is in flight anyway)
    auto load_row = [&](vec_t* raw, int t) { dprow_load<DT, VPL>(raw, xrow + (size_t)min(t, t1 - 1) * frame_vecs, nvec, lane); };
    // normalise the row held in raw[] into cur[] (x / max(||x||, eps)), the reference's rounding per dtype (dprow.cuh)
    auto normalise = [&](vec_t* raw, float* cur) { dprow_normalise<DT, VPL>(raw, cur, nvec, lane); };
    const int tb = (t0 == 0) ? 1 : t0;   // first row this wave produces a distance for
    float res = 1.0f;                    // lane i: result of row tb + i (or of row 0 for the lane that gets it)
    // cos / distance of row t (in cur[]) against the previous row (prevn[])
    auto emit = [&](int t, const float* prevn, const float* cur) {
        const float dot = dprow_dot<DT, VPL>(prevn, cur);
        if (lane == t - tb) res = emit_cos ? dot : 1.0f - dot;
    };

    load_row(rawA, t0 == 0 ? 0 : t0 - 1);   // first row, or the halo row of the previous strip
    load_row(rawB, tb);
    normalise(rawA, nA);
    load_row(rawA, tb + 1);
    // rows tb, tb+2, ... go through rawB -> nB, rows tb+1, tb+3, ... through rawA -> nA; a raw buffer is
    // re-issued (two rows ahead) as soon as its row has been unpacked
    int t = tb;
    for (; t + 1 < t1; t += 2) {   // whole pairs only: the loads outstanding at the loop head are always B then A
        normalise(rawB, nB);
        load_row(rawB, t + 2);
        emit(t, nA, nB);
        normalise(rawA, nA);
        load_row(rawA, t + 3);
        emit(t + 1, nB, nA);
    }
    if (t < t1) {
        normalise(rawB, nB);
        emit(t, nA, nB);
    }
    // one store per produced row: MA-LLM keeps the similarity itself in [T-1, N]; DPSelect keeps 1 - cos in
    // [T, N] with torch.ones_like(dis[:1]) for frame 0   (visual_compression.py:103-106)
    const int tr = tb + lane;
    if (tr < t1) dis[(size_t)(emit_cos ? tr - 1 : tr) * N + n] = res;
    if (t0 == 0 && lane == 0 && !emit_cos) dis[n] = 1.0f;
}

// Generic fallback: any C (scalar loads, two passes over each row through L2).  One wave per (t,n).
template <int DT>
__global__ __launch_bounds__(256) void dis_kernel_generic(const void* __restrict__ xv, int T, int N, int C,
                                                          int emit_cos, float* __restrict__ dis) {
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (wave >= (size_t)T * N) return;
    const int t = (int)(wave / N), n = (int)(wave % N);
    if (t == 0) {
        if (lane == 0 && !emit_cos) dis[n] = 1.0f;
        return;
    }
    const float dot = dprow_pair_cos_generic<DT>(xv, ((size_t)(t - 1) * N + n) * C, xv, ((size_t)t * N + n) * C, C, lane);
    if (lane == 0) {
        if (emit_cos) dis[(size_t)(t - 1) * N + n] = dot;
        else dis[(size_t)t * N + n] = 1.0f - dot;
    }
}

// ------------------------------------------------------------------------------------------------
// K3-K7, K9: per-row peak stencil + bonus + exact top-k + ordered emit.  One workgroup per row
// (sync: the single patch-mean row; async: one row per patch position).
// ------------------------------------------------------------------------------------------------
// The body is select.cuh's dpselect_row, shared with the segment selection of a stream (dpselect_stream.hip): a whole
// video is a run of T frames with no halo.

__global__ __launch_bounds__(SEL_BLOCK) void dpselect_select_kernel(const float* __restrict__ dis, int T, int N,
                                                                    int tgt, int window, int sync,
                                                                    int64_t* __restrict__ idx,
                                                                    uint8_t* __restrict__ mask,
                                                                    float* __restrict__ keys) {
    __shared__ SelectSmem sm;
    const int row = blockIdx.x;  // patch index in async mode, 0 in sync mode
    // keys: async [N, T]; sync [2, T], row 1 the patch-mean distance
    dpselect_row<SEL_BLOCK>([&](int t) { return dis + (size_t)t * N; }, N, row, T, 0, 0, tgt, window, sync, idx, mask,
                            keys + (size_t)row * T, keys + (size_t)T, sm);
}

// ------------------------------------------------------------------------------------------------
// K8: frame gather.  One wave per output row (t', n); 16-byte vectors, loads batched before stores.
// ------------------------------------------------------------------------------------------------
template <int UNROLL>
__global__ __launch_bounds__(256) void gather_rows16_kernel(const u32x4* __restrict__ x, int T, int N, int rowvec,
                                                            const int64_t* __restrict__ idx, int tgt, int sync,
                                                            u32x4* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t nw = ((size_t)gridDim.x * blockDim.x) / WAVE;
    const size_t rows = (size_t)tgt * N;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; r < rows; r += nw) {
        const int tt = (int)(r / N), n = (int)(r % N);
        const int64_t f = sync ? idx[tt] : idx[r];
        const u32x4* src = x + ((size_t)f * N + n) * rowvec;
        u32x4* dst = out + r * rowvec;
        for (int v0 = 0; v0 < rowvec; v0 += UNROLL * WAVE) {
            u32x4 buf[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int v = v0 + u * WAVE + lane;
                if (v < rowvec) buf[u] = src[v];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int v = v0 + u * WAVE + lane;
                if (v < rowvec) dst[v] = buf[u];
            }
        }
    }
}

__global__ __launch_bounds__(256) void gather_rows_bytes_kernel(const uint8_t* __restrict__ x, int T, int N,
                                                                size_t rowbytes, const int64_t* __restrict__ idx,
                                                                int tgt, int sync, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t nw = ((size_t)gridDim.x * blockDim.x) / WAVE;
    const size_t rows = (size_t)tgt * N;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; r < rows; r += nw) {
        const int tt = (int)(r / N), n = (int)(r % N);
        const int64_t f = sync ? idx[tt] : idx[r];
        const uint8_t* src = x + ((size_t)f * N + n) * rowbytes;
        uint8_t* dst = out + r * rowbytes;
        for (size_t b = lane; b < rowbytes; b += WAVE) dst[b] = src[b];
    }
}

// ------------------------------------------------------------------------------------------------
// MA-LLM / MA-LLM-hard (visual_compression.py:5-83): one merge step = adjacent cosine (dis_kernel in
// cosine mode) -> arg-max frame pair per patch position -> merge + shift into a [T-1,N,C] bank.
// ------------------------------------------------------------------------------------------------
// The order of torch.max(dim) over similarities (:24 / :67): the maximum wins, NaN counts as the maximum (a zero fp16
// row gives 0 / 0), and among equals - several NaNs included - the lowest index wins.  Does (v2, i2) come before (v, i)?
// An empty candidate is (-inf, INT_MAX): every entry comes before it, it comes before none.
__device__ __forceinline__ bool sim_beats(float v2, int i2, float v, int i) {
    const bool n2 = v2 != v2, n = v != v;
    if (n2 != n) return n2;
    return (n2 || v2 == v) ? i2 < i : v2 > v;
}

// idx[n] = first arg-max over t of sim[t,n] in that order; sync: of the patch-mean row, the same for every n (:20-24)
__global__ __launch_bounds__(256) void mallm_argmax_kernel(const float* __restrict__ cosv, int T1, int N, int sync,
                                                           int round_bf16, int64_t* __restrict__ idx) {
    extern __shared__ float mrow[];  // sync: [T1] patch means
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int n = blockIdx.x;
    if (sync) {
        for (int t = wid; t < T1; t += 4) {  // similarity_matrix.mean(-1): fp32 accumulate, one rounding
            float s = 0.f;
            for (int j = lane; j < N; j += WAVE) s += cosv[(size_t)t * N + j];
            s = wave_sum(s);
            if (lane == 0) {
                float m = s / (float)N;
                mrow[t] = round_to(m, round_bf16);   // 0 = fp32, 1 = bf16, 2 = fp16 (the bank's dtype)
            }
        }
        __syncthreads();
    }
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int t = tid; t < T1; t += 256) {
        const float v = sync ? mrow[t] : cosv[(size_t)t * N + n];
        if (sim_beats(v, t, best, bidx)) {
            best = v;
            bidx = t;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, WAVE);
        const int i2 = __shfl_xor(bidx, o, WAVE);
        if (sim_beats(v2, i2, best, bidx)) {
            best = v2;
            bidx = i2;
        }
    }
    if (lane == 0) { bv[wid] = best; bi[wid] = bidx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (sim_beats(bv[w], bi[w], bv[0], bi[0])) {
                bv[0] = bv[w];
                bi[0] = bi[w];
            }
        if (sync) for (int j = 0; j < N; ++j) idx[j] = bi[0];
        else idx[n] = bi[0];
    }
}

// out[t,n,:] for the T-1 output frames; one thread per element (the op is a streaming copy with at most two
// source rows per output row).  Soft merge keeps the reference's op order and roundings (:35-45):
//   (x[d]*s[d]) / s[d]   and at the merged slot   ((x[i]*s[i]) + (x[i+1]*s[i+1])) / (s[i] + s[i+1])
template <int DT>
__global__ __launch_bounds__(256) void mallm_merge_kernel(const void* __restrict__ xv, const void* __restrict__ sv,
                                                          const int64_t* __restrict__ idx, int T, int N, int C, int hard,
                                                          void* __restrict__ outv, void* __restrict__ sov) {
    const size_t total = (size_t)(T - 1) * N * C;
    auto ldx = [&](size_t i) -> float {
        if constexpr (DT != RTK_F32) return H16<DT>::ld(xv, i);
        else return ((const float*)xv)[i];
    };
    auto lds = [&](size_t i) -> float {
        if constexpr (DT != RTK_F32) return H16<DT>::ld(sv, i);
        else return ((const float*)sv)[i];
    };
    auto rnd = [&](float v) -> float {
        if constexpr (DT != RTK_F32) return H16<DT>::rnd(v);
        else return v;
    };
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const size_t tn = e / C;
        const int n = (int)(tn % N), t = (int)(tn / N);
        const int ix = (int)idx[n];
        float o;
        if (hard) {
            const int d = t + (t >= ix);
            if (DT != RTK_F32) ((uint16_t*)outv)[e] = ((const uint16_t*)xv)[((size_t)d * N + n) * C + c];
            else ((float*)outv)[e] = ((const float*)xv)[((size_t)d * N + n) * C + c];
            continue;
        }
        const int d = t + (t > ix);
        const float sd = lds((size_t)d * N + n);
        const float xd = ldx(((size_t)d * N + n) * C + c);
        float den = sd;
        if (t != ix) {
            o = rnd(__fdiv_rn(rnd(__fmul_rn(xd, sd)), sd));
        } else {
            const float ss = lds((size_t)(ix + 1) * N + n);
            const float xs = ldx(((size_t)(ix + 1) * N + n) * C + c);
            den = rnd(__fadd_rn(sd, ss));
            o = rnd(__fdiv_rn(rnd(__fadd_rn(rnd(__fmul_rn(xd, sd)), rnd(__fmul_rn(xs, ss)))), den));
        }
        if constexpr (DT != RTK_F32) H16<DT>::st(outv, e, o);
        else ((float*)outv)[e] = o;
        if (c == 0) {
            if constexpr (DT != RTK_F32) H16<DT>::st(sov, tn, den);
            else ((float*)sov)[tn] = den;
        }
    }
}

}  // namespace rtk

using namespace rtk;

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
template <int DT>
static int launch_dis(const void* x, int T, int N, int C, int emit_cos, float* dis, hipStream_t st) {
    constexpr int PV = Elem<DT>::PER_VEC;
    using vec_t = typename Elem<DT>::vec_t;
    const bool vec_ok = (C % PV == 0) && (((uintptr_t)x & 15) == 0);
    const int nvec = C / PV;
    const int vpl = (nvec + WAVE - 1) / WAVE;
    if (!vec_ok || vpl > 16) {
        const size_t waves = (size_t)T * N;
        const unsigned grid = (unsigned)((waves * WAVE + 255) / 256);
        RTK_LAUNCH(KID_DIS, dis_kernel_generic<DT>, dim3(grid), dim3(256), 0, st, x, T, N, C, emit_cos, dis);
        RTK_LAUNCH_CHECK("dis_kernel_generic");
        return RTK_OK;
    }
    // strips sized so that the whole job is one resident set of waves (dprow_strip_rows)
    const vec_t* xv = (const vec_t*)x;
    dprow_with_vpl(vpl, [&](auto vc) {
        constexpr int V = decltype(vc)::value;
        static int resident = 0;   // waves of this instantiation the chip holds at once
        if (!resident) resident = dprow_resident_waves(dis_kernel<DT, V>);
        const int strip = dprow_strip_rows(T, N, (size_t)resident);
        const size_t waves = (size_t)N * ((T + strip - 1) / strip);
        const unsigned grid = (unsigned)((waves * WAVE + 255) / 256);
        RTK_LAUNCH(KID_DIS, (dis_kernel<DT, V>), dim3(grid), dim3(256), 0, st, xv, T, N, nvec, strip, emit_cos, dis);
    });
    RTK_LAUNCH_CHECK("dis_kernel");
    return RTK_OK;
}

extern "C" int rtk_dpselect_dis(const void* x, int T, int N, int C, int dtype, float* dis, rtk_stream_t stream) {
    RTK_CHECK_ARG(x && dis, "rtk_dpselect_dis: NULL pointer");
    RTK_CHECK_ARG(T >= 1 && N >= 1 && C >= 1, "rtk_dpselect_dis: bad shape T=%d N=%d C=%d", T, N, C);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RTK_F32) return launch_dis<RTK_F32>(x, T, N, C, 0, dis, st);
    if (dtype == RTK_BF16) return launch_dis<RTK_BF16>(x, T, N, C, 0, dis, st);
    if (dtype == RTK_F16) return launch_dis<RTK_F16>(x, T, N, C, 0, dis, st);
    set_error("rtk_dpselect_dis: unsupported dtype %d", dtype);
    return RTK_EINVAL;
}

extern "C" int rtk_adjacent_cosine(const void* x, int T, int N, int C, int dtype, float* cos_out, rtk_stream_t stream) {
    RTK_CHECK_ARG(x && cos_out, "rtk_adjacent_cosine: NULL pointer");
    RTK_CHECK_ARG(T >= 2 && N >= 1 && C >= 1, "rtk_adjacent_cosine: bad shape T=%d N=%d C=%d", T, N, C);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RTK_F32) return launch_dis<RTK_F32>(x, T, N, C, 1, cos_out, st);
    if (dtype == RTK_BF16) return launch_dis<RTK_BF16>(x, T, N, C, 1, cos_out, st);
    if (dtype == RTK_F16) return launch_dis<RTK_F16>(x, T, N, C, 1, cos_out, st);
    set_error("rtk_adjacent_cosine: unsupported dtype %d", dtype);
    return RTK_EINVAL;
}

extern "C" int rtk_mallm_argmax(const float* cosv, int T1, int N, int sync, int round_bf16, int64_t* idx,
                                rtk_stream_t stream) {
    RTK_CHECK_ARG(cosv && idx, "rtk_mallm_argmax: NULL pointer");
    RTK_CHECK_ARG(T1 >= 1 && N >= 1, "rtk_mallm_argmax: bad shape T1=%d N=%d", T1, N);
    const size_t lds = sync ? (size_t)T1 * sizeof(float) : 0;
    if (lds > 64 * 1024) {
        set_error("rtk_mallm_argmax: %d frames exceed the sync path's LDS row", T1);
        return RTK_EUNSUPPORTED;
    }
    RTK_LAUNCH(KID_DPSEL, mallm_argmax_kernel, dim3(sync ? 1 : N), dim3(256), lds, (hipStream_t)stream, cosv, T1, N, sync,
               round_bf16, idx);
    RTK_LAUNCH_CHECK("mallm_argmax_kernel");
    return RTK_OK;
}

extern "C" int rtk_mallm_merge(const void* x, const void* sizes, const int64_t* idx, int T, int N, int C, int dtype,
                               int hard, void* out, void* sizes_out, rtk_stream_t stream) {
    RTK_CHECK_ARG(x && idx && out, "rtk_mallm_merge: NULL pointer");
    RTK_CHECK_ARG(hard || (sizes && sizes_out), "rtk_mallm_merge: the soft merge needs sizes and sizes_out");
    RTK_CHECK_ARG(T >= 2 && N >= 1 && C >= 1, "rtk_mallm_merge: bad shape T=%d N=%d C=%d", T, N, C);
    RTK_CHECK_ARG(dtype == RTK_F32 || dtype == RTK_BF16 || dtype == RTK_F16, "rtk_mallm_merge: unsupported dtype %d", dtype);
    const size_t total = (size_t)(T - 1) * N * C;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65535u * 16u);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RTK_BF16)
        RTK_LAUNCH(KID_GATHER, mallm_merge_kernel<RTK_BF16>, dim3(grid), dim3(256), 0, st, x, sizes, idx, T, N, C, hard, out,
                   sizes_out);
    else if (dtype == RTK_F16)
        RTK_LAUNCH(KID_GATHER, mallm_merge_kernel<RTK_F16>, dim3(grid), dim3(256), 0, st, x, sizes, idx, T, N, C, hard, out,
                   sizes_out);
    else
        RTK_LAUNCH(KID_GATHER, mallm_merge_kernel<RTK_F32>, dim3(grid), dim3(256), 0, st, x, sizes, idx, T, N, C, hard, out,
                   sizes_out);
    RTK_LAUNCH_CHECK("mallm_merge_kernel");
    return RTK_OK;
}

extern "C" int rtk_dpselect_select(const float* dis, int T, int N, int tgt, int window, int sync, int64_t* idx,
                                   uint8_t* mask, float* keys, rtk_stream_t stream) {
    RTK_CHECK_ARG(dis && idx && mask && keys, "rtk_dpselect_select: NULL pointer");
    RTK_CHECK_ARG(T >= 1 && N >= 1 && window >= 1, "rtk_dpselect_select: bad shape T=%d N=%d window=%d", T, N, window);
    RTK_CHECK_ARG(tgt >= 1 && tgt <= T, "rtk_dpselect_select: tgt_mem_len %d out of range [1,%d]", tgt, T);
    if (!sync && N == 1) {
        set_error("DPSelect async mode with N == 1: the reference raises IndexError (visual_compression.py:153-156)");
        return RTK_EREFCRASH;
    }
    RTK_LAUNCH(KID_DPSEL, dpselect_select_kernel, dim3(sync ? 1 : N), dim3(SEL_BLOCK), 0, (hipStream_t)stream, dis, T, N,
                       tgt, window, sync, idx, mask, keys);
    RTK_LAUNCH_CHECK("dpselect_select_kernel");
    return RTK_OK;
}

extern "C" int rtk_gather_frames(const void* x, int T, int N, int C, int dtype, const int64_t* idx, int tgt, int sync,
                                 void* out, rtk_stream_t stream) {
    RTK_CHECK_ARG(x && idx && out, "rtk_gather_frames: NULL pointer");
    RTK_CHECK_ARG(T >= 1 && N >= 1 && C >= 1 && tgt >= 1, "rtk_gather_frames: bad shape");
    RTK_CHECK_ARG(dtype == RTK_F32 || dtype == RTK_BF16 || dtype == RTK_F16, "rtk_gather_frames: unsupported dtype %d", dtype);
    const size_t esize = dtype == RTK_F32 ? 4 : 2;
    const size_t rowbytes = (size_t)C * esize;
    const size_t rows = (size_t)tgt * N;
    const unsigned grid = (unsigned)std::min<size_t>((rows + 3) / 4, 8192);
    hipStream_t st = (hipStream_t)stream;
    if (rowbytes % 16 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0) {
        RTK_LAUNCH(KID_GATHER, gather_rows16_kernel<4>, dim3(grid), dim3(256), 0, st, (const u32x4*)x, T, N,
                           (int)(rowbytes / 16), idx, tgt, sync, (u32x4*)out);
    } else {
        RTK_LAUNCH(KID_GATHER, gather_rows_bytes_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t*)x, T, N, rowbytes,
                           idx, tgt, sync, (uint8_t*)out);
    }
    RTK_LAUNCH_CHECK("gather_rows_kernel");
    return RTK_OK;
}

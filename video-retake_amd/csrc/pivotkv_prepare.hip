// pivotkv_prepare.hip — the kernels that turn a chunk's rotated q, k (and v) into what the PivotKV scoring and the cache
// need: the un-rotated, packed operands q~ [Hq,L,D] and k~ [Hkv,L,D] of the score passes (pos_embed_reforge,
// longvideo_cache.py:76-78: ((x*cos) - (rotate_half(x)*sin)) / a^2, one rounding per torch op), written into the score
// workspace (score_layout.cuh).
//   unrotate_pack_vec_kernel / unrotate_pack_kernel   from cos / sin tables: the RTK_SCORE_PREPARE stage of
//                                                     rtk_pivotkv_score (score_unrotate)
//   prepare_native_kernel   the per-update form (rtk_pivotkv_prepare, rtk_pivotkv_update): tables built in registers
//                           from the position ids, k and v appended to the cache tail in the same pass, and optionally
//                           the next layer's continuity shift of the ids riding in the launch
// The un-rotation itself is written once, in common.cuh (unrotate_words), for these kernels and the attention prologue
// (pivotkv_update.hip); only the scalar fallback below spells it per element.
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "score_layout.cuh"

namespace rtk {

// ------------------------------------------------------------------------------------------------
// un-rotate + pack:  q [Hq,L,D] and k [Hkv,L,D] (strided) -> contiguous [H,L,D] copies (same dtype)
//   cos == NULL: plain copy;  else ((x*cos) - (rotate_half(x)*sin)) / a^2  with one rounding per
//   torch op (bf16: every intermediate is a bf16 tensor; fp32: no fma contraction).
// One thread owns a 16-byte chunk of the first half of a token row plus its rotation partner in the
// second half, keeps that token's cos/sin in registers and walks UNROT_HEADS heads with it.
// ------------------------------------------------------------------------------------------------
constexpr int UNROT_HEADS = 7;

// DIV: 0 = no division (attention_scaling^2 == 1), 1 = multiply by the reciprocal (bf16 only, the host has
// verified EXHAUSTIVELY over all 65536 bf16 inputs that bf16(x * rcp) == bf16(x / a2) for this a2), 2 = IEEE
// FAST (RTK_BF16_FAST, bf16 inputs only): q~ is stored as fp16(q~ * qscale) and k~ additionally as fp16 in k_fast (the
// bf16 k~ in k_out - what the eviction re-rotates - is skipped when k_out is NULL).
template <int DT, int DIV, bool FAST = false>
__global__ __launch_bounds__(256) void unrotate_pack_vec_kernel(const char* __restrict__ q, int64_t q_sh, int64_t q_sl,
                                                                const char* __restrict__ k, int64_t k_sh, int64_t k_sl,
                                                                int Hq, int Hkv, int L, int D,
                                                                const float* __restrict__ cosv,
                                                                const float* __restrict__ sinv, float a2, float rcp_a2,
                                                                char* __restrict__ q_out, char* __restrict__ k_out,
                                                                char* __restrict__ k_fast = nullptr, float qscale = 1.f) {
    using V = Vec16<DT>;
    constexpr int VE = V::VE;
    constexpr int ES = 16 / VE;
    const int h2 = D / 2, lpr = h2 / VE;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= L * lpr) return;
    const int l = id / lpr, d = (id - l * lpr) * VE;
    // blockIdx.y walks head groups: first the q groups, then the k groups
    const int qgroups = (Hq + UNROT_HEADS - 1) / UNROT_HEADS;
    const bool is_q = (int)blockIdx.y < qgroups;
    const int hg = is_q ? blockIdx.y : blockIdx.y - qgroups;
    const int H = is_q ? Hq : Hkv;
    const char* src = is_q ? q : k;
    char* dst = is_q ? q_out : k_out;
    const int64_t sh = is_q ? q_sh : k_sh, sl = is_q ? q_sl : k_sl;
    float c1[VE], s1[VE], c2[VE], s2[VE];
    if (cosv) {
#pragma unroll
        for (int e = 0; e < VE; e += 4) {
            *(float4*)(c1 + e) = *(const float4*)(cosv + (size_t)l * D + d + e);
            *(float4*)(s1 + e) = *(const float4*)(sinv + (size_t)l * D + d + e);
            *(float4*)(c2 + e) = *(const float4*)(cosv + (size_t)l * D + d + h2 + e);
            *(float4*)(s2 + e) = *(const float4*)(sinv + (size_t)l * D + d + h2 + e);
        }
    }
    const int hb = hg * UNROT_HEADS;
    // all loads first (UNROT_HEADS independent row pairs in flight), then the arithmetic and the stores
    u32x4 lo[UNROT_HEADS], hi[UNROT_HEADS];
#pragma unroll
    for (int u = 0; u < UNROT_HEADS; ++u) {
        const int h = min(hb + u, H - 1);
        const char* row = src + ((size_t)h * sh + (size_t)l * sl) * ES;
        lo[u] = *(const u32x4*)(row + (size_t)d * ES);
        hi[u] = *(const u32x4*)(row + (size_t)(d + h2) * ES);
    }
#pragma unroll
    for (int u = 0; u < UNROT_HEADS; ++u) {
        const int h = hb + u;
        if (h >= H) break;
        char* orow = dst + ((size_t)h * L + l) * D * ES;
        // FAST: where the un-rotated chunk pair (bf16 values) goes - q as scaled fp16, k as bf16 (if wanted) + fp16
        auto store_fast = [&](const u32x4& a, const u32x4& b) {
            if (is_q) {
                *(u32x4*)(orow + (size_t)d * ES) = bf16x8_to_f16x8(a, qscale);
                *(u32x4*)(orow + (size_t)(d + h2) * ES) = bf16x8_to_f16x8(b, qscale);
            } else {
                if (dst) {
                    *(u32x4*)(orow + (size_t)d * ES) = a;
                    *(u32x4*)(orow + (size_t)(d + h2) * ES) = b;
                }
                char* frow = k_fast + ((size_t)h * L + l) * D * ES;
                *(u32x4*)(frow + (size_t)d * ES) = bf16x8_to_f16x8(a, 1.f);
                *(u32x4*)(frow + (size_t)(d + h2) * ES) = bf16x8_to_f16x8(b, 1.f);
            }
        };
        if (!cosv) {
            if constexpr (FAST) { store_fast(lo[u], hi[u]); continue; }
            *(u32x4*)(orow + (size_t)d * ES) = lo[u];
            *(u32x4*)(orow + (size_t)(d + h2) * ES) = hi[u];
            continue;
        }
        // x~ = ((x*cos) - (rotate_half(x)*sin)) / a^2, one rounding per torch op (:76-78): unrotate_words on the chunk pair
        WV<4> r1, r2;
        unrotate_words<DT, 4>(WV<4>{{lo[u].x, lo[u].y, lo[u].z, lo[u].w}}, WV<4>{{hi[u].x, hi[u].y, hi[u].z, hi[u].w}}, c1, s1, c2,
                              s2, a2, rcp_a2, std::integral_constant<int, DIV>{}, r1, r2);
        const u32x4 o1 = {r1.w[0], r1.w[1], r1.w[2], r1.w[3]}, o2 = {r2.w[0], r2.w[1], r2.w[2], r2.w[3]};
        if constexpr (FAST) {
            store_fast(o1, o2);
        } else {
            *(u32x4*)(orow + (size_t)d * ES) = o1;
            *(u32x4*)(orow + (size_t)(d + h2) * ES) = o2;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Fused prepare (native RoPE tables only): one pass over the chunk's q, k, v that
//   builds the token's cos/sin chunk in registers (what rope_table_kernel writes to HBM: same sincos_cr, same
//   scaling, same bf16 rounding), un-rotates q and k with it (same arithmetic as unrotate_pack_vec_kernel),
//   and appends k and v to the cache tail (what append_kernel does) — k is read once instead of twice and
//   three launches become one.  One thread = one token x one 16-byte chunk pair; blockIdx.y splits the heads
//   in two: y = 0 the first half of the q heads + k (k~ and the k tail), y = 1 the second half + the v tail.
// ------------------------------------------------------------------------------------------------
// NW = 32-bit words per thread and row half: 4 (16-byte accesses; fp32) or, for the 16-bit dtypes, PREP_NW = 1.  A
// wave of the 16-byte form issues ~3500 VALU instructions (the per-op rounding chains of 18 heads plus 8 correctly
// rounded sin / cos pairs) and a chunk of 2304 tokens gives barely half the chip's SIMDs one such wave: that form is bound
// by the serial instruction stream of its waves.  Narrow chunks split the same work over 4x the waves; what remains is the
// read + write traffic (45 MB per call at L = 2304) at ~3 TB/s plus the launch ramp.

constexpr int RTK_SHIFT_COUNTERS = 64;   // arrival counters of RTK_UPDATE_SHIFT_NEXT (<= PREP_BLOCK: one per watching thread)
constexpr int RTK_SHIFT_STRIDE = 32;     // ... 128 bytes apart
constexpr int RTK_SHIFT_STATUS = RTK_SHIFT_STRIDE - 1;     // word of the first line that latches a wait that ran out
// polls of the watching workgroup before it gives up (an agent-scope load, a barrier and s_sleep 4 per poll: ~2-3 s; the
// workers need microseconds).  Same policy as compact_units_kernel's bounded wait, but latched instead of trapped: the
// host can raise, reset and carry on, and the test suite can force it.
constexpr unsigned RTK_SHIFT_MAX_POLLS = 1u << 21;
static_assert(RTK_SHIFT_COUNTERS <= PREP_BLOCK, "one watching thread per counter");

template <int DT, int DIV, bool FAST = false, int NW = 4>
__global__ __launch_bounds__(PREP_BLOCK) void prepare_native_kernel(const char* __restrict__ q, int64_t q_sh, int64_t q_sl,
                                                            const char* __restrict__ k, int64_t k_sh, int64_t k_sl,
                                                            const char* __restrict__ v, int64_t v_sh, int64_t v_sl,
                                                            int Hq, int Hkv, int L, int D,
                                                            const int64_t* pos, int64_t pos_ld,
                                                            const float* __restrict__ inv_freq, float scaling, RowSel rs,
                                                            int round_bf16, float a2, float rcp_a2,
                                                            char* __restrict__ q_out, char* __restrict__ k_out,
                                                            char* __restrict__ k_tail, char* __restrict__ v_tail,
                                                            int64_t tail_sh, int P, int64_t* __restrict__ pos_copy,
                                                            char* __restrict__ k_fast = nullptr, float qscale = 1.f,
                                                            int64_t* shift_row = nullptr, const int64_t* next_prev = nullptr,
                                                            int* ticket = nullptr, int* status = nullptr) {
    using V = Vec16<DT>;
    static_assert(NW == 4 || ((NW == 2 || NW == 1) && DT != RTK_F32), "8- / 4-byte chunks: 16-bit dtypes only");
    constexpr int ES = 16 / V::VE;          // bytes per element
    constexpr int VE = 4 * NW / ES;         // elements per thread and row half
    using W = WV<NW>;
    const int h2 = D / 2, lpr = h2 / VE;
    // RTK_UPDATE_SHIFT_NEXT: the NEXT layer's continuity shift (qwen2_vl.py:68-73) rides in this launch.  Every working
    // workgroup reads the chunk's ids, so the row may only be rewritten once all of them have.  Each adds one to one of
    // RTK_SHIFT_COUNTERS counters (own cache lines) once its ids are in registers - fire and forget, nobody waits; the
    // FIRST workgroup of the grid (an extra column) does no other work: it watches the counters reach the launch's totals,
    // zeroes them for the next launch, rewrites the row and counts the launch in ticket[0], beside the others' work.
    // The wait is bounded by a POLL count (polls only advance while this wave runs: a process that is switched out, a
    // debugger, a throttled clock cannot trip it - a wall-clock bound could).  If it ever runs out - the counters were
    // not zero at launch, i.e. the words were shared or not zeroed - NOTHING is shifted and NOTHING is zeroed: the watcher
    // latches ticket[RTK_SHIFT_STATUS] (and the host-visible *status, if given) and returns, and so does the watcher of
    // every later launch until the host has seen the latch and reset the words (PivotKVCache raises: the ids of the layers
    // after the failed launch were not shifted).  A row is only ever rewritten after every reader was counted in.
    const int bx = (int)blockIdx.x - (shift_row ? 1 : 0), gx = (int)gridDim.x - (shift_row ? 1 : 0);
    if (bx < 0) {
        if (blockIdx.y != 0) return;
        __shared__ int s_latched;
        if (threadIdx.x == 0)
            s_latched = __hip_atomic_load(ticket + RTK_SHIFT_STATUS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        __syncthreads();
        if (s_latched) return;   // an earlier launch's wait ran out: the counters are not trustworthy until the host resets them
        constexpr int E = 8;   // ids per thread and round, two rounds in flight
        const int nwork = gx * (int)gridDim.y, step = E * (int)blockDim.x;
        const long long delta = (next_prev ? (long long)next_prev[0] : -1ll) + 1 - (long long)shift_row[0];
        long long v[2][E];
        auto fetch = [&](long long* r, int base) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = base + e * (int)blockDim.x + (int)threadIdx.x;
                r[e] = i < L ? (long long)shift_row[i] : 0;
            }
        };
        fetch(v[0], 0);        // the first round of the row is on its way while the others start up
        // counter c takes the workgroups whose linear index is c modulo RTK_SHIFT_COUNTERS
        const int c = (int)threadIdx.x;   // (blockDim.x >= RTK_SHIFT_COUNTERS: one counter per thread)
        unsigned* mine = (unsigned*)ticket + RTK_SHIFT_STRIDE * (1 + c);
        const unsigned want = (unsigned)(nwork / RTK_SHIFT_COUNTERS + (c < nwork % RTK_SHIFT_COUNTERS ? 1 : 0));
        unsigned polls = 0;
        for (;;) {
            int ok = 1;
            if (c < RTK_SHIFT_COUNTERS) ok = __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want;
            if (__syncthreads_and(ok)) break;
            if (++polls > RTK_SHIFT_MAX_POLLS) {   // (uniform: every thread counts the same polls)
                if (threadIdx.x == 0) {
                    __hip_atomic_fetch_add(ticket + RTK_SHIFT_STATUS, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (status) {
                        __hip_atomic_fetch_add(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        __threadfence_system();
                    }
                }
                return;        // ids untouched, counters untouched
            }
            __builtin_amdgcn_s_sleep(4);
        }
        if (c < RTK_SHIFT_COUNTERS) __hip_atomic_store(mine, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (delta != 0) {      // t[0:L] += (prev_next + 1) - t[0]
            int cur = 0;
            for (int base = 0; base < L; base += step, cur ^= 1) {
                if (base + step < L) fetch(v[cur ^ 1], base + step);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = base + e * (int)blockDim.x + (int)threadIdx.x;
                    if (i < L) shift_row[i] = v[cur][e] + delta;
                }
            }
        }
        if (threadIdx.x == 0) ticket[0] += 1;   // launches that carried a shift (diagnostics)
        return;
    }
    const int id = bx * (int)blockDim.x + (int)threadIdx.x;
    if (id >= L * lpr) return;
    const int l = id / lpr, d = (id - l * lpr) * VE;
    if (pos_copy && blockIdx.y == 0 && d == 0)   // the ids the caller may shift in place before the deferred selection runs
        for (int p = 0; p < P; ++p) pos_copy[(size_t)p * L + l] = pos[(size_t)p * pos_ld + l];
    constexpr int HU = PREP_HU;   // heads per batch: all loads of a batch are issued before its arithmetic and stores
    const int ny = gridDim.y, qper = (Hq + ny - 1) / ny;
    const int qb = uniform_int(min((int)blockIdx.y * qper, Hq)), qe = uniform_int(min(qb + qper, Hq));   // (head loops in SGPRs)
    // the KV heads: y = 0 takes k (k~ for the scoring / eviction + the rotated rows for the tail), the last y takes v
    const bool has_kv = blockIdx.y == 0 || (int)blockIdx.y == ny - 1;
    const char* src = blockIdx.y == 0 ? k : v;
    const int64_t sh = blockIdx.y == 0 ? k_sh : v_sh, sl = blockIdx.y == 0 ? k_sl : v_sl;
    char* tail = blockIdx.y == 0 ? k_tail : v_tail;
    const int nkv = has_kv ? Hkv : 0;
    // Software pipeline over head batches: the rows of batch b+1 (after the last query batch: the first KV batch)
    // are requested before batch b is un-rotated and stored, and the first batch before the table arithmetic
    // (sin / cos are ~25 fp64 operations per value) - with ~1.5 waves per SIMD nothing else hides a round trip.
    W lo[HU], hi[HU], lon[HU], hin[HU];
    // a row's address = descriptor (tensor base) + soffset (the head: wave-uniform, a scalar multiply) + voffset (this
    // thread's byte offset inside a head, computed once); the launcher has checked that every extent fits 31 bits
    const uint32_t off_q = (uint32_t)(((int64_t)l * q_sl + d) * ES), off_kv = (uint32_t)(((int64_t)l * sl + d) * ES);
    const uint32_t off_o = (uint32_t)(((int64_t)l * D + d) * ES), half = (uint32_t)(h2 * ES);
    const uint32_t off_q2 = off_q + half, off_kv2 = off_kv + half, off_o2 = off_o + half;
    const __amdgpu_buffer_rsrc_t r_q = buf_rsrc(q), r_src = buf_rsrc(src), r_qo = buf_rsrc(q_out), r_ko = buf_rsrc(k_out),
                                 r_tail = buf_rsrc(tail), r_kf = buf_rsrc(k_fast);
    const uint32_t hs_q = (uint32_t)(q_sh * ES), hs_kv = (uint32_t)(sh * ES), hs_o = (uint32_t)((int64_t)L * D * ES),
                   hs_t = (uint32_t)(tail_sh * ES);
    auto load_q = [&](W* a, W* b, int hb) { load_heads<NW, HU>(a, b, r_q, off_q, off_q2, hs_q, hb, qe - 1); };
    auto load_kv = [&](W* a, W* b, int hb) { load_heads<NW, 4>(a, b, r_src, off_kv, off_kv2, hs_kv, hb, Hkv - 1); };
    float pid[3];   // the token's ids (t / h / w rows; a 1-D id fills all three)
#pragma unroll
    for (int p = 0; p < 3; ++p) pid[p] = (float)pos[(size_t)min(p, P - 1) * pos_ld + l];
    if (qb < qe) load_q(lo, hi, qb);
    else if (nkv) load_kv(lo, hi, 0);
    float c1[VE], s1[VE], c2[VE], s2[VE];
    rope_chunk<VE>(inv_freq, rs, d, h2, pid, scaling, round_bf16, c1, s1, c2, s2);
    if (shift_row) {   // (kernel argument: uniform)  this workgroup holds its ids: count it in (see the top of the kernel)
        __syncthreads();   // every wave is past rope_chunk (pid consumed) and past the pos_copy stores (their loads returned)
        if (threadIdx.x == 0)
            __hip_atomic_fetch_add((unsigned*)ticket + RTK_SHIFT_STRIDE * (1 + ((int)blockIdx.y * gx + bx) % RTK_SHIFT_COUNTERS),
                                   1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // x~ = ((x*cos) - (rotate_half(x)*sin)) / a^2 for one head's chunk pair, one rounding per torch op (:76-78)
    auto unrot = [&](const W& lo, const W& hi, W& olo, W& ohi) {
        unrotate_words<DT, NW>(lo, hi, c1, s1, c2, s2, a2, rcp_a2, std::integral_constant<int, DIV>{}, olo, ohi);
    };
    for (int hb = qb; hb < qe; hb += HU) {
        if (hb + HU < qe) load_q(lon, hin, hb + HU);
        else if (nkv) load_kv(lon, hin, 0);
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int h = hb + u;
            if (h >= qe) break;
            W olo, ohi;
            unrot(lo[u], hi[u], olo, ohi);
            if constexpr (FAST) {   // the score's A / B operand: fp16(q~ * log2(e)/sqrt(D))
                olo = bf16_to_f16_words<NW>(olo, qscale);
                ohi = bf16_to_f16_words<NW>(ohi, qscale);
            }
            const uint32_t so = head_soff(h, hs_o);
            buf_store<NW>(olo, r_qo, off_o, so);
            buf_store<NW>(ohi, r_qo, off_o2, so);
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            lo[u] = lon[u];
            hi[u] = hin[u];
        }
    }
    for (int hb = 0; hb < nkv; hb += 4) {
        if (hb + 4 < nkv) load_kv(lon, hin, hb + 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int h = hb + u;
            if (h >= nkv) break;
            const uint32_t sot = head_soff(h, hs_t);
            buf_store<NW>(lo[u], r_tail, off_o, sot);
            buf_store<NW>(hi[u], r_tail, off_o2, sot);
            if (blockIdx.y == 0) {
                W olo, ohi;
                unrot(lo[u], hi[u], olo, ohi);
                const uint32_t so = head_soff(h, hs_o);
                buf_store<NW>(olo, r_ko, off_o, so);
                buf_store<NW>(ohi, r_ko, off_o2, so);
                if constexpr (FAST) {   // the same k~ as fp16 for the score passes (exact re-encoding)
                    buf_store<NW>(bf16_to_f16_words<NW>(olo, 1.f), r_kf, off_o, so);
                    buf_store<NW>(bf16_to_f16_words<NW>(ohi, 1.f), r_kf, off_o2, so);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lo[u] = lon[u];
            hi[u] = hin[u];
        }
    }
}

// scalar fallback (any even head_dim, any alignment): one thread per channel pair, so there is no packed pair to round
// through - it keeps the per-element form of the same op chain (H16<DT>::rnd after every torch op) instead of unrotate_words
template <int DT>
__global__ __launch_bounds__(256) void unrotate_pack_kernel(const void* __restrict__ xv, int64_t stride_h,
                                                            int64_t stride_l, int H, int L, int D,
                                                            const float* __restrict__ cosv,
                                                            const float* __restrict__ sinv, float a2,
                                                            void* __restrict__ outv) {
    const int h2 = D / 2;
    const size_t total = (size_t)H * L * h2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % h2);
        const size_t hl = i / h2;
        const int l = (int)(hl % L);
        const int h = (int)(hl / L);
        const size_t src = (size_t)h * stride_h + (size_t)l * stride_l;
        const size_t dst = hl * D;
        float x1, x2;
        if constexpr (DT != RTK_F32) {
            x1 = H16<DT>::ld(xv, src + d);
            x2 = H16<DT>::ld(xv, src + d + h2);
        } else {
            x1 = ((const float*)xv)[src + d];
            x2 = ((const float*)xv)[src + d + h2];
        }
        float o1 = x1, o2 = x2;
        if (cosv) {
            const float c1 = cosv[(size_t)l * D + d], s1 = sinv[(size_t)l * D + d];
            const float c2 = cosv[(size_t)l * D + d + h2], s2 = sinv[(size_t)l * D + d + h2];
            if constexpr (DT != RTK_F32) {
                using Hh = H16<DT>;
                o1 = Hh::rnd(Hh::rnd(Hh::rnd(x1 * c1) - Hh::rnd(-x2 * s1)) / a2);
                o2 = Hh::rnd(Hh::rnd(Hh::rnd(x2 * c2) - Hh::rnd(x1 * s2)) / a2);
            } else {
                o1 = __fdiv_rn(__fsub_rn(__fmul_rn(x1, c1), __fmul_rn(-x2, s1)), a2);
                o2 = __fdiv_rn(__fsub_rn(__fmul_rn(x2, c2), __fmul_rn(x1, s2)), a2);
            }
        }
        if constexpr (DT != RTK_F32) {
            H16<DT>::st(outv, dst + d, o1);
            H16<DT>::st(outv, dst + d + h2, o2);
        } else {
            ((float*)outv)[dst + d] = o1;
            ((float*)outv)[dst + d + h2] = o2;
        }
    }
}

// bf16(x * (1/a2)) == bf16(x / a2) for EVERY finite bf16 x?  (x is bf16-valued in the un-rotate chain, so the
// check is exhaustive: 65536 cases, cached per a2.)  True for the YaRN factor-4 scaling 1.1386^2.
bool bf16_rcp_is_exact(float a2) {
    static std::mutex mu;
    static std::map<uint32_t, bool> cache;
    uint32_t key;
    memcpy(&key, &a2, 4);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    auto to_bf = [](float f) -> uint16_t {
        uint32_t u;
        memcpy(&u, &f, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    };
    const volatile float rcp = 1.0f / a2;
    bool ok = std::isfinite(rcp) && a2 != 0.0f;
    for (uint32_t b = 0; ok && b < 65536; ++b) {
        const uint32_t u = b << 16;
        float x;
        memcpy(&x, &u, 4);
        if (!std::isfinite(x)) continue;
        const volatile float qd = x / a2, qm = x * rcp;   // volatile: no fused / extended-precision evaluation
        // flush-to-zero differences between host and device do not matter: both sides would round tiny values the same
        if (to_bf(qd) != to_bf(qm)) ok = false;
    }
    cache[key] = ok;
    return ok;
}

// DIV of the un-rotate kernels for the divisor a2 = attention_scaling^2 (rotate: tables were given)
template <int DT> static int pick_div(bool rotate, float a2) {
    return (!rotate || a2 == 1.0f) ? 0 : ((DT == RTK_BF16 && bf16_rcp_is_exact(a2)) ? 1 : 2);
}
// f(compile-time DIV) for the run-time div; only bf16 has the reciprocal form (DIV 1)
template <int DT, class F> static void with_div(int div, F&& f) {
    if (div == 0) return f(std::integral_constant<int, 0>{});
    if constexpr (DT == RTK_BF16) {
        if (div == 1) return f(std::integral_constant<int, 1>{});
    }
    f(std::integral_constant<int, 2>{});
}

template <int DT>
static int unrotate_impl(const void* q, int64_t qsh, int64_t qsl, const void* k, int64_t ksh, int64_t ksl, int Hq, int Hkv,
                         int L, int D, const float* cosv, const float* sinv, float a, char* q_out, char* k_out, char* k_f16,
                         hipStream_t st) {
    const float a2 = (float)((double)a * (double)a);  // python float ** 2, then an fp32 tensor / scalar
    constexpr int VE = Vec16<DT>::VE;
    const int es = 16 / VE;
    char* kt = k_f16 ? k_f16 : k_out;   // the copy of k~ the passes read
    const bool vec_ok = (D % (2 * VE) == 0) && ((qsh * es) % 16 == 0) && ((qsl * es) % 16 == 0) &&
                        ((ksh * es) % 16 == 0) && ((ksl * es) % 16 == 0) &&
                        ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)q_out | (uintptr_t)kt) & 15) == 0) &&
                        (!cosv || (((uintptr_t)cosv | (uintptr_t)sinv) & 15) == 0);
    if (k_f16 && !(vec_ok && D == HD)) {
        set_error("rtk_pivotkv_score: RTK_BF16_FAST needs head_dim %d and 16-byte aligned rows", HD);
        return RTK_EUNSUPPORTED;
    }
    if (vec_ok) {
        const int threads = L * (D / 2 / VE);
        const int groups = (Hq + UNROT_HEADS - 1) / UNROT_HEADS + (Hkv + UNROT_HEADS - 1) / UNROT_HEADS;
        const dim3 grid((threads + 255) / 256, groups);
        const float rcp = 1.0f / a2;
        // FAST: q~ -> fp16(q~ * log2(e)/sqrt(D)); k~ -> bf16 (only if the caller wants it) + fp16
        const float qscale = k_f16 ? 1.4426950408889634f / sqrtf((float)HD) : 1.f;
        auto launch = [&](auto kern) {
            RTK_LAUNCH(KID_UNROT, kern, grid, dim3(256), 0, st, (const char*)q, qsh, qsl, (const char*)k, ksh, ksl, Hq, Hkv, L, D,
                       cosv, sinv, a2, rcp, q_out, k_out, k_f16, qscale);
        };
        with_div<DT>(pick_div<DT>(cosv != nullptr, a2), [&](auto div) {
            constexpr int DIV = decltype(div)::value;
            if constexpr (DT == RTK_BF16) {
                if (k_f16) return launch(unrotate_pack_vec_kernel<DT, DIV, true>);
            }
            launch(unrotate_pack_vec_kernel<DT, DIV, false>);
        });
    } else {
        const size_t nq = (size_t)Hq * L * (D / 2), nk = (size_t)Hkv * L * (D / 2);
        const dim3 gq((unsigned)std::min<size_t>((nq + 255) / 256, 8192)), gk((unsigned)std::min<size_t>((nk + 255) / 256, 8192));
        RTK_LAUNCH(KID_UNROT, unrotate_pack_kernel<DT>, gq, dim3(256), 0, st, q, qsh, qsl, Hq, L, D, cosv, sinv, a2, (void*)q_out);
        RTK_LAUNCH(KID_UNROT, unrotate_pack_kernel<DT>, gk, dim3(256), 0, st, k, ksh, ksl, Hkv, L, D, cosv, sinv, a2, (void*)k_out);
    }
    RTK_LAUNCH_CHECK("unrotate_pack_kernel");
    return RTK_OK;
}

int score_unrotate(int payload, const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, int64_t k_stride_h,
                   int64_t k_stride_l, int Hq, int Hkv, int L, int D, const float* cosv, const float* sinv,
                   float attention_scaling, char* q_out, char* k_out, char* k_f16, hipStream_t st) {
    auto call = [&](auto dt) {
        return unrotate_impl<decltype(dt)::value>(q, q_stride_h, q_stride_l, k, k_stride_h, k_stride_l, Hq, Hkv, L, D, cosv, sinv,
                                                  attention_scaling, q_out, k_out, k_f16, st);
    };
    return with_payload(payload, call);
}

// one prepare_native_kernel launch: qt / k_fast are q~ and (RTK_BF16_FAST) the fp16 k~ inside a.workspace
template <int DT>
static int prepare_impl(const PrepareArgs& a, const RowSel& rs, char* qt, char* k_fast, hipStream_t st) {
    const float a2 = (float)((double)a.attention_scaling * (double)a.attention_scaling);
    const float rcp = 1.0f / a2;
    // 16-bit dtypes: 4-byte chunks per thread - four times the waves of the 16-byte form, a quarter of the instruction
    // stream each (same-box A/B, profiles/r11_ab_prepare_chunk_width.txt: 20.0 -> 16.1 us at L = 2304, 29.6 -> 28.4 at 6272)
    constexpr int NW = DT != RTK_F32 ? PREP_NW : 4;   // 32-bit words per thread and row half
    constexpr int VE = NW * 4 / (DT == RTK_F32 ? 4 : 2);
    const int threads = a.L * (a.D / 2 / VE);
    static_assert(PREP_YSPLIT >= 2, "the first y-slice takes k and the LAST one v: one slice would never append v");
    // (+ one column of workgroups when the next layer's id shift rides along: its last one does the shift)
    const dim3 grid((threads + PREP_BLOCK - 1) / PREP_BLOCK + (a.shift_row ? 1 : 0), PREP_YSPLIT);
    // k_fast (RTK_BF16_FAST): q~ as fp16(q~ * log2(e)/sqrt(D)), k~ as bf16 (eviction) and as fp16 at k_fast (scoring)
    const float qscale = k_fast ? 1.4426950408889634f / sqrtf((float)a.D) : 1.f;
    auto launch = [&](auto kern) {
        RTK_LAUNCH(KID_UNROT, kern, grid, dim3(PREP_BLOCK), 0, st, (const char*)a.q, a.q_stride_h, a.q_stride_l, (const char*)a.k,
                   a.k_stride_h, a.k_stride_l, (const char*)a.v, a.v_stride_h, a.v_stride_l, a.Hq, a.Hkv, a.L, a.D, a.pos,
                   a.pos_stride, a.inv_freq, a.attention_scaling, rs, a.round_bf16, a2, rcp, qt, (char*)a.k_unrot,
                   (char*)a.k_tail, (char*)a.v_tail, a.tail_stride_h, a.P, a.pos_copy, k_fast, qscale, a.shift_row, a.next_prev,
                   a.ticket, a.status);
    };
    with_div<DT>(pick_div<DT>(true, a2), [&](auto div) {
        constexpr int DIV = decltype(div)::value;
        if constexpr (DT == RTK_BF16) {
            if (k_fast) return launch(prepare_native_kernel<DT, DIV, true, NW>);
        }
        launch(prepare_native_kernel<DT, DIV, false, NW>);
    });
    RTK_LAUNCH_CHECK("prepare_native_kernel");
    return RTK_OK;
}

}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_prepare(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k,
                                   int64_t k_stride_h, int64_t k_stride_l, const void* v, int64_t v_stride_h,
                                   int64_t v_stride_l, int Hq, int Hkv, int L, int D, int dtype, const int64_t* pos,
                                   int64_t pos_stride, int P, const float* inv_freq, float attention_scaling,
                                   const int* sections_host, int nsec, int round_bf16, void* k_unrot, void* workspace,
                                   size_t workspace_bytes, void* k_tail, void* v_tail, int64_t tail_stride_h,
                                   int64_t* pos_copy, rtk_stream_t stream) {
    return pivotkv_prepare_shift({q, q_stride_h, q_stride_l, k, k_stride_h, k_stride_l, v, v_stride_h, v_stride_l, Hq, Hkv, L, D,
                                  dtype, pos, pos_stride, P, inv_freq, attention_scaling, sections_host, nsec, round_bf16,
                                  k_unrot, workspace, workspace_bytes, k_tail, v_tail, tail_stride_h, pos_copy,
                                  nullptr, nullptr, nullptr, 0, nullptr}, stream);
}

// words of rtk_update_io.ticket: the launch count (word 0) and the run-out latch (word 31) in the first cache line, then
// the arrival counters of the prepare launch, a cache line each
extern "C" size_t rtk_pivotkv_shift_ticket_ints(int L, int D) {
    (void)L; (void)D;   // one line for the launch count, one per counter
    return (size_t)RTK_SHIFT_STRIDE * (1 + RTK_SHIFT_COUNTERS);
}

// rtk_pivotkv_prepare + (a.shift_row != NULL) the next layer's continuity shift in the same launch (PrepareArgs, common.cuh)
int rtk::pivotkv_prepare_shift(PrepareArgs a, rtk_stream_t stream) {
    RTK_CHECK_ARG(!a.shift_row || (a.ticket && a.ticket_ints >= (int64_t)rtk_pivotkv_shift_ticket_ints(a.L, a.D)),
                  "rtk_pivotkv_prepare: the in-launch id shift needs rtk_pivotkv_shift_ticket_ints(L, D) zeroed device words");
    const bool k_only = (a.dtype & RTK_PREPARE_K_ONLY) != 0;   // keep-all chunk: no q~
    a.dtype &= ~RTK_PREPARE_K_ONLY;
    const int dtype_full = a.dtype;            // may carry RTK_SCORE_MANY_UNITS: the workspace layout follows the split policy
    const int dtype = a.dtype &= ~RTK_SCORE_MANY_UNITS;
    const int L = a.L, D = a.D;
    RTK_CHECK_ARG(a.q && a.k && a.v && a.pos && a.inv_freq && a.k_unrot && a.workspace && a.k_tail && a.v_tail,
                  "rtk_pivotkv_prepare: NULL pointer");
    RTK_CHECK_ARG(a.Hq >= 1 && a.Hkv >= 1 && L >= 1 && D >= 2, "rtk_pivotkv_prepare: bad shape");
    RTK_CHECK_ARG(dtype == RTK_F32 || dtype == RTK_BF16 || dtype == RTK_BF16_FAST || dtype == RTK_F16,
                  "rtk_pivotkv_prepare: unsupported dtype %d", dtype);
    RTK_CHECK_ARG(a.pos_stride >= L, "rtk_pivotkv_prepare: pos_stride %lld < L %d", (long long)a.pos_stride, L);
    const bool fast = dtype == RTK_BF16_FAST && !k_only;
    if (fast && D != HD) {
        set_error("rtk_pivotkv_prepare: RTK_BF16_FAST needs head_dim %d", HD);
        return RTK_EUNSUPPORTED;
    }
    RTK_CHECK_ARG(((uintptr_t)a.workspace & 255) == 0, "rtk_pivotkv_prepare: workspace must be 256-byte aligned");
    const ScoreWs w = score_ws(a.Hq, a.Hkv, L, D, dtype_full);
    if (!k_only && a.workspace_bytes < w.total) {
        set_error("rtk_pivotkv_prepare: workspace %zu < required %zu bytes", a.workspace_bytes, w.total);
        return RTK_EWORKSPACE;
    }
    if (k_only) a.Hq = 0;   // the kernel's query loop is empty; k / v take the same path
    const int Hq = a.Hq, Hkv = a.Hkv, es = dtype != RTK_F32 ? 2 : 4;
    char* qt = (char*)a.workspace + w.q_off;
    // (declined: callers fall back to rtk_rope_table + rtk_pivotkv_score + rtk_pivotkv_append)
    int rc = check_buffer_operands("rtk_pivotkv_prepare", es, D, L,
                                   {{a.q, Hq, a.q_stride_h, a.q_stride_l}, {a.k, Hkv, a.k_stride_h, a.k_stride_l},
                                    {a.v, Hkv, a.v_stride_h, a.v_stride_l}, {a.k_tail, Hkv, a.tail_stride_h, D},
                                    {a.v_tail, Hkv, a.tail_stride_h, D},
                                    {qt, Hq, (int64_t)L * D, D}, {a.k_unrot, Hkv, (int64_t)L * D, D}});   // the packed q~ and k~
    if (rc) return rc;
    RowSel rs;
    rc = make_rowsel(rs, a.P, D, a.sections_host, a.nsec, "rtk_pivotkv_prepare");
    if (rc) return rc;
    char* k_fast = fast ? (char*)a.workspace + w.k_off : nullptr;
    return with_payload(dtype, [&](auto dt) { return prepare_impl<decltype(dt)::value>(a, rs, qt, k_fast, (hipStream_t)stream); });
}

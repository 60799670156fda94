// pivotkv_update.hip — PivotKVCache.update and the per-chunk flush as ONE call each (rtk_pivotkv_update / _flush /
// _append_rope, include/retake_hip.h), and the attention prologue: the one kernel that takes a layer's pre-RoPE
// projections to everything the layer's attention and the deferred PivotKV scoring need.  The RoPE arithmetic
// (rotate_words, unrotate_words) and the operand rules of the buffer-addressed kernels (check_buffer_operands) are
// common.cuh's, shared with pivotkv_prepare.hip.
//
// Why: a 2048-frame video is 1,792 updates (qwen2_vl.py:670-720 calls the decoder once per chunk, every layer calls
// cache.update, longvideo_cache.py:217).  At the real Qwen2-VL geometry (L = 2304) the GPU work of one update is ~20 us;
// ~50 us of host work per update (argument marshalling for a 30-argument launch, view construction, dict bookkeeping)
// made the step host-bound.  The argument blocks are bound once per chunk geometry (rtk_pivotkv_batch) and per layer
// (rtk_layer_state); an update is then four pointer stores and one call.
#include <algorithm>
#include <vector>

#include "common.cuh"

namespace rtk {

// ------------------------------------------------------------------------------------------------
// Attention prologue (qwen2_vl.py:55-86 / llava_onevision.py:59-141 + longvideo_cache.py:238, :248-259), from the
// PRE-RoPE projections q0 [Hq,L,D], k0, v0 [Hkv,L,D] (strided: the [L, H*D] layout the projections produce):
//   ids      t' = t + (prev + 1 - t[0]) on the temporal row (the continuity shift, qwen2_vl.py:68-73); a copy of the
//            shifted ids goes to pos_copy for the deferred selection
//   tables   cos / sin of the token's ids in registers: rope_chunk (= rtk_rope_table's arithmetic: fp32 id * inv_freq,
//            correctly rounded sin / cos, * attention_scaling, rounded to the model dtype like the rotary module's
//            `.to(x.dtype)`), M-RoPE rows picked per channel (:68-74)
//   q_rot    (q0*cos) + (rotate_half(q0)*sin), one rounding per torch op (apply_multimodal_rotary_pos_emb :80-81)
//            -> the layer's attention; may alias q0 (every address is read and written by one thread only)
//   k tail   the same rotation of k0, appended to the cache tail; v tail: v0 (:238)
//   q~, k~   the score passes' operands.  The reference un-rotates the rotated tensors (:248-259); un-rotating a
//            rotation returns the pre-RoPE value up to the rounding of the round trip, so q~ := q0 and
//            k~ := k0 - copies into the contiguous [H,L,D] layout the matrix passes stream.
// One thread = one token x one NW-word chunk pair (d, d + D/2); blockIdx.y splits the query heads, y = 0 also takes
// k, the last y takes v.  Same software pipeline as prepare_native_kernel: the rows of head batch b+1 are requested
// before batch b is rotated and stored, and the first batch before the table arithmetic.
// ------------------------------------------------------------------------------------------------
template <int DT, bool FAST, int NW, bool RT = false>
__global__ __launch_bounds__(PREP_BLOCK) void prologue_kernel(const char* q, int64_t q_sh, int64_t q_sl,
                                                      const char* __restrict__ k, int64_t k_sh, int64_t k_sl,
                                                      const char* __restrict__ v, int64_t v_sh, int64_t v_sl,
                                                      int Hq, int Hkv, int L, int D,
                                                      const int64_t* pos, int64_t pos_ld,
                                                      const int64_t* __restrict__ prev,
                                                      const float* __restrict__ inv_freq, float scaling, RowSel rs,
                                                      int round_mode, char* q_rot, int64_t qr_sh, int64_t qr_sl,
                                                      char* __restrict__ q_out, char* __restrict__ k_out,
                                                      char* __restrict__ k_tail, char* __restrict__ v_tail,
                                                      int64_t tail_sh, int P, int64_t* __restrict__ pos_copy,
                                                      int64_t pos_copy_ld, char* __restrict__ k_fast, float qscale,
                                                      int64_t* shift_back, float a2, float rcp_a2, int div) {
    using V = Vec16<DT>;
    static_assert(NW == 4 || ((NW == 2 || NW == 1) && DT != RTK_F32), "8- / 4-byte chunks: 16-bit dtypes only");
    constexpr int ES = 16 / V::VE;          // bytes per element
    constexpr int VE = 4 * NW / ES;         // elements per thread and row half
    using W = WV<NW>;
    const int h2 = D / 2, lpr = h2 / VE;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= L * lpr) return;
    const int l = id / lpr, d = (id - l * lpr) * VE;
    // continuity shift: the whole temporal row moves so that its first id follows the layer's last cached id.  The row's
    // first id is read ONCE per thread (a relaxed atomic load the compiler can neither split nor repeat): a one-token
    // segment's launch stores the shifted id back into pos[0] while other workgroups may still be reading it, and both
    // the delta and the token's own id must come from the same value (old: delta = prev + 1 - t0, id = prev + 1; new:
    // delta = 0, id = prev + 1).
    const long long t0 = (long long)__hip_atomic_load(pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long delta = (prev ? (long long)prev[0] : -1ll) + 1 - t0;
    // pos_ld == 0: the three M-RoPE rows are ONE row seen three times (HF's decode ids, `.expand(3, -1, -1)`,
    // qwen2_vl.py:589): the reference's in-place shift of row 0 moves the shared storage, i.e. t, h and w together
    const bool rows_alias = pos_ld == 0;
    long long ids[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int pr = min(p, P - 1);
        const bool temporal = pr == 0 || rows_alias;
        const long long raw = (temporal && l == 0) ? t0 : (long long)pos[(size_t)pr * pos_ld + l];
        ids[p] = raw + (temporal ? delta : 0ll);
    }
    if (pos_copy && blockIdx.y == 0 && d == 0)
        for (int p = 0; p < P; ++p) pos_copy[(size_t)p * pos_copy_ld + l] = ids[p];
    // a one-token segment (decode): the caller's temporal id is shifted in place by this launch (qwen2_vl.py:73) - the
    // shift is idempotent (afterwards t[0] == prev + 1, so a thread that reads the new value computes delta 0 and the
    // same id) and a single aligned 8-byte atomic store cannot be seen torn, so no workgroup order is needed
    if (shift_back && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        __hip_atomic_store(shift_back, (int64_t)ids[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    constexpr int HU = PREP_HU;
    const int ny = gridDim.y, qper = (Hq + ny - 1) / ny;
    const int qb = uniform_int(min((int)blockIdx.y * qper, Hq)), qe = uniform_int(min(qb + qper, Hq));   // (head loops in SGPRs)
    const bool is_k = blockIdx.y == 0;
    const bool has_kv = is_k || (int)blockIdx.y == ny - 1;
    const char* src = is_k ? k : v;
    const int64_t sh = is_k ? k_sh : v_sh, sl = is_k ? k_sl : v_sl;
    char* tail = is_k ? k_tail : v_tail;
    const int nkv = has_kv ? Hkv : 0;
    W lo[HU], hi[HU], lon[HU], hin[HU];
    // a row's address = descriptor (tensor base) + soffset (the head: wave-uniform, a scalar multiply) + voffset (this
    // thread's byte offset inside a head, computed once); the launcher has checked that every extent fits 31 bits
    const uint32_t off_q = (uint32_t)(((int64_t)l * q_sl + d) * ES), off_kv = (uint32_t)(((int64_t)l * sl + d) * ES);
    const uint32_t off_qr = (uint32_t)(((int64_t)l * qr_sl + d) * ES);
    const uint32_t off_o = (uint32_t)(((int64_t)l * D + d) * ES), half = (uint32_t)(h2 * ES);
    const uint32_t off_q2 = off_q + half, off_kv2 = off_kv + half, off_o2 = off_o + half, off_qr2 = off_qr + half;
    const __amdgpu_buffer_rsrc_t r_q = buf_rsrc(q), r_src = buf_rsrc(src), r_qo = buf_rsrc(q_out), r_ko = buf_rsrc(k_out),
                                 r_tail = buf_rsrc(tail), r_kf = buf_rsrc(k_fast), r_qr = buf_rsrc(q_rot);
    const uint32_t hs_q = (uint32_t)(q_sh * ES), hs_kv = (uint32_t)(sh * ES), hs_o = (uint32_t)((int64_t)L * D * ES),
                   hs_t = (uint32_t)(tail_sh * ES), hs_qr = (uint32_t)(qr_sh * ES);
    auto load_q = [&](W* a, W* b, int hb) { load_heads<NW, HU>(a, b, r_q, off_q, off_q2, hs_q, hb, qe - 1); };
    auto load_kv = [&](W* a, W* b, int hb) { load_heads<NW, 4>(a, b, r_src, off_kv, off_kv2, hs_kv, hb, Hkv - 1); };
    float pid[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) pid[p] = (float)ids[p];   // position_ids.float() inside the rotary module
    if (qb < qe) load_q(lo, hi, qb);
    else if (nkv) load_kv(lo, hi, 0);
    float c1[VE], s1[VE], c2[VE], s2[VE];
    rope_chunk<VE>(inv_freq, rs, d, h2, pid, scaling, round_mode, c1, s1, c2, s2);
    // (x*cos) + (rotate_half(x)*sin) for one head's chunk pair, one rounding per torch op
    auto rot = [&](const W& lo, const W& hi, W& olo, W& ohi) { rotate_words<DT, NW>(lo, hi, c1, s1, c2, s2, olo, ohi); };
    // RT (reference operands): x~ = ((x*cos) - (rotate_half(x)*sin)) / a^2 of the ROTATED pair, one rounding per torch op
    // (longvideo_cache.py:76-78) - the un-rotation the reference applies to what its attention handed over.  div (uniform):
    // 0 a^2 == 1, 1 multiply by the reciprocal (bf16, proven identical for every bf16 input: bf16_rcp_is_exact), 2 IEEE
    // division.  This is unrotate_words (common.cuh) with a run-time div, kept as a LOCAL COPY: through the shared function
    // the two bf16 RT instantiations are scheduled differently (same arithmetic, ~10 instructions moved, one VGPR fewer)
    // and nobody has timed that form on an MI355X yet.  A change to one text must be made to the other:
    // test_prologue_with_reference_operands_equals_the_update_route_bitwise compares the two bit for bit.
    auto unrot = [&](const W& lo, const W& hi, W& olo, W& ohi) {
        if constexpr (DT != RTK_F32) {
            using Hh = H16<DT>;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const float x1a = Hh::lo(lo.w[w]), x1b = Hh::hi(lo.w[w]), x2a = Hh::lo(hi.w[w]), x2b = Hh::hi(hi.w[w]);
                const int e = 2 * w;
                const uint32_t p1 = Hh::pack2(x1a * c1[e], x1b * c1[e + 1]);
                const uint32_t n1 = Hh::pack2(x2a * s1[e], x2b * s1[e + 1]);
                const uint32_t p2 = Hh::pack2(x2a * c2[e], x2b * c2[e + 1]);
                const uint32_t n2 = Hh::pack2(x1a * s2[e], x1b * s2[e + 1]);
                uint32_t t1 = Hh::pack2(Hh::lo(p1) + Hh::lo(n1), Hh::hi(p1) + Hh::hi(n1));
                uint32_t t2 = Hh::pack2(Hh::lo(p2) - Hh::lo(n2), Hh::hi(p2) - Hh::hi(n2));
                if (div == 1) {
                    t1 = Hh::pack2(Hh::lo(t1) * rcp_a2, Hh::hi(t1) * rcp_a2);
                    t2 = Hh::pack2(Hh::lo(t2) * rcp_a2, Hh::hi(t2) * rcp_a2);
                } else if (div == 2) {
                    t1 = Hh::pack2(__fdiv_rn(Hh::lo(t1), a2), __fdiv_rn(Hh::hi(t1), a2));
                    t2 = Hh::pack2(__fdiv_rn(Hh::lo(t2), a2), __fdiv_rn(Hh::hi(t2), a2));
                }
                olo.w[w] = t1;
                ohi.w[w] = t2;
            }
        } else {
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const float x1 = __uint_as_float(lo.w[e]), x2 = __uint_as_float(hi.w[e]);
                float o1 = __fsub_rn(__fmul_rn(x1, c1[e]), __fmul_rn(-x2, s1[e]));
                float o2 = __fsub_rn(__fmul_rn(x2, c2[e]), __fmul_rn(x1, s2[e]));
                if (div != 0) {
                    o1 = __fdiv_rn(o1, a2);
                    o2 = __fdiv_rn(o2, a2);
                }
                olo.w[e] = __float_as_uint(o1);
                ohi.w[e] = __float_as_uint(o2);
            }
        }
    };
    for (int hb = qb; hb < qe; hb += HU) {
        if (hb + HU < qe) load_q(lon, hin, hb + HU);
        else if (nkv) load_kv(lon, hin, 0);
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int h = hb + u;
            if (h >= qe) break;
            W olo, ohi;
            rot(lo[u], hi[u], olo, ohi);
            if (q_out) {   // q~ := q0, or (RT) the un-rotation of the rotated row (keep-all chunks are not scored: no q~)
                W ql = lo[u], qh = hi[u];
                if constexpr (RT) unrot(olo, ohi, ql, qh);
                if constexpr (FAST) {
                    ql = bf16_to_f16_words<NW>(ql, qscale);
                    qh = bf16_to_f16_words<NW>(qh, qscale);
                }
                buf_store<NW>(ql, r_qo, off_o, head_soff(h, hs_o));
                buf_store<NW>(qh, r_qo, off_o2, head_soff(h, hs_o));
            }
            buf_store<NW>(olo, r_qr, off_qr, head_soff(h, hs_qr));
            buf_store<NW>(ohi, r_qr, off_qr2, head_soff(h, hs_qr));
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
            const uint32_t so_t = head_soff(h, hs_t), so_o = head_soff(h, hs_o);
            if (is_k) {
                W olo, ohi;
                rot(lo[u], hi[u], olo, ohi);
                W kl = lo[u], kh = hi[u];
                if constexpr (RT) unrot(olo, ohi, kl, kh);
                if (k_out) {   // k~ := k0 / (RT) un-rotated tail row (a plain append - text segments, decode - scores nothing: no k~)
                    buf_store<NW>(kl, r_ko, off_o, so_o);
                    buf_store<NW>(kh, r_ko, off_o2, so_o);
                }
                if constexpr (FAST) {
                    buf_store<NW>(bf16_to_f16_words<NW>(kl, 1.f), r_kf, off_o, so_o);
                    buf_store<NW>(bf16_to_f16_words<NW>(kh, 1.f), r_kf, off_o2, so_o);
                }
                buf_store<NW>(olo, r_tail, off_o, so_t);
                buf_store<NW>(ohi, r_tail, off_o2, so_t);
            } else {
                buf_store<NW>(lo[u], r_tail, off_o, so_t);
                buf_store<NW>(hi[u], r_tail, off_o2, so_t);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lo[u] = lon[u];
            hi[u] = hin[u];
        }
    }
}

// one prologue launch: the chunk's geometry and rotary, the caller's tensors (io), and where the results go
struct PrologueArgs {
    int Hq, Hkv, L, D, P, round_mode;
    const float* inv_freq;
    float scaling;
    const rtk_update_io* io;         // q0, k0, v0, q_rot and the position ids
    const int64_t* prev;             // the layer's last cached id (NULL: none)
    char *q_out, *k_out, *k_fast;    // q~, k~ (NULL: not wanted) and RTK_BF16_FAST's fp16 k~
    char *k_tail, *v_tail;
    int64_t tail_sh;
    int64_t* pos_copy;               // the shifted ids, rows pos_copy_ld apart
    int64_t pos_copy_ld;
    int64_t* shift_back;             // a one-token segment's id, shifted in place by the launch
    bool roundtrip;                  // reference operands: q~ / k~ are the un-rotation of the rotated rows
};

template <int DT>
static int prologue_launch(const PrologueArgs& a, const RowSel& rs, hipStream_t st) {
    // reference operands (roundtrip): the divisor of the un-rotation, as torch evaluates `/ attention_scaling ** 2` on
    // a tensor of the model dtype - fp32 opmath with the Python double rounded to fp32 (prepare_impl's rule)
    const float a2 = (float)((double)a.scaling * (double)a.scaling);
    const int div = !a.roundtrip || a2 == 1.0f ? 0 : ((DT == RTK_BF16 && bf16_rcp_is_exact(a2)) ? 1 : 2);
    const float rcp_a2 = 1.0f / a2;
    constexpr int NW = DT != RTK_F32 ? PREP_NW : 4;   // 32-bit words per thread and row half
    constexpr int VE = NW * 4 / (DT == RTK_F32 ? 4 : 2);
    const int threads = a.L * (a.D / 2 / VE);
    const dim3 grid((threads + PREP_BLOCK - 1) / PREP_BLOCK, PREP_YSPLIT);
    const float qscale = a.k_fast ? 1.4426950408889634f / sqrtf((float)a.D) : 1.f;
    const rtk_update_io* io = a.io;
    auto launch = [&](auto kern) {
        RTK_LAUNCH(KID_PROLOGUE, kern, grid, dim3(PREP_BLOCK), 0, st, (const char*)io->q, io->q_stride_h, io->q_stride_l,
                   (const char*)io->k, io->k_stride_h, io->k_stride_l, (const char*)io->v, io->v_stride_h, io->v_stride_l,
                   a.Hq, a.Hkv, a.L, a.D, io->pos, io->pos_stride, a.prev, a.inv_freq, a.scaling, rs, a.round_mode,
                   (char*)io->q_rot, io->qr_stride_h, io->qr_stride_l, a.q_out, a.k_out, a.k_tail, a.v_tail, a.tail_sh, a.P,
                   a.pos_copy, a.pos_copy_ld, a.k_fast, qscale, a.shift_back, a2, rcp_a2, div);
    };
    const bool fast = DT == RTK_BF16 && a.k_fast;
    if constexpr (DT == RTK_BF16) {
        if (fast) {
            if (a.roundtrip) launch(prologue_kernel<DT, true, NW, true>);
            else launch(prologue_kernel<DT, true, NW, false>);
        }
    }
    if (!fast) {
        if (a.roundtrip) launch(prologue_kernel<DT, false, NW, true>);
        else launch(prologue_kernel<DT, false, NW, false>);
    }
    RTK_LAUNCH_CHECK("prologue_kernel");
    return RTK_OK;
}
static int prologue(int dtype, const PrologueArgs& a, const RowSel& rs, rtk_stream_t stream) {
    return with_payload(dtype, [&](auto dt) { return prologue_launch<decltype(dt)::value>(a, rs, (hipStream_t)stream); });
}

// where a layer's next rows go: the tail of its K and V buffers ([Hkv, cap, D], `length` rows used)
struct Tail {
    char *k, *v;
    int64_t stride_h;
};
static Tail tail_of(const rtk_layer_state* ls, int D, int es) {
    const size_t used = (size_t)ls->length * D * es;
    return {(char*)ls->k + used, (char*)ls->v + used, ls->cap * D};
}
// the layer's last cached temporal id, the predecessor of the continuity shift (qwen2_vl.py:68-73); NULL: nothing cached
static const int64_t* last_id(const rtk_layer_state* ls) {
    return (ls->pos && ls->pos_len > 0) ? ls->pos + (ls->pos_len - 1) : nullptr;
}

}  // namespace rtk

using namespace rtk;

static int check_batch(const rtk_pivotkv_batch* b, const char* who) {
    RTK_CHECK_ARG(b, "%s: NULL batch", who);
    RTK_CHECK_ARG(b->Hq >= 1 && b->Hkv >= 1 && b->Hq % b->Hkv == 0 && b->L >= 1 && b->D >= 2 && b->slots >= 1,
                  "%s: bad geometry", who);
    RTK_CHECK_ARG(b->keep >= 1 && b->keep <= b->L, "%s: keep=%d out of range for L=%d", who, b->keep, b->L);
    RTK_CHECK_ARG(b->P == 0 || b->P == 1 || b->P == 3, "%s: P must be 0, 1 or 3, got %d", who, b->P);
    RTK_CHECK_ARG(b->dtype == RTK_F32 || b->dtype == RTK_BF16 || b->dtype == RTK_F16, "%s: unsupported dtype %d", who, b->dtype);
    RTK_CHECK_ARG(b->nsec >= 0 && b->nsec <= 8, "%s: nsec %d out of range", who, b->nsec);
    RTK_CHECK_ARG(b->keep_idx && (b->keep_all || b->v_stage || b->compact_sync), "%s: NULL batch buffer", who);
    RTK_CHECK_ARG(b->keep_all || (b->score_ws && b->partials && b->score && b->sel_ws), "%s: NULL scoring buffer", who);
    return RTK_OK;
}

// rtk_pivotkv_update with RTK_UPDATE_PRE_ROPE: the attention prologue on the pre-RoPE projections
static int update_pre_rope(rtk_pivotkv_batch* b, const rtk_layer_state* ls, int slot, const rtk_update_io* io, const Tail& t,
                           char* ws, char* k_unrot, int64_t* pos_copy, rtk_stream_t stream) {
    const int L = b->L, D = b->D, Hq = b->Hq, Hkv = b->Hkv, score_base = b->score_dtype & 0xFF;
    int es, ve;
    payload_dims(b->dtype, es, ve);
    RTK_CHECK_ARG(io->q_rot, "rtk_pivotkv_update: RTK_UPDATE_PRE_ROPE needs q_rot");
    const bool roundtrip = (io->flags & RTK_UPDATE_ROUNDTRIP) != 0;
    if ((score_base == RTK_BF16_REFROUND || score_base == RTK_F16_REFROUND) && !roundtrip) {
        set_error("rtk_pivotkv_update: score_rounding='reference' scores the reference's round-tripped q~ / k~ "
                  "(set RTK_UPDATE_ROUNDTRIP, or rotate first and update without RTK_UPDATE_PRE_ROPE)");
        return RTK_EUNSUPPORTED;
    }
    RTK_CHECK_ARG(!(roundtrip && (io->flags & RTK_UPDATE_Q_IN_PLACE)),
                  "rtk_pivotkv_update: RTK_UPDATE_ROUNDTRIP makes q~ differ from q0: it cannot be scored in place");
    int rc = check_buffer_operands("rtk_pivotkv_update", es, D, L,
                                   {{io->q, Hq, io->q_stride_h, io->q_stride_l}, {io->q_rot, Hq, io->qr_stride_h, io->qr_stride_l},
                                    {io->k, Hkv, io->k_stride_h, io->k_stride_l}, {io->v, Hkv, io->v_stride_h, io->v_stride_l},
                                    {t.k, Hkv, t.stride_h, D}, {t.v, Hkv, t.stride_h, D},
                                    {ws, Hq, (int64_t)L * D, D}, {k_unrot, Hkv, (int64_t)L * D, D}});   // the packed q~ and k~
    if (rc) return rc;
    if (b->P == 3 && io->pos_stride < L && io->pos_stride != 0) {   // partially overlapping id rows: the eager route
        set_error("rtk_pivotkv_update: position-id rows overlap (pos_stride %lld < L %d)", (long long)io->pos_stride, L);
        return RTK_EUNSUPPORTED;
    }
    const size_t need = rtk_pivotkv_score_workspace_bytes(Hq, Hkv, L, D, b->score_dtype);
    if (!b->keep_all && b->score_ws_bytes < need) {
        set_error("rtk_pivotkv_update: workspace %zu < required %zu bytes", (size_t)b->score_ws_bytes, need);
        return RTK_EWORKSPACE;
    }
    RowSel rs;
    rc = make_rowsel(rs, b->P, D, b->nsec ? b->sections : nullptr, b->nsec, "rtk_pivotkv_update");
    if (rc) return rc;
    char* q_out = b->keep_all ? nullptr : ws;   // q~ at offset 0 of the slot's score workspace
    if ((io->flags & RTK_UPDATE_Q_IN_PLACE) && !b->keep_all) {
        // q~ IS io->q: the batched passes of the flush stream it from where it lies
        if (!b->q_units || !b->batched_passes || score_base == RTK_BF16_FAST || io->q_rot == io->q) {
            set_error("rtk_pivotkv_update: RTK_UPDATE_Q_IN_PLACE needs batch.q_units, the batched passes, exact score "
                      "arithmetic and rotated queries that go elsewhere");
            return RTK_EINVAL;
        }
        for (int u = 0; u < b->slots; ++u)   // one pointer table, one pair of strides per flush
            if (u != slot && b->q_units[u] && (b->q_stride_h != io->q_stride_h || b->q_stride_l != io->q_stride_l)) {
                set_error("rtk_pivotkv_update: the pending units' queries have other strides (flush first)");
                return RTK_EUNSUPPORTED;
            }
        b->q_units[slot] = io->q;
        b->q_stride_h = io->q_stride_h;
        b->q_stride_l = io->q_stride_l;
        q_out = nullptr;
    } else if (b->q_units) {
        b->q_units[slot] = nullptr;
    }
    // RTK_BF16_FAST (bf16 payloads): a second, fp16 copy of k~ inside the workspace, right behind q~ (score_ws: k_off)
    char* k_fast = nullptr;
    if (score_base == RTK_BF16_FAST && !b->keep_all && b->dtype == RTK_BF16)
        k_fast = ws + (((size_t)Hq * L * D * es + 255) & ~(size_t)255);
    return prologue(b->dtype, {Hq, Hkv, L, D, b->P, b->round_mode, b->inv_freq, b->attention_scaling, io, last_id(ls), q_out,
                               k_unrot, k_fast, t.k, t.v, t.stride_h, pos_copy, L, nullptr, roundtrip}, rs, stream);
}

// ... without it: the fused prepare on the rotated q / k, optionally with the NEXT layer's continuity shift in the launch
static int update_rotated(rtk_pivotkv_batch* b, int slot, const rtk_update_io* io, const Tail& t, char* ws, char* k_unrot,
                          int64_t* pos_copy, rtk_stream_t stream) {
    if (b->q_units) b->q_units[slot] = nullptr;
    const int dt = b->prep_dtype | (b->keep_all ? RTK_PREPARE_K_ONLY : 0);
    // RTK_UPDATE_SHIFT_NEXT: the launch also leaves the caller's temporal row shifted for the NEXT layer (qwen2_vl.py:68-73)
    const bool shift_next = (io->flags & RTK_UPDATE_SHIFT_NEXT) != 0;
    if (shift_next && !io->ticket) {
        set_error("rtk_pivotkv_update: RTK_UPDATE_SHIFT_NEXT needs io->ticket (rtk_pivotkv_shift_ticket_ints zeroed device words)");
        return RTK_EINVAL;
    }
    if (shift_next && !b->keep_all && !b->batched_passes) {
        // the per-unit passes may still decline (RTK_EUNSUPPORTED) AFTER the prepare launch has shifted the ids: a caller
        // that falls back to the stage-by-stage route would then re-prepare this layer from the NEXT layer's ids.
        // Decline first, with nothing launched.
        set_error("rtk_pivotkv_update: RTK_UPDATE_SHIFT_NEXT needs the chunk-batched passes or a keep-all batch");
        return RTK_EUNSUPPORTED;
    }
    return pivotkv_prepare_shift({io->q, io->q_stride_h, io->q_stride_l, io->k, io->k_stride_h, io->k_stride_l, io->v,
                                  io->v_stride_h, io->v_stride_l, b->Hq, b->Hkv, b->L, b->D, dt, io->pos, io->pos_stride, b->P,
                                  b->inv_freq, b->attention_scaling, b->nsec ? b->sections : nullptr, b->nsec, b->round_mode,
                                  k_unrot, ws, b->score_ws_bytes, t.k, t.v, t.stride_h, pos_copy,
                                  shift_next ? (int64_t*)io->pos : nullptr, io->next_prev, io->ticket, io->ticket_ints,
                                  shift_next ? io->status : nullptr}, stream);
}

extern "C" int rtk_pivotkv_update(rtk_pivotkv_batch* b, rtk_layer_state* ls, int slot, const rtk_update_io* io,
                                  rtk_stream_t stream) {
    int rc = check_batch(b, "rtk_pivotkv_update");
    if (rc) return rc;
    RTK_CHECK_ARG(ls && io, "rtk_pivotkv_update: NULL layer state or io block");
    RTK_CHECK_ARG(slot >= 0 && slot < b->slots, "rtk_pivotkv_update: slot %d outside the batch (%d slots)", slot, b->slots);
    RTK_CHECK_ARG(io->q && io->k && io->v, "rtk_pivotkv_update: NULL q / k / v");
    RTK_CHECK_ARG(ls->k && ls->v && ls->length >= 0 && ls->length + b->L <= ls->cap,
                  "rtk_pivotkv_update: the layer's cache has no room for the chunk (length %lld + %d > cap %lld)",
                  (long long)ls->length, b->L, (long long)ls->cap);
    RTK_CHECK_ARG(ls->pending == 0, "rtk_pivotkv_update: the layer still has a pending chunk (flush first)");
    if (!b->reforge || !b->inv_freq || b->P == 0 || !io->pos || !b->k_unrot || !b->score_ws) {
        set_error("rtk_pivotkv_update: needs pos_embed_reforge, position ids and an inv_freq rotary (use the per-stage calls)");
        return RTK_EUNSUPPORTED;
    }
    int es, ve;
    payload_dims(b->dtype, es, ve);
    const int L = b->L, D = b->D, Hkv = b->Hkv;
    const Tail t = tail_of(ls, D, es);
    char* ws = (char*)b->score_ws + (size_t)slot * b->score_ws_stride;
    char* k_unrot = (char*)b->k_unrot + (size_t)slot * Hkv * L * D * es;
    int64_t* pos_copy = b->pos_old ? b->pos_old + (size_t)slot * b->P * L : nullptr;
    rc = (io->flags & RTK_UPDATE_PRE_ROPE) ? update_pre_rope(b, ls, slot, io, t, ws, k_unrot, pos_copy, stream)
                                           : update_rotated(b, slot, io, t, ws, k_unrot, pos_copy, stream);
    if (rc) return rc;
    if (!b->keep_all && !b->batched_passes) {
        // shapes outside the chunk-batched passes (fp32 payloads, other head dims): the unit's two matrix passes now
        float* part = b->partials + (size_t)slot * b->partial_floats;
        const bool live = b->skip_masked && ls->mask && b->key_index;
        rc = rtk_pivotkv_score_stages_masked(ws, 0, 0, ws, 0, 0, b->Hq, Hkv, L, D, b->score_dtype, nullptr, nullptr, 1.0f,
                                             b->score + (size_t)slot * L, k_unrot, ws, b->score_ws_bytes, RTK_SCORE_PASSES,
                                             part, live ? ls->mask : nullptr,
                                             live ? b->key_index + (size_t)slot * (L + 1) : nullptr, stream);
        if (rc) return rc;
    }
    ls->pending = L;
    ls->pending_keep = b->keep;
    return RTK_OK;
}

extern "C" int rtk_pivotkv_append_rope(rtk_layer_state* ls, const rtk_update_io* io, int Hq, int Hkv, int n, int D,
                                       int dtype, int P, const float* inv_freq, float attention_scaling,
                                       const int* sections_host, int nsec, int round_mode, int shift_ids_in_place,
                                       rtk_stream_t stream) {
    RTK_CHECK_ARG(ls && io && io->q && io->k && io->v && io->q_rot && io->pos && inv_freq, "rtk_pivotkv_append_rope: NULL pointer");
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && n >= 1 && D >= 2, "rtk_pivotkv_append_rope: bad shape");
    int es, ve;
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "rtk_pivotkv_append_rope: unsupported dtype %d", dtype);
    RTK_CHECK_ARG(P == 1 || P == 3, "rtk_pivotkv_append_rope: P must be 1 or 3, got %d", P);
    RTK_CHECK_ARG(ls->k && ls->v && ls->pending == 0 && ls->length >= 0 && ls->length + n <= ls->cap,
                  "rtk_pivotkv_append_rope: the layer's cache has no room for %d rows (or a chunk is pending)", n);
    RTK_CHECK_ARG(ls->pos && ls->pos_len + n <= ls->pos_cap, "rtk_pivotkv_append_rope: the position cache has no room for %d ids", n);
    if (P == 3 && io->pos_stride < n && io->pos_stride != 0) {   // rows that overlap partially: not a layout torch hands out;
        set_error("rtk_pivotkv_append_rope: position-id rows overlap (pos_stride %lld < n %d)", (long long)io->pos_stride, n);
        return RTK_EUNSUPPORTED;                                     // fully aliased rows (stride 0, `.expand(3, ..)`) are served
    }
    const Tail t = tail_of(ls, D, es);
    int rc = check_buffer_operands("rtk_pivotkv_append_rope", es, D, n,
                                   {{io->q, Hq, io->q_stride_h, io->q_stride_l}, {io->q_rot, Hq, io->qr_stride_h, io->qr_stride_l},
                                    {io->k, Hkv, io->k_stride_h, io->k_stride_l}, {io->v, Hkv, io->v_stride_h, io->v_stride_l},
                                    {t.k, Hkv, t.stride_h, D}, {t.v, Hkv, t.stride_h, D}});
    if (rc) return rc;
    RowSel rs;
    rc = make_rowsel(rs, P, D, sections_host, nsec, "rtk_pivotkv_append_rope");
    if (rc) return rc;
    const int64_t* prev = last_id(ls);
    // one token (a decode step): the kernel shifts the caller's id itself; longer segments take the shift launch after it
    int64_t* shift_back = (shift_ids_in_place && n == 1) ? (int64_t*)io->pos : nullptr;
    // no q~ / k~: nothing is scored.  The shifted ids join the layer's position cache (reference :319-321)
    rc = prologue(dtype, {Hq, Hkv, n, D, P, round_mode, inv_freq, attention_scaling, io, prev, nullptr, nullptr, nullptr, t.k, t.v,
                          t.stride_h, ls->pos + ls->pos_len, ls->pos_cap, shift_back, false}, rs, stream);
    if (rc) return rc;
    if (shift_ids_in_place && !shift_back) {   // qwen2_vl.py:73: later layers (and the caller) see the shifted ids; after the kernel read them
        rc = rtk_position_shift((int64_t*)io->pos, n, prev, stream);
        if (rc) return rc;
    }
    ls->length += n;
    ls->pos_len += n;
    return RTK_OK;
}

// ---- rtk_pivotkv_flush: four stages over the n pending layers (slots[i] = layer i's unit of the batch) ----------------
namespace {
struct Flush {
    rtk_pivotkv_batch* b;
    rtk_layer_state* const* layers;
    const int32_t* slots;
    int n, es;
    rtk_stream_t stream;
    bool reforge() const { return b->reforge != 0; }
    char* k_unrot(int slot) const { return (char*)b->k_unrot + (size_t)slot * b->Hkv * b->L * b->D * es; }
};
}  // namespace

// the attention patch shifts the ids tensor it was handed in place (qwen2_vl.py:73); the prologue left that to here: one
// launch per chunk, with the last layer's rule - what the reference's loop leaves behind
static int flush_shift_row(const Flush& f) {
    rtk_pivotkv_batch* b = f.b;
    if (!b->shift_row) return RTK_OK;
    int rc = rtk_position_shift(b->shift_row, b->L, last_id(f.layers[f.n - 1]), f.stream);
    if (rc) return rc;
    b->shift_row = nullptr;
    return RTK_OK;
}

// the two matrix passes of every unit the update left to the flush (:260-268)
static int flush_score(const Flush& f) {
    rtk_pivotkv_batch* b = f.b;
    if (!b->batched_passes) return RTK_OK;
    const int n = f.n, L = b->L, D = b->D, Hkv = b->Hkv;
    const int32_t* slots = f.slots;
    std::vector<const void*> masks((size_t)n);
    int i = 0;
    auto in_place = [&](int slot) { return b->q_units && b->q_units[slot] != nullptr; };
    while (i < n) {   // every run of consecutive slots whose queries live alike in one launch per kernel
        int j = i;
        while (j + 1 < n && slots[j + 1] == slots[j] + 1 && in_place(slots[j + 1]) == in_place(slots[i])) ++j;
        const int l0 = slots[i], cnt = j - i + 1;
        bool any = false;
        for (int u = 0; u < cnt; ++u) {
            masks[u] = b->skip_masked ? f.layers[i + u]->mask : nullptr;
            any = any || masks[u];
        }
        // queries scored in place (prologue route): every unit of the run, or none
        const void* const* qu = in_place(l0) ? b->q_units + l0 : nullptr;
        int rc = rtk_pivotkv_score_passes_batched_q(
            (char*)b->score_ws + (size_t)l0 * b->score_ws_stride, b->score_ws_stride, f.reforge() ? f.k_unrot(l0) : nullptr,
            (size_t)Hkv * L * D * f.es, b->partials + (size_t)l0 * b->partial_floats, b->partial_floats, cnt, b->Hq, Hkv, L, D,
            b->score_dtype, (any && b->key_index) ? masks.data() : nullptr,
            (any && b->key_index) ? b->key_index + (size_t)l0 * (L + 1) : nullptr, qu, b->q_stride_h, b->q_stride_l, f.stream);
        if (rc) return rc;
        if (qu)
            for (int u = 0; u < cnt; ++u) b->q_units[l0 + u] = nullptr;
        i = j + 1;
    }
    return RTK_OK;
}

// mask override + top-k + id gather / rescale (:269-295)
static int flush_select(const Flush& f) {
    rtk_pivotkv_batch* b = f.b;
    const int n = f.n, L = b->L, keep = b->keep, P = b->P;
    std::vector<rtk_select_unit> su((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int l = f.slots[i];
        rtk_select_unit& u = su[i];
        u.partial = b->partials + (size_t)l * b->partial_floats;
        u.score = b->score + (size_t)l * L;
        u.mask = f.layers[i]->mask;
        u.pos = P ? b->pos_old + (size_t)l * P * L : nullptr;
        u.keep_idx = b->keep_idx + (size_t)l * keep;
        u.rank = nullptr;
        u.pos_out = P ? b->pos_new + (size_t)l * keep : nullptr;
        u.workspace = (char*)b->sel_ws + (size_t)l * b->sel_ws_stride;
    }
    return rtk_pivotkv_select_batched(su.data(), n, b->Hkv, b->rs_n, b->Hq / b->Hkv, L, keep, P, (int)f.reforge(),
                                      (int64_t)b->slots * keep, b->score_dtype, f.stream);
}

// the eviction scan as one in-place launch: kept K re-rotated (or copied) from k~ to the tail, V (and an un-reforged K)
// compacted inside the tail, ids to the position cache (:278-318)
static int flush_compact(const Flush& f) {
    rtk_pivotkv_batch* b = f.b;
    const int n = f.n, L = b->L, D = b->D, keep = b->keep, P = b->P;
    const bool reforge = f.reforge();
    std::vector<rtk_compact_unit> cu((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int l = f.slots[i];
        rtk_layer_state* ls = f.layers[i];
        const Tail t = tail_of(ls, D, f.es);
        rtk_compact_unit& u = cu[i];
        u.k_src = reforge ? f.k_unrot(l) : nullptr;
        u.k_src_stride_h = (int64_t)L * D;
        u.k_tail = t.k;
        u.k_tail_stride_h = t.stride_h;
        u.v_tail = t.v;
        u.v_tail_stride_h = t.stride_h;
        u.keep_idx = b->keep_idx + (size_t)l * keep;
        if (reforge && P) {
            u.pos_src = b->pos_new + (size_t)l * keep;
            u.pos_src_stride = (int64_t)b->slots * keep;
            u.pos_dst = ls->pos + ls->pos_len;
            u.pos_dst_stride = ls->pos_cap;
        } else {
            u.pos_src = u.pos_dst = nullptr;
            u.pos_src_stride = u.pos_dst_stride = 0;
        }
    }
    const int k_mode = !reforge ? RTK_COMPACT_K_INPLACE : (b->defer_rot ? RTK_COMPACT_K_COPY : RTK_COMPACT_K_ROTATE);
    return rtk_pivotkv_compact_batched(cu.data(), n, b->Hkv, D, keep, reforge ? P : 0, b->dtype, k_mode, b->inv_freq,
                                       b->attention_scaling, b->nsec ? b->sections : nullptr, b->nsec, b->round_mode,
                                       b->compact_sync, (size_t)b->compact_sync_ints, f.stream);
}

// ... or staged: the kept rows gathered into the staging buffers (K re-rotated on the way), then placed at the tail
static int flush_evict_place(const Flush& f) {
    rtk_pivotkv_batch* b = f.b;
    const int n = f.n, L = b->L, D = b->D, Hkv = b->Hkv, keep = b->keep, P = b->P, es = f.es;
    const bool reforge = f.reforge();
    std::vector<rtk_evict_unit> eu((size_t)n);
    std::vector<rtk_place_unit> pl((size_t)2 * n);
    int nc = 0;
    for (int i = 0; i < n; ++i) {
        const int l = f.slots[i];
        rtk_layer_state* ls = f.layers[i];
        const Tail t = tail_of(ls, D, es);
        rtk_evict_unit& u = eu[i];
        u.cos_new = u.sin_new = nullptr;
        const int64_t* kidx = b->keep_idx + (size_t)l * keep;
        auto place = [&](void* stage, char* tail) {   // stage [Hkv, keep, D] -> the tail's first `keep` rows
            pl[nc].stage = stage;
            pl[nc].stage_stride_h_bytes = (int64_t)keep * D * es;
            pl[nc].tail = tail;
            pl[nc].tail_stride_h_bytes = t.stride_h * es;
            pl[nc].keep_idx = kidx;
            ++nc;
        };
        if (reforge) {   // kept K = k~ re-rotated at the NEW ids, straight into the cache (:297-306)
            u.k_src = f.k_unrot(l);
            u.k_src_stride_h = (int64_t)L * D;
            // keep-all chunks of pre-RoPE units: new ids == old ids and k~ == k0, so the tail already holds the result
            // (not with a deferred re-rotation: the cache has to hold the UN-rotated rows)
            // (pre_rope == 2: reference operands - k~ carries the round trip's roundings, the kept row is ITS re-rotation)
            u.k_dst = (b->keep_all && b->pre_rope == 1 && !b->defer_rot) ? nullptr : t.k;
            u.k_dst_stride_h = t.stride_h;
        } else {
            u.k_src = t.k;
            u.k_src_stride_h = t.stride_h;
            if (b->keep_all) {
                u.k_dst = nullptr;
                u.k_dst_stride_h = 0;
            } else {
                u.k_dst = (char*)b->k_stage + (size_t)l * Hkv * keep * D * es;
                u.k_dst_stride_h = (int64_t)keep * D;
                place(u.k_dst, t.k);
            }
        }
        u.v_src = t.v;
        u.v_src_stride_h = t.stride_h;
        if (b->keep_all) {   // every V row already sits where it belongs
            u.v_dst = nullptr;
            u.v_dst_stride_h = 0;
        } else {
            u.v_dst = (char*)b->v_stage + (size_t)l * Hkv * keep * D * es;
            u.v_dst_stride_h = (int64_t)keep * D;
            place(u.v_dst, t.v);
        }
        u.keep_idx = kidx;
        if (reforge && P) {   // bookkeeping (:308-309).  keep-all: the ids x 1.0 are the ids (:288-292)
            u.pos_src = b->keep_all ? b->pos_old + (size_t)l * P * L : b->pos_new + (size_t)l * keep;
            u.pos_src_stride = b->keep_all ? (int64_t)L : (int64_t)b->slots * keep;
            u.pos_dst = ls->pos + ls->pos_len;
            u.pos_dst_stride = ls->pos_cap;
        } else {
            u.pos_src = u.pos_dst = nullptr;
            u.pos_src_stride = u.pos_dst_stride = 0;
        }
    }
    int rc = RTK_OK;
    if (reforge && b->defer_rot)   // un-rotated kept rows + their (provisional) ids; the owner rotates once, later
        rc = rtk_pivotkv_evict_batched(eu.data(), n, Hkv, D, keep, P, b->dtype, 3, f.stream);
    else if (reforge)
        rc = rtk_pivotkv_evict_batched_rope(eu.data(), n, Hkv, D, keep, P, b->dtype, b->inv_freq, b->attention_scaling,
                                            b->nsec ? b->sections : nullptr, b->nsec, b->round_mode, 1, f.stream);
    else if (!b->keep_all)
        rc = rtk_pivotkv_evict_batched(eu.data(), n, Hkv, D, keep, 0, b->dtype, 1, f.stream);
    if (rc || !nc) return rc;
    return rtk_pivotkv_place_batched(pl.data(), nc, Hkv, keep, D, b->dtype, f.stream);
}

// the end of a flush: every layer holds `keep` more rows (and ids), nothing is pending
static void finish_layers(const Flush& f) {
    for (int i = 0; i < f.n; ++i) {
        rtk_layer_state* ls = f.layers[i];
        ls->length += f.b->keep;
        ls->pending = 0;
        ls->pending_keep = 0;
        ls->mask = nullptr;
        if (f.reforge() && f.b->P) ls->pos_len += f.b->keep;
    }
    f.b->pre_rope = 0;
}

extern "C" int rtk_pivotkv_flush(rtk_pivotkv_batch* b, rtk_layer_state* const* layers, const int32_t* slots, int n,
                                 rtk_stream_t stream) {
    int rc = check_batch(b, "rtk_pivotkv_flush");
    if (rc) return rc;
    RTK_CHECK_ARG(layers && slots && n >= 1 && n <= b->slots, "rtk_pivotkv_flush: bad layer list");
    const int L = b->L, keep = b->keep, P = b->P;
    const bool reforge = b->reforge != 0;
    if (reforge && (!b->inv_freq || P == 0 || !b->k_unrot || !b->pos_old || !b->pos_new)) {
        set_error("rtk_pivotkv_flush: pos_embed_reforge needs position ids and an inv_freq rotary (use the per-stage calls)");
        return RTK_EUNSUPPORTED;
    }
    if (!reforge && !b->keep_all && !b->k_stage && !b->compact_sync) {
        set_error("rtk_pivotkv_flush: no K staging buffer");
        return RTK_EINVAL;
    }
    for (int i = 0; i < n; ++i) {
        const rtk_layer_state* ls = layers[i];
        RTK_CHECK_ARG(ls && ls->k && ls->v, "rtk_pivotkv_flush: layer %d: NULL state", i);
        RTK_CHECK_ARG(slots[i] >= 0 && slots[i] < b->slots && (i == 0 || slots[i] > slots[i - 1]),
                      "rtk_pivotkv_flush: slots must be ascending and inside the batch");
        RTK_CHECK_ARG(ls->pending == L && ls->pending_keep == keep && ls->length + L <= ls->cap,
                      "rtk_pivotkv_flush: layer %d has no pending chunk of this batch", i);
        RTK_CHECK_ARG(!(reforge && P) || (ls->pos && ls->pos_len + keep <= ls->pos_cap),
                      "rtk_pivotkv_flush: layer %d: position cache has no room for %d ids", i, keep);
    }
    int es, ve;
    payload_dims(b->dtype, es, ve);
    const Flush f{b, layers, slots, n, es, stream};
    rc = flush_shift_row(f);
    if (!rc && !b->keep_all) rc = flush_score(f);
    if (!rc && !b->keep_all) rc = flush_select(f);
    if (!rc) rc = (b->compact_sync && !b->keep_all) ? flush_compact(f) : flush_evict_place(f);
    if (rc) return rc;
    finish_layers(f);
    return RTK_OK;
}

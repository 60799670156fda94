// score_dma.cuh — the score kernels of the 16-bit dtypes (bf16, fp16 payloads, RTK_BF16_FAST), head_dim 128: the
// production path.  Same two passes as score_f32.cuh (pass 1: row log-sum-exp per key split, pass 2: column sums of
// exp(s - lse) per row split; the statistics' operand in registers as the MFMA B operand), but the streamed tile goes
// HBM/L2 -> LDS by buffer_load ... lds with the XOR swizzle applied to the source address: no staging registers, no
// ds_write pass.  v_mfma_f32_32x32x16_bf16 / _f16, fp32 accumulate (products of 16-bit floats are exact in fp32), base-2
// exponentials.  2 x 16 KiB of dynamic LDS (+ 512 B in pass 2).  Batched over units in blockIdx.y.
//   key_compact_kernel        the live (unmasked) keys of pass 2
//   score_pass1_dma_kernel    raw row sums, a row whose sum left fp32's range is published as NaN ...
//   score_pass1_fixup_kernel  ... and recomputed here with the offset-carrying statistic
//   score_pass2_dma_kernel    column sums over the live keys
// key_compact_kernel is a plain (non-template) kernel: one translation unit includes this file.
#pragma once
#include <type_traits>

#include "score_mfma.cuh"

namespace rtk {

// Shape of the kernels (HISTORY.md §4 has the same-box A/B numbers behind every choice): two 32-row register blocks per
// wave (every A fragment read from LDS feeds two MFMAs on independent accumulators: half the fragment reads, DMA issues,
// barriers and waits per MFMA; ~160 VGPRs -> 3 waves per SIMD), the next tile's DMA pieces issued inside block 0's
// softmax, all fragment reads of a block ahead of its MFMAs which alternate strictly between the two accumulators, a last
// tile that is at most half full on the one-block body, pass 2's normalisers by LDS-DMA from wave 0.
constexpr int P1_NB = 2;   // 32-row register blocks per wave, pass 1
constexpr int P2_NB = 2;   // 32-key register blocks per wave, pass 2

// ------------------------------------------------------------------------------------------------
// Live keys of pass 2.  The reference overwrites the score of every key-patch token with 1.0 after the scoring
// (`score.masked_fill_(keypatches_mask_chunk, 1.0)`, longvideo_cache.py:272-274): the column masses of those tokens are
// computed and thrown away.  A key's column mass depends on its own column only, so pass 2 - whose REGISTER operand is
// the keys - can run on the compacted list of unmasked keys and leave the masked columns unwritten: identical bits for
// every column anybody reads, (mask rate) x pass 2 less work (the mask is DPSelect's peak flag: about a third of the
// tokens).  Pass 1 is untouched: the row normalisers are sums over ALL keys.
//   key_index[unit][0 .. n)  ascending indices of the unit's unmasked tokens, key_index[unit][L] = n  (-1: no mask, identity)
// One 1024-thread workgroup per unit: ordered compaction by a block scan of per-thread counts.
// ------------------------------------------------------------------------------------------------
// Where the queries of the units of a batched launch live.  row_pitch == 0: the packed un-rotated copies inside the
// units' score workspaces ([Hq, L, 128] at q + unit * q_unit_bytes).  Else: per-unit base pointers of tensors the caller
// keeps alive - the pre-RoPE projections themselves (the prologue route scores q0 as it is, so no copy is made),
// element (h, i, :) at unit[u] + h * head_stride + i * row_pitch bytes.
constexpr int MAX_Q_UNITS = 32;
struct QView {
    const char* unit[MAX_Q_UNITS];
    int head_stride, row_pitch;
};
constexpr int MAX_MASK_UNITS = 64;
struct KeyMasks {
    const uint8_t* m[MAX_MASK_UNITS];
};
__global__ __launch_bounds__(1024) void key_compact_kernel(KeyMasks masks, int L, int* __restrict__ key_index) {
    __shared__ int wsum[16];
    const uint8_t* __restrict__ mk = masks.m[blockIdx.x];
    int* __restrict__ out = key_index + (size_t)blockIdx.x * (L + 1);
    if (!mk) {
        if (threadIdx.x == 0) out[L] = -1;
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (L + 1023) / 1024;
    const int b = tid * per, e = min(L, b + per);
    int cnt = 0;
    for (int j = b; j < e; ++j) cnt += mk[j] == 0;
    int inc = cnt;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int v = wsum[w];
        base += w < wv ? v : 0;
        total += v;
    }
    int at = base + inc - cnt;
    for (int j = b; j < e; ++j)
        if (mk[j] == 0) out[at++] = j;
    if (tid == 0) out[L] = total;
}

// online max / sum of one query row over the keys this lane sees, one 32-key block at a time (exact modes' fix-up launch,
// log2 domain)
struct RowStatB {
    float m, sum, off;   // off = -m * c2, the exponent offset of the last rescale
    __device__ __forceinline__ void init() { m = -INFINITY; sum = 0.f; off = INFINITY; }
    // Lazy: the 16 exponentials are taken against the offset of the LAST rescale (no max over the block, no
    // rescale of the running sum); only when some lane's block sum is not a finite number below 2^96 - a key beat the
    // stale offset by ~96 binary orders, or nothing has been seen yet (m = -inf makes the offset +inf) - the whole wave
    // takes the ordinary online step for this block.  Any offset gives the same sum mathematically and fp32 keeps its
    // relative precision over that range, so the result is as exact as a max per block (not bitwise equal to it).
    // Saves ~13 of the ~64 VALU instructions per 32 x 32 block in a kernel that is bound by instruction issue.
    template <bool RAGGED>
    __device__ __forceinline__ void update(f32x16& a, int j0, int j_end, int hf, float c2) {
        if (RAGGED) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row(r, hf) >= j_end) a[r] = -INFINITY;
        }
        float add = __builtin_amdgcn_exp2f(fmaf(a[0], c2, off));   // (0 + e0 would cost an instruction: -0 semantics)
#pragma unroll
        for (int r = 1; r < 16; ++r) add += __builtin_amdgcn_exp2f(fmaf(a[r], c2, off));
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(add < 0x1p96f)) == 0, 1)) {
            sum += add;
            return;
        }
        const float mn = fmaxf(m, max16(a));
        if (mn == -INFINITY) return;   // no key seen yet on this lane and none in this block
        const float nb2 = -mn * c2;
        add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) add += __builtin_amdgcn_exp2f(fmaf(a[r], c2, nb2));
        sum = sum * __builtin_amdgcn_exp2f((m - mn) * c2) + add;
        m = mn;
        off = nb2;
    }
    __device__ __forceinline__ float finish(float c2) const {
        const float m2 = __shfl_xor(m, 32, WAVE), s2 = __shfl_xor(sum, 32, WAVE);
        const float mm = fmaxf(m, m2);
        if (mm == -INFINITY) return -INFINITY;
        const float tot = sum * __builtin_amdgcn_exp2f((m - mm) * c2) + s2 * __builtin_amdgcn_exp2f((m2 - mm) * c2);
        return mm * c2 + __builtin_amdgcn_logf(tot);  // v_log_f32 = log2
    }
};

// RTK_BF16_FAST pass 1: the accumulators ARE base-2 logits (q~ was pre-scaled), so a logit needs no multiply.
// RowStatR - the production form - adds exp2(logit) to the row sum with NO offset and no test: two instructions per
// logit, the minimum.  That is exact whenever the row's sum stays inside fp32's comfortable range; a row whose sum
// left it (a logit beyond ~2^7 in base 2 -> inf, or every logit below ~-60 -> precision lost in subnormals) is
// detected ONCE, at the end - inf and NaN are sticky in a sum of non-negative terms - and published as NaN; the
// fix-up launch that follows (score_pass1_fixup_kernel) recomputes exactly the row tiles that own a NaN with
// RowStatF, the offset-carrying form.  Deterministic: which rows take which path depends on the data only.
struct RowStatR {
    float sum;
    __device__ __forceinline__ void init() { sum = 0.f; }
    template <bool RAGGED>
    __device__ __forceinline__ void update(f32x16& a, int j0, int j_end, int hf) {
        if (RAGGED) {  // keys >= j_end do not exist
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row(r, hf) >= j_end) a[r] = -INFINITY;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(a[r]);
    }
    __device__ __forceinline__ float finish() const {
        const float tot = sum + __shfl_xor(sum, 32, WAVE);
        const bool fine = tot < 0x1p120f && tot > 0x1p-60f;      // false for inf and NaN as well
        return fine ? __builtin_amdgcn_logf(tot) : __builtin_nanf("");   // v_log_f32 = log2
    }
};

// The same for the exact modes (bf16 / fp16 payloads, un-scaled operands): exp2(dot * c2) added to the row sum, no offset,
// no per-block test - one multiply more than RowStatR, but none of RowStatB's bookkeeping (the lazy test costs a compare,
// a ballot and a branch per 32-key block, and the offset a register): same end-of-row check, same fix-up launch, which
// then runs RowStatB.
struct RowStatRX {
    float sum;
    __device__ __forceinline__ void init() { sum = 0.f; }
    template <bool RAGGED>
    __device__ __forceinline__ void update(f32x16& a, int j0, int j_end, int hf, float c2) {
        if (RAGGED) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row(r, hf) >= j_end) a[r] = -INFINITY;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(a[r] * c2);
    }
    __device__ __forceinline__ float finish() const {
        const float tot = sum + __shfl_xor(sum, 32, WAVE);
        const bool fine = tot < 0x1p120f && tot > 0x1p-60f;
        return fine ? __builtin_amdgcn_logf(tot) : __builtin_nanf("");
    }
};

// The robust form (fix-up launch only): sum = sum_j exp2(s_j + off) over the keys this lane has seen, i.e. the true
// total is sum * 2^-off.  Lazy like RowStatB: the offset is that of the last rescale; when some lane's block sum is
// not a finite number below 2^96, or nothing has been seen yet (`primed`, wave-uniform), the wave re-bases on the
// block's maximum.
struct RowStatF {
    float sum, off;
    __device__ __forceinline__ void init() { sum = 0.f; off = 0.f; }
    template <bool RAGGED>
    __device__ __forceinline__ void update(f32x16& a, int j0, int j_end, int hf, bool& primed) {
        if (RAGGED) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row(r, hf) >= j_end) a[r] = -INFINITY;
        }
        if (primed) {
            float add = __builtin_amdgcn_exp2f(a[0] + off);
#pragma unroll
            for (int r = 1; r < 16; ++r) add += __builtin_amdgcn_exp2f(a[r] + off);
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(add < 0x1p96f)) == 0, 1)) {
                sum += add;
                return;
            }
        }
        const float mx = max16(a);
        // a lane without a key in the block (ragged tail: mx = -inf) keeps its offset: add = 0, sum unchanged
        const float noff = (mx == -INFINITY) ? off : (primed ? -fmaxf(mx, -off) : -mx);
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) add += __builtin_amdgcn_exp2f(a[r] + noff);
        // the first re-base starts from sum = 0 with a meaningless offset (0 * 2^(noff - 0) may be 0 * inf); later ones
        // only ever lower the offset (noff <= off), so the rescale factor is <= 1
        sum = primed ? sum * __builtin_amdgcn_exp2f(noff - off) + add : add;
        off = noff;
        primed = true;
    }
    __device__ __forceinline__ float finish() const {
        const float m1 = sum > 0.f ? -off : -INFINITY;   // a half that saw no key (ragged tail) carries no scale
        const float m2 = __shfl_xor(m1, 32, WAVE), s2 = __shfl_xor(sum, 32, WAVE);
        const float mm = fmaxf(m1, m2);
        if (mm == -INFINITY) return -INFINITY;            // an empty row
        const float tot = sum * __builtin_amdgcn_exp2f(m1 - mm) + s2 * __builtin_amdgcn_exp2f(m2 - mm);
        return mm + __builtin_amdgcn_logf(tot);
    }
};

// ------------------------------------------------------------------------------------------------
// pass 2, LDS-DMA form (bf16, the production kernel): the decomposition of score_pass2_kernel without its in-wave
// software pipeline (one 32-row block of logits live at a time: ~95 VGPRs -> 4 waves per SIMD), and the streamed
// query tile goes HBM/L2 -> LDS directly (buffer_load_dwordx4 ... lds): no staging registers, no ds_write pass.  A wave's DMA instruction fills
// 1 KiB of LDS linearly (lane * 16 B), so the XOR swizzle of the tile is applied to the SOURCE address:
// LDS position p of row r receives chunk p ^ (r & 15), the same involution the fragment reads apply.
// NB = 32-key register blocks per wave (NB = 2: every A fragment read from LDS feeds two MFMAs).
// ------------------------------------------------------------------------------------------------
// The work of one workgroup: NB x 32 keys per wave starting at key j_base + wid * 32 * NB, the query rows of split rs.
template <int NB, bool FAST = false, bool F16 = false>   // F16: exact softmax on fp16 payloads (RTK_F16)
__device__ __forceinline__ void score_pass2_dma_body(const char* __restrict__ q, const char* __restrict__ k,
                                                     const float* __restrict__ lse, int Hq, int Hkv, int L,
                                                     int rows_per_split, int RS, float* __restrict__ partial, int j_base,
                                                     int g, int rs, const int* __restrict__ kidx, int Lk, int q_hs,
                                                     int q_pitch) {
    // q_hs / q_pitch: bytes between the heads / rows of q (packed copy: L * 256 and 256)
    // kidx / Lk: the unit's live keys (ascending token indices, Lk of them; kidx == NULL: all L tokens, Lk == L).  j_base
    // and the wave's key offsets count positions of THAT list; a position's token index names the k~ row it loads and
    // the column of `partial` it writes.
    constexpr int DT = RTK_BF16;
    using M = MM<DT>;
    using T = Tile<DT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lse_s = (float*)(smem + 2 * T::BYTES);  // [2][TILE_ROWS]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), hf = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int G = Hq / Hkv;
    const int j0 = j_base + wid * (32 * NB);
    const char* kg = k + (size_t)g * L * HD * M::ESIZE;
    const int ib = rs * rows_per_split, ie = min(L, ib + rows_per_split);
    const int nrows = ie - ib;
    const int tiles_per_head = (nrows + TILE_ROWS - 1) / TILE_ROWS;
    const int ntiles = tiles_per_head * G;

    int frag_off[M::NREG];
    {
        const int row = lane & 31;
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) frag_off[r] = row * T::ROWB + ((M::chunk_of(r, hf) ^ (row & 15)) * 16);
    }
    u32x4 kf[NB][M::NREG];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int jp = j0 + 32 * nb + (lane & 31);           // position in the live-key list
        const bool ok = jp < Lk;
        const int row = ok ? (kidx ? kidx[jp] : jp) : 0;      // token index = k~ row
        const u32x4* p = (const u32x4*)(kg + (size_t)row * HD * M::ESIZE);
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) kf[nb][r] = ok ? p[M::chunk_of(r, hf)] : u32x4{0, 0, 0, 0};
    }
    const float c2 = 1.4426950408889634f / sqrtf((float)HD);
    float col[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) col[nb] = 0.f;

    // DMA addressing: piece P = 4u + wid (u = 0..3) covers tile rows 4P .. 4P+3; this lane fills position
    // (lane & 15) of row 4P + (lane >> 4) with source chunk (lane & 15) ^ (row & 15)
    const int drow = 4 * wid + (lane >> 4);                                        // row inside a 16-row group
    const int dvoff = drow * q_pitch + (((lane & 15) ^ (drow & 15)) * 16);           // + u * 16 rows via soffset
    // (a row past L lies past the buffer for a strided projection and inside the next head for the packed copy: zeros
    // or finite values, either way met by lse = +inf)
    const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)q, 0, (Hq - 1) * q_hs + (L - 1) * q_pitch + HD * M::ESIZE, 0x00020000);
    const __amdgpu_buffer_rsrc_t lrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)lse, 0, Hq * L * 4, 0x00020000);
    const bool lse_dma = (nrows % TILE_ROWS == 0);   // uniform: no row of a tile lies past the split
    float lstA = 0.f;
    int nt = 0;
    const int last_row = Hq * L - 1;
    int nrow0 = (g * G) * L + ib;           // row of lse [Hq, L] the cursor's head starts its split at
    int qoff0 = (g * G) * q_hs + ib * q_pitch;   // byte offset of that row in q
    // issues the DMA of the cursor tile into LDS buffer `b`, fetches this thread's lse element, advances the cursor
#define RTK_DMA_ISSUE(b)                                                                                  \
    {                                                                                                     \
        const int qb__ = qoff0 + nt * TILE_ROWS * q_pitch;                                                \
        _Pragma("unroll")                                                                                 \
        for (int u = 0; u < 4; ++u)                                                                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                     \
                qrsrc, (void __attribute__((address_space(3)))*)(smem + (b) * T::BYTES + (4 * u + wid) * 1024), 16, \
                dvoff, qb__ + 16 * u * q_pitch, 0, 0);                                                    \
        const int r__ = nt * TILE_ROWS + (tid & (TILE_ROWS - 1));                                         \
        lstA = (r__ < nrows) ? lse[min(nrow0 + r__, last_row)] : (FAST ? -INFINITY : INFINITY);           \
        const bool wrap__ = (nt + 1 == tiles_per_head);                                                   \
        nt = wrap__ ? 0 : nt + 1;                                                                         \
        nrow0 += wrap__ ? L : 0;                                                                          \
        qoff0 += wrap__ ? q_hs : 0;                                                                       \
    }
#define RTK_DMA_PIECES(b, rb, U0, U1)                                                                     \
    {                                                                                                     \
        _Pragma("unroll")                                                                                 \
        for (int u = U0; u < U1; ++u)                                                                     \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                     \
                qrsrc, (void __attribute__((address_space(3)))*)(smem + (b) * T::BYTES + (4 * u + wid) * 1024), 16, \
                dvoff, (rb) + 16 * u * q_pitch, 0, 0);                                                    \
    }
#define RTK_DMA_TAIL(b)                                                                                   \
    {                                                                                                     \
        const int r__ = nt * TILE_ROWS + (tid & (TILE_ROWS - 1));                                         \
        if (lse_dma) { /* whole tiles only: the 64 normalisers go HBM/L2 -> LDS like the tile itself */   \
            if (wid == 0)                                                                                 \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                 \
                    lrsrc, (void __attribute__((address_space(3)))*)(lse_s + (b) * TILE_ROWS), 4, lane * 4, \
                    (nrow0 + nt * TILE_ROWS) * 4, 0, 0);                                                  \
        } else if (wid == 0) lstA = (r__ < nrows) ? lse[min(nrow0 + r__, last_row)] : (FAST ? -INFINITY : INFINITY); \
        const bool wrap__ = (nt + 1 == tiles_per_head);                                                   \
        nt = wrap__ ? 0 : nt + 1;                                                                         \
        nrow0 += wrap__ ? L : 0;                                                                          \
        qoff0 += wrap__ ? q_hs : 0;                                                                       \
    }
#define RTK_DMA_STEP(BUF, ISSUE)                                                                          \
    {                                                                                                     \
        constexpr int buf = BUF;                                                                          \
        const char* cur = smem + buf * T::BYTES;                                                          \
        const float* lcur = lse_s + buf * TILE_ROWS;                                                      \
        const int rb__ = qoff0 + nt * TILE_ROWS * q_pitch;   /* byte offset of the next tile's rows */    \
        if constexpr (ISSUE) RTK_DMA_TAIL(buf ^ 1)                                  \
        _Pragma("unroll")                                                                                 \
        for (int blk = 0; blk < 2; ++blk) {                                                               \
            u32x4 a[M::NREG];                                                                             \
            float ls[16];                                                                                 \
            _Pragma("unroll")                                                                             \
            for (int r = 0; r < M::NREG; ++r) a[r] = *(const u32x4*)(cur + blk * 32 * T::ROWB + frag_off[r]); \
            load_ls(ls, lcur, blk, hf);                                                                   \
            f32x16 acc[NB], lsv;                                                                          \
            _Pragma("unroll")                                                                             \
            for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x16{0};                                          \
            if constexpr (FAST) { /* the accumulator chains start from -lse (what `ls` holds in this mode) */ \
                _Pragma("unroll")                                                                         \
                for (int r = 0; r < 16; ++r) lsv[r] = ls[r];                                              \
            }                                                                                             \
            __builtin_amdgcn_sched_barrier(0);                                        \
            _Pragma("unroll")                                                                             \
            for (int r = 0; r < M::NREG; ++r) {                                                           \
                _Pragma("unroll")                                                                         \
                for (int nb = 0; nb < NB; ++nb) {                                                         \
                    if constexpr (FAST) mma16<true>(acc[nb], a[r], kf[nb][r], r == 0 ? lsv : acc[nb]);   \
                    else if constexpr (F16) mma16<true>(acc[nb], a[r], kf[nb][r], acc[nb]);               \
                    else M::mma(acc[nb], a[r], kf[nb][r]);                                                \
                    __builtin_amdgcn_sched_group_barrier(SGB_MFMA, 1, 0);            \
                }                                                                                         \
            }                                                                                             \
            __builtin_amdgcn_sched_barrier(0);                                        \
            _Pragma("unroll")                                                                             \
            for (int nb = 0; nb < NB; ++nb) {                                                             \
                if constexpr (FAST) {                                                                     \
                    _Pragma("unroll")                                                                     \
                    for (int r = 0; r < 16; ++r) col[nb] += __builtin_amdgcn_exp2f(acc[nb][r]);           \
                } else colsum_block(col[nb], acc[nb], ls, c2);                                            \
                asm volatile("" : "+v"(col[nb]) : : "memory");                                            \
                __builtin_amdgcn_sched_barrier(0);                                                        \
                if constexpr (ISSUE) {                                              \
                    if (blk == 0) {                                                                       \
                        if (NB == 1) RTK_DMA_PIECES(buf ^ 1, rb__, 0, 4)                                  \
                        else if (nb == 0) RTK_DMA_PIECES(buf ^ 1, rb__, 0, 2)                             \
                        else if (nb == 1) RTK_DMA_PIECES(buf ^ 1, rb__, 2, 4)                             \
                        __builtin_amdgcn_sched_barrier(0);                                                \
                    }                                                                                     \
                }                                                                                         \
            }                                                                                             \
        }                                                                                                 \
        if constexpr (ISSUE) {                                                                            \
            if (!lse_dma && tid < TILE_ROWS) lse_s[(buf ^ 1) * TILE_ROWS + tid] = lstA;                   \
        }                                                                                                 \
        __syncthreads(); /* drains the DMA (vmcnt(0)) and the LDS reads of this tile */                   \
    }
    RTK_DMA_ISSUE(0)
    if (tid < TILE_ROWS) lse_s[tid] = lstA;
    __syncthreads();
    int it = 0;
    for (; it + 2 < ntiles; it += 2) {
        RTK_DMA_STEP(0, true)
        RTK_DMA_STEP(1, true)
    }
    if (it < ntiles) {
        if (it + 1 < ntiles) RTK_DMA_STEP(0, true)
        else RTK_DMA_STEP(0, false)
        ++it;
    }
    if (it < ntiles) {
        RTK_DMA_STEP(1, false)
        ++it;
    }
#undef RTK_DMA_STEP
#undef RTK_DMA_ISSUE
    int lane_late = lane;
    asm volatile("" : "+v"(lane_late));   // the output address is formed here, not carried (and spilled) through the loop
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const float c = col[nb] + __shfl_xor(col[nb], 32, WAVE);
        const int jp = j0 + 32 * nb + (lane_late & 31);
        if (lane_late < 32 && jp < Lk) partial[((size_t)g * RS + rs) * L + (kidx ? kidx[jp] : jp)] = c;
    }
}

// blockIdx.x -> (key tile bx, KV head g, row split rs), blockIdx.y = unit of a batched launch.  A key tile is
// REG_ROWS * NB keys (4 waves x NB x 32).  When the LAST tile holds at most half of that (L = 6272 = 24.5 tiles of 256),
// its workgroups run the one-block body on 32 keys per wave instead of leaving two of four waves without a key: the
// tile costs half the MFMAs (2 % of the launch's arithmetic was spent on keys past L).
template <int NB, bool FAST = false, bool F16 = false>
__global__ __launch_bounds__(SC_BLOCK, (NB == 1 ? 4 : (NB == 2 ? 3 : (NB == 3 ? 2 : 2)))) void score_pass2_dma_kernel(
    const char* __restrict__ q, const char* __restrict__ k, const float* __restrict__ lse, int Hq, int Hkv, int L,
    int rows_per_split, int col_tiles, int RS, int xcd_remap, float* __restrict__ partial, size_t q_unit_bytes,
    size_t k_unit_bytes, size_t lse_unit_floats, size_t part_unit_floats, const int* __restrict__ key_index, QView qv) {
    const int q_hs = qv.row_pitch ? qv.head_stride : L * HD * 2, q_pitch = qv.row_pitch ? qv.row_pitch : HD * 2;
    q = qv.row_pitch ? qv.unit[blockIdx.y] : q + blockIdx.y * q_unit_bytes;
    k += blockIdx.y * k_unit_bytes;
    lse += blockIdx.y * lse_unit_floats;
    partial += blockIdx.y * part_unit_floats;
    // the unit's live keys (key_compact_kernel); a workgroup whose key tile lies past them has nothing to do
    const int* kidx = nullptr;
    int Lk = L;
    if (key_index) {
        const int* ki = key_index + (size_t)blockIdx.y * (L + 1);
        const int n = ki[L];
        if (n >= 0) {
            kidx = ki;
            Lk = n;
        }
    }
    int bx, g, rs;
    {
        int grp;
        if (xcd_remap) {
            const int xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
            grp = xcd + NXCD * (slot / col_tiles);
            bx = slot % col_tiles;
        } else {
            grp = blockIdx.x / col_tiles;
            bx = blockIdx.x % col_tiles;
        }
        g = grp % Hkv;
        rs = grp / Hkv;
    }
    const int j_base = bx * (REG_ROWS * NB);
    if (j_base >= Lk) return;
    if constexpr (NB == 2) {
        if (Lk - j_base <= REG_ROWS) {   // uniform per workgroup
            score_pass2_dma_body<1, FAST, F16>(q, k, lse, Hq, Hkv, L, rows_per_split, RS, partial, j_base, g, rs, kidx, Lk, q_hs,
                                               q_pitch);
            return;
        }
    }
    score_pass2_dma_body<NB, FAST, F16>(q, k, lse, Hq, Hkv, L, rows_per_split, RS, partial, j_base, g, rs, kidx, Lk, q_hs, q_pitch);
}

// ------------------------------------------------------------------------------------------------
// pass 1, LDS-DMA form (bf16): same decomposition as score_pass1_kernel (32 query rows per wave in
// registers, 64-key tiles streamed), with the key tile DMA'd straight into the swizzled LDS image and one
// 32-key block in flight per wave (~100 VGPRs -> 4 waves per SIMD).
// ------------------------------------------------------------------------------------------------
// The work of one workgroup: NB x 32 query rows of head h per wave starting at row i_base + wid * 32 * NB, key split ks.
// MODE is a set of flags: P1_F16 = the operands are fp16 (fast mode, fp16 payloads), P1_SCALED = q~ was pre-scaled by
// log2(e)/sqrt(D) (fast mode: the accumulators are base-2 logits), P1_RAW = plain row sums checked once at the end
// (a fix-up launch with the same flags minus P1_RAW follows).  Statistic: RAW ? (SCALED ? RowStatR : RowStatRX)
//                                                                              : (SCALED ? RowStatF : RowStatB).
constexpr int P1_F16 = 1, P1_SCALED = 2, P1_RAW = 4;
template <int NB, int MODE>
__device__ __forceinline__ void score_pass1_dma_body(const char* __restrict__ q, const char* __restrict__ k, int Hq, int Hkv,
                                                     int L, int keys_per_split, float* __restrict__ lse_part, int i_base, int h,
                                                     int ks, int neg_out, int q_hs, int q_pitch) {
    constexpr int DT = RTK_BF16;
    using M = MM<DT>;
    using T = Tile<DT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), hf = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int G = Hq / Hkv;
    const int g = h / G;
    const int i0 = i_base + wid * (32 * NB);   // this wave's NB x 32 query rows
    // A wave whose rows all lie past L (a last tile that is between half and three quarters full) keeps its DMA pieces and
    // barriers but skips the MFMAs and the softmax; wave-uniform.  (A last tile that is at most half full runs the
    // one-block body instead, see score_pass1_dma_kernel.)
    const bool live = __builtin_amdgcn_readfirstlane(i0) < L;
    const int jb = ks * keys_per_split, je = min(L, jb + keys_per_split);
    const int nkeys = je - jb;
    const int nfull = nkeys / TILE_ROWS;
    const int ntiles = (nkeys + TILE_ROWS - 1) / TILE_ROWS;
    u32x4 qf[NB][M::NREG];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) load_reg_frag<DT>(q + (size_t)h * q_hs, i0 + 32 * nb, L, lane, qf[nb], q_pitch);
    int frag_off[M::NREG];
    {
        const int row = lane & 31;
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) frag_off[r] = row * T::ROWB + ((M::chunk_of(r, hf) ^ (row & 15)) * 16);
    }
    const float c2 = 1.4426950408889634f / sqrtf((float)HD);
    constexpr bool F16OPS = (MODE & P1_F16) != 0, SCALED = (MODE & P1_SCALED) != 0, RAW = (MODE & P1_RAW) != 0;
    using Stat = std::conditional_t<RAW, std::conditional_t<SCALED, RowStatR, RowStatRX>,
                                    std::conditional_t<SCALED, RowStatF, RowStatB>>;
    Stat rs[NB];
    bool primed[NB];       // RowStatF: has this wave re-based its rows yet?  (wave-uniform)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        rs[nb].init();
        primed[nb] = false;
    }
    const int drow = 4 * wid + (lane >> 4);
    const int dvoff = drow * T::ROWB + (((lane & 15) ^ (drow & 15)) * 16);
    const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(k + (size_t)g * L * HD * M::ESIZE), 0, L * HD * M::ESIZE, 0x00020000);
#define RTK_DMA1_ISSUE(t, b)                                                                              \
    {                                                                                                     \
        _Pragma("unroll")                                                                                 \
        for (int u = 0; u < 4; ++u)                                                                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                     \
                krsrc, (void __attribute__((address_space(3)))*)(smem + (b) * T::BYTES + (4 * u + wid) * 1024), 16, \
                dvoff, (jb + (t) * TILE_ROWS + 16 * u) * T::ROWB, 0, 0);                                  \
    }
#define RTK_DMA1_PIECES(t, b, U0, U1)                                                                     \
    {                                                                                                     \
        _Pragma("unroll")                                                                                 \
        for (int u = U0; u < U1; ++u)                                                                     \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                     \
                krsrc, (void __attribute__((address_space(3)))*)(smem + (b) * T::BYTES + (4 * u + wid) * 1024), 16, \
                dvoff, (jb + (t) * TILE_ROWS + 16 * u) * T::ROWB, 0, 0);                                  \
    }
#define RTK_DMA1_STEP(JT, BUF, ISSUE, RAG)                                                                \
    {                                                                                                     \
        constexpr int buf = BUF;                                                                          \
        const char* cur = smem + buf * T::BYTES;                                                          \
        if (!live) { /* this wave's query rows lie past L: it only moves its share of the next tile */    \
            if constexpr (ISSUE) RTK_DMA1_PIECES((JT) + 1, buf ^ 1, 0, 4)           \
        } else {                                                                                          \
        _Pragma("unroll")                                                                                 \
        for (int blk = 0; blk < 2; ++blk) {                                                               \
            u32x4 a[M::NREG];                                                                             \
            _Pragma("unroll")                                                                             \
            for (int r = 0; r < M::NREG; ++r) a[r] = *(const u32x4*)(cur + blk * 32 * T::ROWB + frag_off[r]); \
            f32x16 acc[NB];                                                                               \
            _Pragma("unroll")                                                                             \
            for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x16{0};                                          \
            __builtin_amdgcn_sched_barrier(0);                                        \
            _Pragma("unroll")                                                                             \
            for (int r = 0; r < M::NREG; ++r) {                                                           \
                _Pragma("unroll")                                                                         \
                for (int nb = 0; nb < NB; ++nb) {                                                         \
                    if constexpr (F16OPS) mma16<true>(acc[nb], a[r], qf[nb][r], acc[nb]);                 \
                    else M::mma(acc[nb], a[r], qf[nb][r]);                                                \
                    __builtin_amdgcn_sched_group_barrier(SGB_MFMA, 1, 0);            \
                }                                                                                         \
            }                                                                                             \
            __builtin_amdgcn_sched_barrier(0);                                        \
            _Pragma("unroll")                                                                             \
            for (int nb = 0; nb < NB; ++nb) {                                                             \
                if constexpr (RAW && SCALED) {                                                            \
                    rs[nb].template update<RAG>(acc[nb], (JT) * TILE_ROWS + 32 * blk, nkeys, hf);         \
                    asm volatile("" : "+v"(rs[nb].sum) : : "memory");                                     \
                } else if constexpr (RAW) {                                                               \
                    rs[nb].template update<RAG>(acc[nb], (JT) * TILE_ROWS + 32 * blk, nkeys, hf, c2);     \
                    asm volatile("" : "+v"(rs[nb].sum) : : "memory");                                     \
                } else if constexpr (SCALED) {                                                            \
                    rs[nb].template update<RAG>(acc[nb], (JT) * TILE_ROWS + 32 * blk, nkeys, hf, primed[nb]); \
                    asm volatile("" : "+v"(rs[nb].sum), "+v"(rs[nb].off) : : "memory");                   \
                } else {                                                                                  \
                rs[nb].template update<RAG>(acc[nb], (JT) * TILE_ROWS + 32 * blk, nkeys, hf, c2);         \
                asm volatile("" : "+v"(rs[nb].sum), "+v"(rs[nb].m) : : "memory");                         \
                }                                                                                         \
                __builtin_amdgcn_sched_barrier(0);                                                        \
                if constexpr (ISSUE) {   /* next tile's DMA pieces inside block 0's softmax */ \
                    if (blk == 0) {                                                                       \
                        if (NB == 1) RTK_DMA1_PIECES((JT) + 1, buf ^ 1, 0, 4)                             \
                        else if (nb == 0) RTK_DMA1_PIECES((JT) + 1, buf ^ 1, 0, 2)                        \
                        else if (nb == 1) RTK_DMA1_PIECES((JT) + 1, buf ^ 1, 2, 4)                        \
                        __builtin_amdgcn_sched_barrier(0);                                                \
                    }                                                                                     \
                }                                                                                         \
            }                                                                                             \
        }                                                                                                 \
        }                                                                                                 \
        __syncthreads(); /* drains the DMA (vmcnt(0)) and the LDS reads of this tile */                   \
    }
    RTK_DMA1_ISSUE(0, 0)
    __syncthreads();
    int jt = 0;
    for (; jt + 2 < nfull; jt += 2) {   // both tiles full, and a tile jt + 2 exists
        RTK_DMA1_STEP(jt, 0, true, false)
        RTK_DMA1_STEP(jt + 1, 1, true, false)
    }
    // at most three tiles left (jt even => buffer parity static); only the last one can be ragged
#define RTK_DMA1_TAIL(PAR)                                                     \
    if (jt < ntiles) {                                                         \
        if (jt + 1 < ntiles) {                                                 \
            if (jt < nfull) RTK_DMA1_STEP(jt, PAR, true, false)                \
            else RTK_DMA1_STEP(jt, PAR, true, true)                            \
        } else {                                                               \
            if (jt < nfull) RTK_DMA1_STEP(jt, PAR, false, false)               \
            else RTK_DMA1_STEP(jt, PAR, false, true)                           \
        }                                                                      \
        ++jt;                                                                  \
    }
    RTK_DMA1_TAIL(0)
    RTK_DMA1_TAIL(1)
    RTK_DMA1_TAIL(0)
#undef RTK_DMA1_TAIL
#undef RTK_DMA1_STEP
#undef RTK_DMA1_PIECES
#undef RTK_DMA1_ISSUE
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        float out;
        if constexpr (RAW || SCALED) out = rs[nb].finish();
        else out = rs[nb].finish(c2);
        const int i = i0 + 32 * nb + (lane & 31);
        if (hf == 0 && i < L) lse_part[((size_t)ks * Hq + h) * L + i] = neg_out ? -out : out;
    }
}

// blockIdx.x -> (row tile bx, head h, key split ks), blockIdx.y = (layer, chunk) unit of a batched launch: same shapes,
// operands one unit stride apart.  Like pass 2, a last row tile that is at most half full (L = 6272 = 24.5 tiles) runs the
// one-block body on 32 rows per wave.
template <int NB, int MODE>
__global__ __launch_bounds__(SC_BLOCK, (NB == 1 ? 4 : 3)) void score_pass1_dma_kernel(
    const char* __restrict__ q, const char* __restrict__ k, int Hq, int Hkv, int L, int keys_per_split, int row_tiles,
    int xcd_remap, float* __restrict__ lse_part, size_t q_unit_bytes, size_t k_unit_bytes, size_t lse_unit_floats,
    int neg_out, QView qv) {
    const int q_hs = qv.row_pitch ? qv.head_stride : L * HD * 2, q_pitch = qv.row_pitch ? qv.row_pitch : HD * 2;
    q = qv.row_pitch ? qv.unit[blockIdx.y] : q + blockIdx.y * q_unit_bytes;
    k += blockIdx.y * k_unit_bytes;
    lse_part += blockIdx.y * lse_unit_floats;
    const int G = Hq / Hkv;
    int bx, h, ks;
    {
        const int per_group = row_tiles * G;
        int grp, w;
        if (xcd_remap) {
            const int xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
            grp = xcd + NXCD * (slot / per_group);
            w = slot % per_group;
        } else {
            grp = blockIdx.x / per_group;
            w = blockIdx.x % per_group;
        }
        ks = grp / Hkv;
        h = (grp % Hkv) * G + w / row_tiles;
        bx = w % row_tiles;
    }
    const int i_base = bx * (REG_ROWS * NB);
    if constexpr (NB == 2) {
        if (L - i_base <= REG_ROWS) {   // uniform per workgroup
            score_pass1_dma_body<1, MODE>(q, k, Hq, Hkv, L, keys_per_split, lse_part, i_base, h, ks, neg_out, q_hs, q_pitch);
            return;
        }
    }
    score_pass1_dma_body<NB, MODE>(q, k, Hq, Hkv, L, keys_per_split, lse_part, i_base, h, ks, neg_out, q_hs, q_pitch);
}

// RTK_BF16_FAST fix-up launch: the row tiles whose plain sums left fp32's range (published as NaN by RowStatR) are
// recomputed with the offset-carrying form.  Normally there is nothing to fix, so the launch must cost next to nothing: a
// workgroup looks at FIX_TILES consecutive row tiles at once - one load per thread and tile, all in flight together, the
// per-thread NaN bits OR-ed into one LDS word - and runs the robust body only for a tile that holds a NaN (1/32 of the
// main kernel's workgroups instead of a full-size grid whose 39 200 workgroups read 1 KB each and leave: ~60 us).
// Tiles are numbered ((ks * Hq + h) * row_tiles + bx); no XCD-aware decode (nothing streams in the common case).
constexpr int FIX_TILES = 32;   // tiles per workgroup = bits of its NaN mask; 28 units x 700 tiles -> 616 workgroups: one resident round
// NaN scan of FIX_TILES consecutive row tiles (RT rows each) of the row statistics, by the whole workgroup: bit u of the
// result (valid after the caller's barriers, OR-ed into an LDS word) says tile t0 + u holds a NaN.  Tile t =
// kh * row_tiles + bx covers lse_part[kh * L + bx * RT + (0 .. RT)).  16-byte loads, every thread busy, 4 loads per
// thread for 32 tiles of 128 rows (the first form - one scalar load per thread and tile from half the threads - cost
// 12-15 us per launch: tools/debug/fixup_probe.sh).
template <int RT>
__device__ __forceinline__ unsigned scan_nan_tiles(const float* __restrict__ lse_part, int t0, int n_tiles, int row_tiles, int L) {
    constexpr int V4 = RT / 4;                       // 16-byte groups per tile
    constexpr int TPP = SC_BLOCK / V4;               // tiles the workgroup covers per load
    static_assert(SC_BLOCK % V4 == 0 && FIX_TILES % TPP == 0, "scan shape");
    const int tid = (int)threadIdx.x;
    const int ul = tid / V4, r0 = (tid - ul * V4) * 4;
    unsigned mine = 0;
    if ((L & 3) == 0) {
        float4 v[FIX_TILES / TPP];
#pragma unroll
        for (int j = 0; j < FIX_TILES / TPP; ++j) {
            const int t = t0 + ul + j * TPP;
            const int bx = t % row_tiles, kh = t / row_tiles;
            const int i = bx * RT + r0;
            v[j] = (t < n_tiles && i < L) ? *(const float4*)(lse_part + (size_t)kh * L + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < FIX_TILES / TPP; ++j)
            mine |= (v[j].x != v[j].x || v[j].y != v[j].y || v[j].z != v[j].z || v[j].w != v[j].w) ? (1u << (ul + j * TPP)) : 0u;
    } else {
        for (int j = 0; j < FIX_TILES / TPP; ++j) {
            const int t = t0 + ul + j * TPP;
            const int bx = t % row_tiles, kh = t / row_tiles;
            bool nan = false;
            for (int e = 0; e < 4; ++e) {
                const int i = bx * RT + r0 + e;
                const float x = (t < n_tiles && i < L) ? lse_part[(size_t)kh * L + i] : 0.f;
                nan = nan || x != x;
            }
            mine |= nan ? (1u << (ul + j * TPP)) : 0u;
        }
    }
    return mine;
}

template <int NB, int MODE>   // MODE: the robust flags (no P1_RAW) of the launch being repaired
__global__ __launch_bounds__(SC_BLOCK, 2) void score_pass1_fixup_kernel(   // (2: registers, not occupancy - no spills)
    const char* __restrict__ q, const char* __restrict__ k, int Hq, int Hkv, int L, int keys_per_split, int row_tiles,
    int n_tiles, float* __restrict__ lse_part, size_t q_unit_bytes, size_t k_unit_bytes, size_t lse_unit_floats,
    int neg_out, QView qv) {
    const int q_hs = qv.row_pitch ? qv.head_stride : L * HD * 2, q_pitch = qv.row_pitch ? qv.row_pitch : HD * 2;
    q = qv.row_pitch ? qv.unit[blockIdx.y] : q + blockIdx.y * q_unit_bytes;
    k += blockIdx.y * k_unit_bytes;
    lse_part += blockIdx.y * lse_unit_floats;
    const int t0 = blockIdx.x * FIX_TILES;
    __shared__ unsigned nan_tiles;       // bit u: tile t0 + u holds a NaN
    if (threadIdx.x == 0) nan_tiles = 0;
    const unsigned mine = scan_nan_tiles<REG_ROWS * NB>(lse_part, t0, n_tiles, row_tiles, L);
    __syncthreads();
    if (mine) atomicOr(&nan_tiles, mine);
    __syncthreads();
    unsigned todo = nan_tiles;   // uniform: the whole workgroup takes the same path
    while (todo) {
        const int u = __builtin_ctz(todo);
        todo &= todo - 1;
        const int t = t0 + u;
        const int bx = t % row_tiles, kh = t / row_tiles;
        const int h = kh % Hq, ks = kh / Hq;
        const int i_base = bx * (REG_ROWS * NB);
        if (NB == 2 && L - i_base <= REG_ROWS)
            score_pass1_dma_body<1, MODE>(q, k, Hq, Hkv, L, keys_per_split, lse_part, i_base, h, ks, neg_out, q_hs, q_pitch);
        else
            score_pass1_dma_body<NB, MODE>(q, k, Hq, Hkv, L, keys_per_split, lse_part, i_base, h, ks, neg_out, q_hs, q_pitch);
        __syncthreads();   // the next tile's prologue writes the LDS buffers this one was still reading
    }
}

}  // namespace rtk

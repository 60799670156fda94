// score_f32.cuh — the fp32 score kernels: the parity path (v_mfma_f32_32x32x2_f32, an exact fp32 fma chain, the
// reference's operation order: dot / sqrt(D), natural exp) and the generic any-head_dim fallback (plain VALU).
//   score_pass1_kernel / score_pass2_kernel  head_dim 128.  The operand whose statistics are kept (query rows in pass 1,
//       keys in pass 2) sits in registers as the MFMA B operand - one 32-row block per wave (NB = 1), so every lane owns
//       one row / column and the reduction over the streamed operand is lane-local over the 16 accumulator registers plus
//       one cross-half shuffle.  The streamed operand goes HBM/L2 -> registers -> XOR-swizzled LDS tile (conflict-free
//       ds_read_b128), the next tile's global loads in flight during the MFMAs.  (Two register blocks need ~250 VGPRs
//       and a second staging set bought nothing: the kernels are bound by instruction issue.)  2 x 32 KiB of dynamic
//       LDS (+ 512 B in pass 2): the launcher opts in above 64 KiB.
//   score_pass1_generic / score_pass2_generic  any head_dim, any dtype: same two passes, one thread per key.
// The register-block loops run once (F32_NB = 1).  They stay loops on purpose: with plain scalars in their place the
// compiler emits a different schedule for both kernels (tools/kernel_diff.py against the looped form), as it does when
// the tails lose their third, never-taken copy of the step or the loop bounds are written jt + 2.
// score_pass1_kernel and score_pass2_kernel are plain (non-template) kernels: one translation unit includes this file.
#pragma once
#include "score_thin.cuh"

namespace rtk {

constexpr int F32_NB = 1;   // 32-row register blocks per wave of the fp32 kernels

// ------------------------------------------------------------------------------------------------
// pass 1: partial row log-sum-exp over one key split
//   lse_part[ks,h,i] = log sum_{j in split ks} exp(q_hi . k_gj / sqrt(D))
// 1-D grid of Hkv * KS * ceil(L/128) * G workgroups (XCD-aware decode below), 256 threads; wave w keeps query rows
// i0 + 32w + (lane&31) in registers.
// ------------------------------------------------------------------------------------------------
struct RowStat {  // online max / sum of one query row, over the keys this lane sees: m = max logit, sum of exp(x - m)
    float m, sum;
    __device__ __forceinline__ void init() { m = -INFINITY; sum = 0.f; }
    template <bool RAGGED>
    __device__ __forceinline__ void update(f32x16& a0, f32x16& a1, int j0, int j_end, int hf, float sqrt_d) {
        // the reference's operation order: logits = dot / sqrt(D), natural exp
#pragma unroll
        for (int r = 0; r < 16; ++r) { a0[r] = __fdiv_rn(a0[r], sqrt_d); a1[r] = __fdiv_rn(a1[r], sqrt_d); }
        if (RAGGED) {  // keys >= j_end do not exist
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (j0 + acc_row(r, hf) >= j_end) a0[r] = -INFINITY;
                if (j0 + 32 + acc_row(r, hf) >= j_end) a1[r] = -INFINITY;
            }
        }
        const float mn = fmaxf(m, fmaxf(max16(a0), max16(a1)));
        if (RAGGED && mn == -INFINITY) return;
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) add += expf(a0[r] - mn);
#pragma unroll
        for (int r = 0; r < 16; ++r) add += expf(a1[r] - mn);
        sum = sum * expf(m - mn) + add;
        m = mn;
    }
    // merge with the other half-wave (disjoint key subsets of the same row) and take the log
    __device__ __forceinline__ float finish() const {
        const float m2 = __shfl_xor(m, 32, WAVE), s2 = __shfl_xor(sum, 32, WAVE);
        const float mm = fmaxf(m, m2);
        if (mm == -INFINITY) return -INFINITY;  // no key seen (cannot happen for a non-empty split)
        const float tot = sum * expf(m - mm) + s2 * expf(m2 - mm);
        return mm + logf(tot);
    }
};


__global__ __launch_bounds__(SC_BLOCK) void score_pass1_kernel(const char* __restrict__ q, const char* __restrict__ k,
                                                               int Hq, int Hkv, int L, int keys_per_split,
                                                               int row_tiles, int xcd_remap,
                                                               float* __restrict__ lse_part) {
    constexpr int DT = RTK_F32, NB = F32_NB;
    using M = MM<DT>;
    using T = Tile<DT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, hf = lane >> 5;
    // XCD-aware decode of a 1-D grid (block b runs on XCD b % 8): all workgroups that stream the same
    // key split of the same KV group share an XCD, so the split stays resident in that XCD's L2.
    const int G = Hq / Hkv;
    int bx, h, ks;
    {
        const int per_group = row_tiles * G;                 // workgroups sharing one (g, ks) key stream
        int grp, w;
        if (xcd_remap) {  // only when the group count is a multiple of 8 (balanced XCDs)
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
    const int g = h / G;
    const int i0 = bx * (REG_ROWS * NB) + wid * (32 * NB);   // this wave's NB*32 query rows
    const int jb = ks * keys_per_split, je = min(L, jb + keys_per_split);
    const char* qh = q + (size_t)h * L * HD * M::ESIZE;
    Pipe<DT> pp;
    pp.init(tid, lane);
    u32x4 qf[NB][M::NREG];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) load_reg_frag<DT>(qh, i0 + 32 * nb, L, lane, qf[nb]);

    const int nkeys = je - jb;
    const int nfull = nkeys / TILE_ROWS;              // full tiles
    const int ntiles = (nkeys + TILE_ROWS - 1) / TILE_ROWS;
    const float sqrt_d = sqrtf((float)HD);
    RowStat rs[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) rs[nb].init();

    constexpr int AHEAD = 1;   // tiles between the one being computed and the one whose loads are in flight
    u32x4 st[T::STAGE];        // staging registers of the tile in flight
    // descriptor over this KV group's [L, 128] key matrix (wave-uniform: kernel arguments and blockIdx only)
    const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(k + (size_t)g * L * HD * M::ESIZE), 0, L * HD * M::ESIZE, 0x00020000);
#define RTK_LOAD_TILE(t) pp.load(krsrc, jb + (t) * TILE_ROWS, st)
    RTK_LOAD_TILE(0);
    pp.store(smem, st);
    __syncthreads();

    // Every A fragment read from LDS feeds NB MFMAs (one per register block).  The MFMA -> softmax
    // dependency is hidden by the other waves on the SIMD (an explicit in-wave pipeline as in pass 2
    // measured equal here).  Tile jt is computed from LDS buffer jt & 1 while the loads of tile jt + AHEAD are
    // in flight; they are written to the other buffer at the end of the step.
    // ISSUE / STORE are compile-time in the steady-state loop: no load sits inside a conditional there.
#define RTK_STEP1(JT, PAR, ISSUE, STORE, MAYRAG) \
    { \
        constexpr int par = PAR; \
        const char* cur = smem + par * T::BYTES; \
        char* nxt = smem + (par ^ 1) * T::BYTES; \
        if constexpr (ISSUE) RTK_LOAD_TILE((JT) + AHEAD); \
        f32x16 acc0[NB], acc1[NB]; \
        { \
            u32x4 a[M::NREG]; \
            pp.read_frags(a, cur, 0); \
_Pragma("unroll") \
            for (int nb = 0; nb < NB; ++nb) { acc0[nb] = f32x16{0}; pp.mma_frags(acc0[nb], a, qf[nb]); } \
            pp.read_frags(a, cur, 1); \
_Pragma("unroll") \
            for (int nb = 0; nb < NB; ++nb) { acc1[nb] = f32x16{0}; pp.mma_frags(acc1[nb], a, qf[nb]); } \
        } \
_Pragma("unroll") \
        for (int nb = 0; nb < NB; ++nb) { \
            /* steady state: tiles are full by construction (a run-time test here gets if-converted into 64 */ \
            /* v_cmp + v_cndmask per tile: 40 % more VALU issue in a kernel that is issue bound)            */ \
            if (!(MAYRAG) || (JT) < nfull) rs[nb].template update<false>(acc0[nb], acc1[nb], 0, 0, hf, sqrt_d); \
            else rs[nb].template update<true>(acc0[nb], acc1[nb], (JT) * TILE_ROWS, nkeys, hf, sqrt_d); \
        } \
        if constexpr (STORE) pp.store(nxt, st); \
        __syncthreads(); \
    }
    int jt = 0;
    for (; jt + AHEAD + 1 < ntiles; jt += 2) {  // steady state, two tiles per trip (parities are constants)
        RTK_STEP1(jt, 0, true, true, false)      // jt + 2 < ntiles here, and only the last tile can be ragged
        RTK_STEP1(jt + 1, 1, true, true, false)
    }
    // tail: at most AHEAD + 1 tiles; jt is even here, so the parities are known statically
#define RTK_TAIL(PAR)                                              \
    if (jt < ntiles) {                                             \
        if (jt + 1 < ntiles) RTK_STEP1(jt, PAR, true, true, true)        \
        else RTK_STEP1(jt, PAR, false, false, true)                      \
        ++jt;                                                      \
    }
    RTK_TAIL(0)
    RTK_TAIL(1)
    RTK_TAIL(0)
#undef RTK_TAIL
#undef RTK_STEP1
#undef RTK_LOAD_TILE
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const float out = rs[nb].finish();
        const int i = i0 + 32 * nb + (lane & 31);
        if (hf == 0 && i < L) lse_part[((size_t)ks * Hq + h) * L + i] = out;
    }
}
// ------------------------------------------------------------------------------------------------
// pass 2: partial[g,split,j] = sum_{h in g} sum_{i in split} exp(s_hij - lse[h,i])
// 1-D grid of Hkv * RS * ceil(L/128) workgroups; wave w keeps keys j0 + 32w + (lane&31) in registers.
// lse[h,i] is the combined normaliser (lse_combine_kernel has folded pass 1's key splits).
// ------------------------------------------------------------------------------------------------
// col += sum_r exp(acc[r] / sqrt(D) - ls[r]) for one 32x32 block (16 values per lane)
__device__ __forceinline__ void colsum_block_f32(float& col, const f32x16& acc, const float* ls, float sqrt_d) {
#pragma unroll
    for (int r = 0; r < 16; ++r) col += expf(__fdiv_rn(acc[r], sqrt_d) - ls[r]);
}

__global__ __launch_bounds__(SC_BLOCK) void score_pass2_kernel(const char* __restrict__ q, const char* __restrict__ k,
                                                               const float* __restrict__ lse, int Hq, int Hkv, int L,
                                                               int rows_per_split, int col_tiles, int RS,
                                                               int xcd_remap, float* __restrict__ partial,
                                                               const int* __restrict__ key_index) {
    constexpr int DT = RTK_F32, NB = F32_NB;
    using M = MM<DT>;
    using T = Tile<DT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lse_s = (float*)(smem + 2 * T::BYTES);  // [2][TILE_ROWS]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, hf = lane >> 5;
    // live keys (key_compact_kernel, see score_pass2_dma_kernel): list positions name the k~ row and the output column
    const int* kidx = nullptr;
    int Lk = L;
    if (key_index && key_index[L] >= 0) {
        kidx = key_index;
        Lk = key_index[L];
    }
    // XCD-aware decode (block b runs on XCD b % 8): the col_tiles workgroups that stream the same query
    // rows (same KV group, same row split) share an XCD and therefore its L2.
    const int G = Hq / Hkv;
    int bx, g, rs;
    {
        int grp;
        if (xcd_remap) {
            const int xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
            grp = xcd + NXCD * (slot / col_tiles);           // (g, rs) pair index
            bx = slot % col_tiles;
        } else {
            grp = blockIdx.x / col_tiles;
            bx = blockIdx.x % col_tiles;
        }
        g = grp % Hkv;
        rs = grp / Hkv;
    }
    const int j0 = bx * (REG_ROWS * NB) + wid * (32 * NB);   // this wave's NB*32 keys (positions in the live list)
    if (bx * (REG_ROWS * NB) >= Lk) return;                   // uniform per workgroup
    const char* kg = k + (size_t)g * L * HD * M::ESIZE;
    const int ib = rs * rows_per_split, ie = min(L, ib + rows_per_split);
    const int nrows = ie - ib;
    const int tiles_per_head = (nrows + TILE_ROWS - 1) / TILE_ROWS;   // >= 1: empty splits are not launched
    const int ntiles = tiles_per_head * G;

    Pipe<DT> pp;
    pp.init(tid, lane);
    u32x4 kf[NB][M::NREG];
    int jcol[NB];   // token index of this lane's key per register block, -1 past the list
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int jp = j0 + 32 * nb + (lane & 31);
        jcol[nb] = jp < Lk ? (kidx ? kidx[jp] : jp) : -1;
        const u32x4* p = (const u32x4*)(kg + (size_t)max(jcol[nb], 0) * HD * M::ESIZE);
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) kf[nb][r] = jcol[nb] >= 0 ? p[M::chunk_of(r, hf)] : u32x4{0, 0, 0, 0};
    }

    const float sqrt_d = sqrtf((float)HD);
    float col[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) col[nb] = 0.f;
    constexpr int AHEAD = 1;   // tiles between the one being computed and the one whose loads are in flight
    u32x4 st[T::STAGE];        // staging registers of the tile in flight
    float lst = 0.f;           // ... and this thread's element of its row normalisers

    // cursor of the tile being prefetched: row tile inside the split, source pointers of the current head
    int nt = 0;
    const int last_row = Hq * L - 1;  // last row of the whole q~ buffer
    const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)q, 0, Hq * L * HD * M::ESIZE, 0x00020000);
    int nrow0 = (g * G) * L + ib;     // first buffer row of the cursor head's split
    // loads the cursor tile (+ this thread's lse element) into the staging registers, then advances the cursor;
    // rows past the split end get lse = +inf: exp(s - inf) = 0 whatever filler the tile holds
#define RTK_ISSUE()                                                                     \
    {                                                                                   \
        pp.load(qrsrc, nrow0 + nt * TILE_ROWS, st);                                     \
        const int r__ = nt * TILE_ROWS + (tid & (TILE_ROWS - 1));                       \
        lst = (r__ < nrows) ? lse[min(nrow0 + r__, last_row)] : INFINITY;               \
        const bool wrap__ = (nt + 1 == tiles_per_head);                                 \
        nt = wrap__ ? 0 : nt + 1;                                                       \
        nrow0 += wrap__ ? L : 0;                                                        \
    }
    // Software pipeline inside the wave: while the matrix pipe runs the 8*NB MFMAs of one 32-row block,
    // the VALU finishes the previous block (fma + exp2 + add per value; the row normalisers are shared by
    // the NB register blocks).  `pend` / `pls` carry a tile's second block across the barrier into the
    // next tile's first MFMA group.
    f32x16 pend[NB];
    float pls[16];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) pend[nb] = f32x16{0};
#pragma unroll
    for (int r = 0; r < 16; ++r) pls[r] = INFINITY;  // exp(-inf) = 0: nothing pending yet
#define RTK_STEP2(BUF, ISSUE, STORE) \
    { \
        constexpr int buf = BUF; \
        const char* cur = smem + buf * T::BYTES; \
        const float* lcur = lse_s + buf * TILE_ROWS; \
        if constexpr (ISSUE) RTK_ISSUE() \
        u32x4 a0[M::NREG], a1[M::NREG]; \
        pp.read_frags(a0, cur, 0); \
        pp.read_frags(a1, cur, 1); \
        float ls0[16], ls1[16]; \
        load_ls(ls0, lcur, 0, hf); \
        load_ls(ls1, lcur, 1, hf); \
        __builtin_amdgcn_sched_barrier(0); \
        f32x16 acc0[NB]; \
_Pragma("unroll") \
        for (int nb = 0; nb < NB; ++nb) { \
            acc0[nb] = f32x16{0}; \
            pp.mma_frags(acc0[nb], a0, kf[nb]); \
            colsum_block_f32(col[nb], pend[nb], pls, sqrt_d); \
            asm volatile("" : "+v"(acc0[nb]), "+v"(col[nb])); \
        } \
        __builtin_amdgcn_sched_barrier(0); \
_Pragma("unroll") \
        for (int nb = 0; nb < NB; ++nb) { \
            pend[nb] = f32x16{0}; \
            pp.mma_frags(pend[nb], a1, kf[nb]); \
            colsum_block_f32(col[nb], acc0[nb], ls0, sqrt_d); \
            asm volatile("" : "+v"(pend[nb]), "+v"(col[nb])); \
        } \
        __builtin_amdgcn_sched_barrier(0); \
_Pragma("unroll") \
        for (int r = 0; r < 16; ++r) pls[r] = ls1[r]; \
        if constexpr (STORE) { \
            pp.store(smem + (buf ^ 1) * T::BYTES, st); \
            if (tid < TILE_ROWS) lse_s[(buf ^ 1) * TILE_ROWS + tid] = lst; \
        } \
        __syncthreads(); \
    }
    RTK_ISSUE()
    pp.store(smem, st);
    if (tid < TILE_ROWS) lse_s[tid] = lst;
    __syncthreads();
    int it = 0;
    for (; it + AHEAD + 1 < ntiles; it += 2) {  // steady state: loads are unconditional => counted vmcnt waits
        RTK_STEP2(0, true, true)
        RTK_STEP2(1, true, true)
    }
    // tail: at most AHEAD + 1 tiles; `it` is even here, so the parities are static
#define RTK_TAIL(PAR)                                        \
    if (it < ntiles) {                                       \
        if (it + 1 < ntiles) RTK_STEP2(PAR, true, true)      \
        else RTK_STEP2(PAR, false, false)                    \
        ++it;                                                \
    }
    RTK_TAIL(0)
    RTK_TAIL(1)
    RTK_TAIL(0)
#undef RTK_TAIL
#undef RTK_STEP2
#undef RTK_ISSUE
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        colsum_block_f32(col[nb], pend[nb], pls, sqrt_d);  // drain the pipeline
        col[nb] += __shfl_xor(col[nb], 32, WAVE);
        if (hf == 0 && jcol[nb] >= 0) partial[((size_t)g * RS + rs) * L + jcol[nb]] = col[nb];
    }
}
// ------------------------------------------------------------------------------------------------
// generic fallback (any head_dim; small problems): plain fp32 VALU, same two passes.
// ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void score_pass1_generic(const void* __restrict__ q, const void* __restrict__ k,
                                                           int Hq, int Hkv, int L, int D, float* __restrict__ lse) {
    extern __shared__ float qs[];  // [D]
    __shared__ float red_m[4], red_s[4];
    const int i = blockIdx.x, h = blockIdx.y, g = h / (Hq / Hkv), tid = threadIdx.x;
    for (int d = tid; d < D; d += blockDim.x) qs[d] = ld_any<DT>(q, ((size_t)h * L + i) * D + d);
    __syncthreads();
    const float sqrt_d = sqrtf((float)D);
    float m = -INFINITY, sum = 0.f;
    for (int j = tid; j < L; j += blockDim.x) {
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(qs[d], ld_any<DT>(k, ((size_t)g * L + j) * D + d), s);
        s = __fdiv_rn(s, sqrt_d);
        const float mn = fmaxf(m, s);
        sum = sum * expf(m - mn) + expf(s - mn);
        m = mn;
    }
    // wave then block combine of (m, sum)
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, WAVE), s2 = __shfl_xor(sum, o, WAVE);
        const float mm = fmaxf(m, m2);
        if (mm > -INFINITY) sum = sum * expf(m - mm) + s2 * expf(m2 - mm);
        m = mm;
    }
    if ((tid & 63) == 0) { red_m[tid / 64] = m; red_s[tid / 64] = sum; }
    __syncthreads();
    if (tid == 0) {
        float mm = red_m[0], ss = red_s[0];
        for (int w = 1; w < 4; ++w) {
            const float m2 = red_m[w], s2 = red_s[w];
            const float mx = fmaxf(mm, m2);
            if (mx > -INFINITY) ss = ss * expf(mm - mx) + s2 * expf(m2 - mx);
            mm = mx;
        }
        lse[(size_t)h * L + i] = mm + logf(ss);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void score_pass2_generic(const void* __restrict__ q, const void* __restrict__ k,
                                                           const float* __restrict__ lse, int Hq, int Hkv, int L, int D,
                                                           float* __restrict__ partial) {
    extern __shared__ float qs[];  // [D]
    const int g = blockIdx.y, G = Hq / Hkv, tid = threadIdx.x;
    const int j = blockIdx.x * blockDim.x + tid;
    const float sqrt_d = sqrtf((float)D);
    float col = 0.f;
    for (int hh = 0; hh < G; ++hh) {
        const int h = g * G + hh;
        float blk = 0.f;   // two-level sum: 64-row blocks, then blocks (a plain running sum over G * L terms drifts by ~1e-5)
        for (int i = 0; i < L; ++i) {
            __syncthreads();
            for (int d = tid; d < D; d += blockDim.x) qs[d] = ld_any<DT>(q, ((size_t)h * L + i) * D + d);
            __syncthreads();
            if (j < L) {
                float s = 0.f;
                for (int d = 0; d < D; ++d) s = fmaf(qs[d], ld_any<DT>(k, ((size_t)g * L + j) * D + d), s);
                blk += expf(__fdiv_rn(s, sqrt_d) - lse[(size_t)h * L + i]);
            }
            if ((i & 63) == 63 || i + 1 == L) {
                col += blk;
                blk = 0.f;
            }
        }
    }
    if (j < L) partial[(size_t)g * L + j] = col;
}

}  // namespace rtk

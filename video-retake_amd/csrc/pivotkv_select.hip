// pivotkv_select.hip — PivotKV selection on gfx950: which rows of a chunk survive.
// Replaces longvideo_cache.py:272-295 (masked_fill_, topk + sort, the gather of the temporal ids and their rescale).
// Exact top-k with ties lowest index first, three forms with the same result bit for bit: one workgroup with the keys
// re-read from memory (any L), one workgroup per unit with the keys in LDS (L <= 16384), and the chip-wide rank / emit
// pair.  The batched entry point first reduces the units' column partials to scores (finalize).
#include <algorithm>
#include <atomic>

#include "common.cuh"
#include "select.cuh"

namespace rtk {


constexpr int PSEL_BLOCK = 1024;

__global__ __launch_bounds__(PSEL_BLOCK) void pivotkv_select_kernel(float* __restrict__ score,
                                                                    const uint8_t* __restrict__ mask, int L, int keep,
                                                                    const int64_t* __restrict__ pos, int P,
                                                                    int reforge, int64_t* __restrict__ keep_idx,
                                                                    int32_t* __restrict__ rank,
                                                                    int64_t* __restrict__ pos_out, int64_t pos_ld) {
    __shared__ SelectSmem sm;
    __shared__ long long red[PSEL_BLOCK / WAVE];
    const int tid = threadIdx.x;
    for (int i = tid; i < L; i += PSEL_BLOCK) {
        if (mask && mask[i]) score[i] = 1.0f;  // attn_weights.masked_fill_(mask, 1.)  (:274)
        rank[i] = -1;
    }
    __syncthreads();
    auto key = [&](int i) -> uint32_t { return f2key(score[i]); };
    uint32_t thr;
    int need_eq;
    block_radix_threshold<PSEL_BLOCK>(key, L, keep, sm, thr, need_eq);
    block_ordered_compact<PSEL_BLOCK>(key, L, thr, need_eq, sm, [&](int r, int i) {
        keep_idx[r] = i;  // topk(keep).sort()  (:276-277)
        rank[i] = r;
        if (pos)
            for (int p = 0; p < P; ++p) pos_out[(size_t)p * pos_ld + r] = pos[(size_t)p * L + i];  // :283-288
    });
    if (!(pos && reforge)) return;
    __syncthreads();
    // min_temp_id = compressed_position_ids[0].min()  (:293)
    long long mn = 0x7fffffffffffffffLL;
    for (int r = tid; r < keep; r += PSEL_BLOCK) mn = min(mn, (long long)pos_out[r]);
    block_min_ll<PSEL_BLOCK / WAVE>(mn, red);
    // comp_ratio = keep_len / k_len (python float) ; int64 * float -> float32 multiply ; .long() truncates (:294-295)
    const float ratio = (float)((double)keep / (double)L);
    for (int r = tid; r < keep; r += PSEL_BLOCK) {
        const float f = (float)((long long)pos_out[r] - mn) * ratio;
        pos_out[r] = mn + (long long)f;
    }
}

constexpr uint32_t KEY_ONE = 0xBF800000u;   // f2key(1.0f)

// ------------------------------------------------------------------------------------------------
// One workgroup per unit, small code: the selection of a batched launch runs on ONE CU per unit, where what counts is
// the number of instructions issued AND fetched - a kernel is entered with a cold instruction cache, and the
// register-resident form of this kernel (keys of 8 consecutive tokens per thread, every loop unrolled: 14 KB of
// straight-line code executed once) took 31 us per 28-unit launch at L = 6272 against 24 us for this one, 4.5 KB
// (same-box A/B, profiles/r13_ab_select.txt).  The keys live in LDS
// (thread t owns tokens [t*per, (t+1)*per), row stride per|1 words: conflict-free), every per-token loop is a real
// loop, and all global traffic is coalesced:
//   0  scores (+ mask override, :272-274) -> keys; the tokens at exactly 1.0 (every key-patch token) are counted once
//   1  4 radix passes of 8 bits over the LDS keys: a wave whose digits all agree issues one atomic
//   2  one packed block scan (greater | equal << 16): output position of every thread's first kept token
//   3  kept indices -> LDS in ascending order
//   4  cooperative over the kept rows: temporal ids gathered, min_temp_id (:293)
//   5  cooperative, coalesced stores: keep_idx, gathered / rescaled ids (:283-295), rank
// Exact radix select, ties lowest index first: the results of the chip-wide rank / emit pair and of the generic kernel above.
// ------------------------------------------------------------------------------------------------
constexpr int SEL_LDS_MAX_PER = 16;   // tokens per thread: L <= 16384
__host__ __device__ inline size_t select_lds_bytes(int L, int keep) {
    const int per = (L + PSEL_BLOCK - 1) / PSEL_BLOCK;
    return ((size_t)(per | 1) * PSEL_BLOCK + (size_t)keep) * sizeof(uint32_t);
}

__device__ __forceinline__ void select_lds_body(float* __restrict__ score, const uint8_t* __restrict__ mask, int L, int keep,
                                                const int64_t* __restrict__ pos, int P, int reforge,
                                                int64_t* __restrict__ keep_idx, int32_t* __restrict__ rank,
                                                int64_t* __restrict__ pos_out, int64_t pos_ld) {
    extern __shared__ uint32_t sel_lds[];
    __shared__ SelectSmem sm;
    __shared__ uint32_t wtot[PSEL_BLOCK / WAVE];
    __shared__ long long red[PSEL_BLOCK / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int per = (L + PSEL_BLOCK - 1) / PSEL_BLOCK, ps = per | 1;
    uint32_t* keyL = sel_lds;                         // token i at (i / per) * ps + i % per
    uint32_t* keepL = sel_lds + (size_t)ps * PSEL_BLOCK;
    const int base = tid * per, kb = tid * ps;
    const int mine = max(0, min(per, L - base));      // tokens this thread owns
    // ---- 0: keys --------------------------------------------------------------------------------------------
    uint32_t ones = 0;
    // i / per as a multiply-high: exact for i < 2^14 and 2 <= per <= 16 (the error term i * (M - 2^20/per) / 2^20 < 1/per)
    const uint32_t magic = (((1u << 20) + (uint32_t)per - 1u) / (uint32_t)per) << 12;
    for (int i = tid; i < L; i += PSEL_BLOCK) {
        float sc = score[i];
        if (mask && mask[i]) {  // attn_weights.masked_fill_(mask, 1.)  (:274)
            sc = 1.0f;
            score[i] = 1.0f;
        }
        const uint32_t k = f2key(sc);
        const int t = per == 1 ? i : (int)__umulhi((uint32_t)i, magic);
        keyL[t * ps + (i - t * per)] = k;
        ones += (uint32_t)__popcll(__ballot(k == KEY_ONE));
        if (rank) rank[i] = -1;
    }
    if (lane == 0) wtot[wid] = ones;
    // ---- 1: exact k-th largest key --------------------------------------------------------------------------
    uint32_t prefix = 0, pmask = 0;
    int kk = keep;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) sm.hist[tid] = 0;
        __syncthreads();
        if (tid == PSEL_BLOCK - 1 && (KEY_ONE & pmask) == prefix) {   // the tokens at 1.0, as one count
            uint32_t n1 = 0;
            for (int w = 0; w < PSEL_BLOCK / WAVE; ++w) n1 += wtot[w];
            if (n1) atomicAdd(&sm.hist[(KEY_ONE >> shift) & 255u], n1);
        }
#pragma unroll 1
        for (int e = 0; e < per; ++e) {
            const uint32_t k = keyL[kb + e];
            const bool m = e < mine && k != KEY_ONE && (k & pmask) == prefix;
            const uint32_t d = (k >> shift) & 255u;
            const unsigned long long bal = __ballot(m);
            if (bal != 0) {                                           // wave-uniform
                const int leader = __ffsll((long long)bal) - 1;
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
                if (__ballot(m && d == d0) == bal) {                  // every digit of the wave alike: one atomic
                    if (lane == leader) atomicAdd(&sm.hist[d0], (uint32_t)__popcll(bal));
                } else if (m) {
                    atomicAdd(&sm.hist[d], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < WAVE) {
            const uint32_t h0 = sm.hist[4 * lane], h1 = sm.hist[4 * lane + 1], h2 = sm.hist[4 * lane + 2],
                           h3 = sm.hist[4 * lane + 3];
            const uint32_t own = h0 + h1 + h2 + h3;
            uint32_t incl = own;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t t = __shfl_down(incl, o, WAVE);
                if (lane + o < WAVE) incl += t;
            }
            const uint32_t above = incl - own;
            if (above < (uint32_t)kk && (uint32_t)kk <= incl) {
                uint32_t c = above;
                int b;
                if ((uint32_t)kk <= c + h3) { b = 3; }
                else { c += h3; if ((uint32_t)kk <= c + h2) { b = 2; }
                else { c += h2; if ((uint32_t)kk <= c + h1) { b = 1; }
                else { c += h1; b = 0; } } }
                sm.bcast[0] = prefix | ((uint32_t)(4 * lane + b) << shift);
                sm.bcast[1] = (uint32_t)kk - c;
            }
        }
        __syncthreads();
        prefix = sm.bcast[0];
        kk = (int)sm.bcast[1];
        pmask |= 255u << shift;
    }
    const uint32_t thr = prefix;
    const int need_eq = kk;
    // ---- 2: where this thread's kept tokens go ----------------------------------------------------------------
    uint32_t own = 0;
#pragma unroll 1
    for (int e = 0; e < mine; ++e) {
        const uint32_t k = keyL[kb + e];
        own += (k > thr ? 1u : 0u) + (k == thr ? 0x10000u : 0u);
    }
    uint32_t inc = own;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += t;
    }
    if (lane == WAVE - 1) wtot[wid] = inc;
    __syncthreads();
    uint32_t before = inc - own;
    for (int w = 0; w < wid; ++w) before += wtot[w];
    const int eq_before = (int)(before >> 16);
    int eq_left = max(0, need_eq - eq_before);                   // ties: lowest index first
    int r = (int)(before & 0xffffu) + min(eq_before, need_eq);
    // ---- 3: kept indices, ascending ----------------------------------------------------------------------------
#pragma unroll 1
    for (int e = 0; e < mine; ++e) {
        const uint32_t k = keyL[kb + e];
        bool sel = k > thr;
        if (k == thr && eq_left > 0) {
            sel = true;
            --eq_left;
        }
        if (sel) keepL[r++] = (uint32_t)(base + e);
    }
    __syncthreads();
    // ---- 4: min_temp_id = compressed_position_ids[0].min()  (:293) ---------------------------------------------
    const bool rf = pos && reforge;
    long long mn = 0x7fffffffffffffffLL;
    if (rf) {
        for (int q = tid; q < keep; q += PSEL_BLOCK) mn = min(mn, (long long)pos[keepL[q]]);
        block_min_ll<PSEL_BLOCK / WAVE>(mn, red);
    }
    // ---- 5: outputs ----------------------------------------------------------------------------------------------
    const float ratio = (float)((double)keep / (double)L);  // comp_ratio = keep_len / k_len (:294)
    for (int q = tid; q < keep; q += PSEL_BLOCK) {
        const int i = (int)keepL[q];
        keep_idx[q] = i;  // topk(keep).sort()  (:276-277)
        if (pos) {
            const long long t0 = pos[i];
            // row 0: gathered id, rescaled when reforging: int64 -> float32 multiply -> truncation (:293-295)
            pos_out[q] = rf ? mn + (long long)((float)(t0 - mn) * ratio) : t0;
            for (int p = 1; p < P; ++p) pos_out[(size_t)p * pos_ld + q] = pos[(size_t)p * L + i];   // :283-288
        }
        if (rank) rank[i] = q;
    }
}

// ------------------------------------------------------------------------------------------------
// Chip-wide selection (the default path): the same exact result as the one-workgroup kernels above, in two
// launches that use every CU instead of one.
//   rank kernel  every workgroup loads ALL L keys into LDS and ranks RANK_TOK tokens by counting:
//                rank_i = #{j : key_j > key_i  or  (key_j == key_i and j < i)}   (ties: lowest index first)
//                token i is kept  <=>  rank_i < keep.                 O(L^2) compares over ~L/32 workgroups
//   emit kernel  ascending compaction: position of a kept token = number of kept tokens before it
//                (= topk(keep).sort()), id gather and temporal rescale
// Integer compares only: bit-reproducible and independent of the launch geometry.
// ------------------------------------------------------------------------------------------------
constexpr int RANK_TOK = 64;           // tokens ranked per workgroup (one per lane of a wave)
constexpr int RANK_SEG = 16;           // waves per workgroup, each scanning one segment of the keys
constexpr int RANK_BLOCK = RANK_TOK * RANK_SEG;

struct SelUnits {
    rtk_select_unit u[RTK_SELECT_MAX_UNITS];
};
// Batched launches (one unit per layer of a chunk): one workgroup per unit, all units side by side.  With >= 8 units in
// flight that beats spreading every unit over the chip: the 28 selections of a chunk take one workgroup's latency
// instead of 28 x 98 ranking workgroups.
__global__ __launch_bounds__(PSEL_BLOCK) void pivotkv_select_lds_units_kernel(SelUnits units, int L, int keep, int P,
                                                                              int reforge, int64_t pos_ld) {
    const rtk_select_unit& u = units.u[blockIdx.x];
    select_lds_body(u.score, u.mask, L, keep, u.pos, P, reforge, u.keep_idx, u.rank, u.pos_out, pos_ld);
}

// scratch layout inside a unit's workspace: sel [L] bytes | per-rank-workgroup counts | per-rank-workgroup minima
__host__ __device__ inline size_t sel_ws_cnt_off(int L) { return ((size_t)L + 255) & ~(size_t)255; }
__host__ __device__ inline size_t sel_ws_tmin_off(int L) {
    const size_t nb = ((size_t)L + 63) / 64;
    return sel_ws_cnt_off(L) + ((nb * 4 + 255) & ~(size_t)255);
}

// score[j] = mean_g( (sum_split partial[g,split,j]) / G ) for every unit that still carries partials
// (longvideo_cache.py:269-270): the deferred form of score_finalize_kernel, same fixed summation order.
__global__ __launch_bounds__(256) void finalize_units_kernel(SelUnits units, int Hkv, int RS, int G, int L) {
    extern __shared__ float fin_gs[];  // [Hkv][64]
    const rtk_select_unit& un = units.u[blockIdx.y];
    if (!un.partial) return;
    const int jl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + jl;
    const int jc = min(j, L - 1);
    for (int g = part; g < Hkv; g += 4) {
        const float* p = un.partial + (size_t)g * RS * L + jc;
        float gs = 0.f;
        int r = 0;
        for (; r + 8 <= RS; r += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u) * L];
#pragma unroll
            for (int u = 0; u < 8; ++u) gs += v[u];
        }
        for (; r < RS; ++r) gs += p[(size_t)r * L];
        fin_gs[g * 64 + jl] = gs / (float)G;
    }
    __syncthreads();
    if (part == 0 && j < L) {
        float tot = 0.f;
        for (int g = 0; g < Hkv; ++g) tot += fin_gs[g * 64 + jl];
        un.score[j] = tot / (float)Hkv;
    }
}

// the same for RTK_BF16_REFROUND / RTK_F16_REFROUND partials ([Hkv*G][RS][L], per head): the reference's 16-bit roundings of the per-head
// sums and the two means (longvideo_cache.py:268-270), finalize_ref_column() in common.cuh
template <bool F16>
__global__ __launch_bounds__(256) void finalize_units_ref_kernel(SelUnits units, int Hkv, int RS, int G, int L) {
    const rtk_select_unit& un = units.u[blockIdx.y];
    if (!un.partial) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < L) un.score[j] = finalize_ref_column<F16>(un.partial, Hkv, RS, G, L, j);
}

__global__ __launch_bounds__(RANK_BLOCK) void pivotkv_rank_kernel(SelUnits units, int L, int keep, int reforge) {
    const rtk_select_unit& un = units.u[blockIdx.y];
    float* __restrict__ score = un.score;
    const uint8_t* __restrict__ mask = un.mask;
    const int64_t* __restrict__ pos = un.pos;
    uint8_t* __restrict__ sel = (uint8_t*)un.workspace;
    int32_t* __restrict__ blk_cnt = (int32_t*)((char*)un.workspace + sel_ws_cnt_off(L));
    int64_t* __restrict__ blk_tmin = (int64_t*)((char*)un.workspace + sel_ws_tmin_off(L));
    const int vec_ok = (((uintptr_t)score & 15) == 0 && ((uintptr_t)mask & 3) == 0) ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t rk_keys[];  // [n4 * 4] keys (zero padded) + [RANK_SEG][RANK_TOK] counts
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * RANK_TOK;
    const int n4 = ((L + RANK_TOK - 1) / RANK_TOK) * (RANK_TOK / 4);   // keys padded to whole workgroup ranges
    int* part = (int*)(rk_keys + (size_t)n4 * 4);
    // every key of the chunk -> LDS (no global store in this loop: the loads pipeline freely).  Masked
    // tokens take the key of 1.0 (attn_weights.masked_fill_(mask, 1.), :274); padding keys are 0, smaller
    // than every real key, and only ever compared with '>'.
    const uint32_t one_key = f2key(1.0f);
    for (int j4 = tid; j4 < n4; j4 += RANK_BLOCK) {
        const int j = 4 * j4;
        uint4 kk = {0u, 0u, 0u, 0u};
        if (vec_ok && j + 3 < L) {
            const float4 sc = *(const float4*)(score + j);
            const uint32_t m = mask ? *(const uint32_t*)(mask + j) : 0u;
            kk.x = (m & 0x000000ffu) ? one_key : f2key(sc.x);
            kk.y = (m & 0x0000ff00u) ? one_key : f2key(sc.y);
            kk.z = (m & 0x00ff0000u) ? one_key : f2key(sc.z);
            kk.w = (m & 0xff000000u) ? one_key : f2key(sc.w);
        } else {
            uint32_t e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j + u < L) e[u] = (mask && mask[j + u]) ? one_key : f2key(score[j + u]);
            kk = uint4{e[0], e[1], e[2], e[3]};
        }
        ((uint4*)rk_keys)[j4] = kk;
    }
    __syncthreads();
    const int t = tid % RANK_TOK;
    const int q = __builtin_amdgcn_readfirstlane(tid / RANK_TOK);   // wave index: uniform, loop bounds are scalar
    const int i = i0 + t;
    const uint32_t ki = (i < L) ? rk_keys[i] : 0xffffffffu;
    const int per = (n4 + RANK_SEG - 1) / RANK_SEG;
    const int j4b = q * per, j4e = min(n4, j4b + per);
    const int own4b = i0 / 4, own4e = own4b + RANK_TOK / 4;
    int cnt = 0;
    const uint4* k4 = (const uint4*)rk_keys;
    // Keys before the workgroup's own token range count on '>=' (ties: lower index first) = '> ki - 1', keys
    // after it on '>'; the own range is handled exactly below.  No real key is 0, so ki - 1 cannot wrap.
    auto count_range = [&](int b, int e, uint32_t thr) {
#pragma unroll 4
        for (int j4 = b; j4 < e; ++j4) {
            const uint4 kk = k4[j4];        // same address in every lane: LDS broadcast
            cnt += (kk.x > thr) + (kk.y > thr) + (kk.z > thr) + (kk.w > thr);
        }
    };
    count_range(j4b, min(j4e, own4b), ki - 1u);
    count_range(max(j4b, own4e), j4e, ki);
    {   // own range [i0, i0 + RANK_TOK): wave q takes keys i0 + 4q .. i0 + 4q + 3 (RANK_SEG * 4 == RANK_TOK)
        static_assert(RANK_SEG * 4 == RANK_TOK, "own-range split");
        const int j = i0 + 4 * q;
        const uint4 kk = k4[j >> 2];        // padding keys (j >= L) are 0: never counted
        cnt += (kk.x > ki || (kk.x == ki && j < i)) + (kk.y > ki || (kk.y == ki && j + 1 < i)) +
               (kk.z > ki || (kk.z == ki && j + 2 < i)) + (kk.w > ki || (kk.w == ki && j + 3 < i));
    }
    part[q * RANK_TOK + t] = cnt;
    __syncthreads();
    if (tid < WAVE) {  // first wave: lane t owns token i0 + t
        bool kept = false;
        long long tm = 0x7fffffffffffffffLL;
        if (i < L) {
            int rank = 0;
#pragma unroll
            for (int sg = 0; sg < RANK_SEG; ++sg) rank += part[sg * RANK_TOK + tid];
            kept = rank < keep;
            sel[i] = kept;
            if (ki == one_key && mask && mask[i]) score[i] = 1.0f;  // masked_fill_ is in place (:274)
            if (kept && pos && reforge) tm = pos[i];
        }
        const unsigned long long b = __ballot(kept);
        for (int o = 32; o > 0; o >>= 1) {
            const long long t2 = __shfl_xor(tm, o, WAVE);
            tm = min(tm, t2);
        }
        if (tid == 0) {
            blk_cnt[blockIdx.x] = (int32_t)__popcll(b);
            blk_tmin[blockIdx.x] = tm;  // min_temp_id partial (:293)
        }
    }
}

// ordered emit: one workgroup per 256 tokens.  The number of kept tokens before its range and min_temp_id
// come from the rank kernel's per-workgroup records (RANK_TOK tokens each).
__global__ __launch_bounds__(256) void pivotkv_emit_kernel(SelUnits units, int L, int keep, int P, int reforge,
                                                           int64_t pos_ld) {
    const rtk_select_unit& un = units.u[blockIdx.y];
    const uint8_t* __restrict__ sel = (const uint8_t*)un.workspace;
    const int32_t* __restrict__ blk_cnt = (const int32_t*)((const char*)un.workspace + sel_ws_cnt_off(L));
    const int64_t* __restrict__ blk_tmin = (const int64_t*)((const char*)un.workspace + sel_ws_tmin_off(L));
    const int64_t* __restrict__ pos = un.pos;
    int64_t* __restrict__ keep_idx = un.keep_idx;
    int32_t* __restrict__ rank = un.rank;
    int64_t* __restrict__ pos_out = un.pos_out;
    __shared__ int wtot[4];
    __shared__ int wsum[4];
    __shared__ long long wmin[4];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int b0 = blockIdx.x * 256;
    const bool rf = pos && reforge;
    const int nb = (L + RANK_TOK - 1) / RANK_TOK, nb_before = b0 / RANK_TOK;
    const int i = b0 + tid;
    const int mine = (i < L) ? (int)sel[i] : 0;
    const long long t0 = (mine && pos) ? (long long)pos[i] : 0;
    int before = 0;
    long long mn = 0x7fffffffffffffffLL;
    for (int b = tid; b < nb; b += 256) {
        before += (b < nb_before) ? blk_cnt[b] : 0;
        if (rf) mn = min(mn, (long long)blk_tmin[b]);
    }
    // wave scan of the own flags + wave sums of `before` / min of mn, then combine across the 4 waves
    int inc = mine;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += t;
    }
    before = wave_sum_i(before);
    for (int o = 32; o > 0; o >>= 1) {
        const long long t = __shfl_xor(mn, o, WAVE);
        mn = min(mn, t);
    }
    if (lane == WAVE - 1) wtot[wid] = inc;
    if (lane == 0) { wsum[wid] = before; wmin[wid] = mn; }
    __syncthreads();
    int r = wsum[0] + wsum[1] + wsum[2] + wsum[3] + inc - mine;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wid) r += wtot[w];
    mn = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
    if (i >= L) return;
    if (!mine) {
        if (rank) rank[i] = -1;
        return;
    }
    keep_idx[r] = i;  // topk(keep).sort()  (:276-277)
    if (rank) rank[i] = r;
    if (pos) {
        // row 0: gathered id, rescaled when reforging: int64 -> float32 multiply -> truncation (:293-295)
        const float ratio = (float)((double)keep / (double)L);  // comp_ratio = keep_len / k_len (:294)
        pos_out[r] = rf ? mn + (long long)((float)(t0 - mn) * ratio) : t0;
        for (int p = 1; p < P; ++p) pos_out[(size_t)p * pos_ld + r] = pos[(size_t)p * L + i];  // :283-288
    }
}
}  // namespace rtk

using namespace rtk;

extern "C" size_t rtk_pivotkv_select_workspace_bytes(int L) {
    if (L <= 0) return 0;
    const size_t nb = ((size_t)L + RANK_TOK - 1) / RANK_TOK;
    return sel_ws_tmin_off(L) + ((nb * 8 + 255) & ~(size_t)255);
}

static bool chipwide_ok(int L) {
    const size_t lds = ((size_t)((L + RANK_TOK - 1) / RANK_TOK) * RANK_TOK + RANK_BLOCK) * sizeof(uint32_t);
    return L >= 512 && lds <= 160 * 1024;
}

constexpr int UNITS_ONE_WG = 8;   // batched launches with at least this many units select one workgroup per unit
// > 64 KiB of dynamic LDS: opt-in per device, remembered in one atomic bit per device
static void select_lds_opt_in() {
    static std::atomic<uint64_t> opted{0};
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    const uint64_t bit = 1ull << (dev_id & 63);
    if (!(opted.load(std::memory_order_relaxed) & bit)) {
        (void)hipFuncSetAttribute((const void*)pivotkv_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)pivotkv_select_lds_units_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
        opted.fetch_or(bit, std::memory_order_relaxed);
    }
}

// finalize (units that carry partials) -> rank -> emit, every unit in the same three launches
static int select_units(const rtk_select_unit* units, int n, int Hkv, int RS, int G, int L, int keep, int P, int reforge,
                        int64_t pos_out_stride, hipStream_t st, int refround = 0 /* 1: bf16 chain, 2: fp16 chain */) {
    select_lds_opt_in();
    const size_t lds = ((size_t)((L + RANK_TOK - 1) / RANK_TOK) * RANK_TOK + RANK_BLOCK) * sizeof(uint32_t);
    for (int b = 0; b < n; b += RTK_SELECT_MAX_UNITS) {
        const int m = std::min(RTK_SELECT_MAX_UNITS, n - b);
        const SelUnits su = pad_units<SelUnits>(units + b, m);
        bool any_partial = false;
        for (int i = 0; i < m; ++i) any_partial = any_partial || su.u[i].partial != nullptr;
        if (any_partial) {
            if (refround)
                RTK_LAUNCH(KID_FINALIZE, refround == 2 ? finalize_units_ref_kernel<true> : finalize_units_ref_kernel<false>,
                           dim3((L + 255) / 256, m), dim3(256), 0, st, su, Hkv, RS, G, L);
            else
                RTK_LAUNCH(KID_FINALIZE, finalize_units_kernel, dim3((L + 63) / 64, m), dim3(256),
                           (size_t)Hkv * 64 * sizeof(float), st, su, Hkv, RS, G, L);
            RTK_LAUNCH_CHECK("finalize_units_kernel");
        }
        const int per = (L + PSEL_BLOCK - 1) / PSEL_BLOCK;
        if (m >= UNITS_ONE_WG && per <= SEL_LDS_MAX_PER) {
            RTK_LAUNCH(KID_PSEL, pivotkv_select_lds_units_kernel, dim3(m), dim3(PSEL_BLOCK), select_lds_bytes(L, keep), st, su, L,
                       keep, P, reforge, pos_out_stride);
            RTK_LAUNCH_CHECK("pivotkv_select_lds_units_kernel");
            continue;
        }
        RTK_LAUNCH(KID_PSEL, pivotkv_rank_kernel, dim3((L + RANK_TOK - 1) / RANK_TOK, m), dim3(RANK_BLOCK), lds, st, su, L, keep,
                   reforge);
        RTK_LAUNCH_CHECK("pivotkv_rank_kernel");
        RTK_LAUNCH(KID_PEMIT, pivotkv_emit_kernel, dim3((L + 255) / 256, m), dim3(256), 0, st, su, L, keep, P, reforge,
                   pos_out_stride);
        RTK_LAUNCH_CHECK("pivotkv_emit_kernel");
    }
    return RTK_OK;
}

extern "C" int rtk_pivotkv_select_batched(const rtk_select_unit* units, int n_units, int Hkv, int RS, int G, int L,
                                          int keep, int P, int reforge, int64_t pos_out_stride, int score_dtype,
                                          rtk_stream_t stream) {
    RTK_CHECK_ARG(units && n_units >= 1, "rtk_pivotkv_select_batched: no units");
    RTK_CHECK_ARG(L >= 1 && keep >= 1 && keep <= L, "rtk_pivotkv_select_batched: keep=%d out of range for L=%d", keep, L);
    RTK_CHECK_ARG(P == 0 || P == 1 || P == 3, "rtk_pivotkv_select_batched: P must be 0, 1 or 3, got %d", P);
    RTK_CHECK_ARG(P == 0 || pos_out_stride >= keep, "rtk_pivotkv_select_batched: pos_out_stride < keep");
    bool partials = false;
    for (int i = 0; i < n_units; ++i) {
        const rtk_select_unit& u = units[i];
        RTK_CHECK_ARG(u.score && u.keep_idx && u.workspace, "rtk_pivotkv_select_batched: unit %d: NULL pointer", i);
        RTK_CHECK_ARG(((uintptr_t)u.workspace & 255) == 0, "rtk_pivotkv_select_batched: unit %d: workspace must be 256-byte aligned", i);
        RTK_CHECK_ARG((u.pos == nullptr) == (u.pos_out == nullptr), "rtk_pivotkv_select_batched: unit %d: pos and pos_out go together", i);
        RTK_CHECK_ARG((u.pos != nullptr) == (P > 0), "rtk_pivotkv_select_batched: unit %d: pos must be given iff P > 0", i);
        partials = partials || u.partial;
    }
    RTK_CHECK_ARG(!partials || (Hkv >= 1 && RS >= 1 && G >= 1), "rtk_pivotkv_select_batched: partials need Hkv, RS, G");
    if (!chipwide_ok(L)) {
        set_error("rtk_pivotkv_select_batched: L=%d is outside the chip-wide selection path (use rtk_pivotkv_select)", L);
        return RTK_EUNSUPPORTED;
    }
    return select_units(units, n_units, Hkv, RS, G, L, keep, P, reforge, pos_out_stride, (hipStream_t)stream,
                        (score_dtype & ~RTK_SCORE_MANY_UNITS) == RTK_BF16_REFROUND ? 1
                        : ((score_dtype & ~RTK_SCORE_MANY_UNITS) == RTK_F16_REFROUND ? 2 : 0));
}

extern "C" int rtk_pivotkv_select(float* score, const uint8_t* mask, int L, int keep, const int64_t* pos, int P,
                                  int reforge, int64_t* keep_idx, int32_t* rank, int64_t* pos_out,
                                  int64_t pos_out_stride, void* workspace, size_t workspace_bytes,
                                  rtk_stream_t stream) {
    RTK_CHECK_ARG(score && keep_idx, "rtk_pivotkv_select: NULL pointer");
    RTK_CHECK_ARG(L >= 1 && keep >= 1 && keep <= L, "rtk_pivotkv_select: keep=%d out of range for L=%d", keep, L);
    RTK_CHECK_ARG((pos == nullptr) == (pos_out == nullptr), "rtk_pivotkv_select: pos and pos_out go together");
    RTK_CHECK_ARG(!pos || P == 1 || P == 3, "rtk_pivotkv_select: P must be 1 or 3, got %d", P);
    RTK_CHECK_ARG(!pos || pos_out_stride >= keep, "rtk_pivotkv_select: pos_out_stride %lld < keep %d",
                  (long long)pos_out_stride, keep);
    hipStream_t st = (hipStream_t)stream;
    const bool chipwide = workspace && workspace_bytes >= rtk_pivotkv_select_workspace_bytes(L) &&
                          ((uintptr_t)workspace & 255) == 0 && chipwide_ok(L);
    rtk_select_unit u;
    u.partial = nullptr;
    u.score = score;
    u.mask = mask;
    u.pos = pos;
    u.keep_idx = keep_idx;
    u.rank = rank;
    u.pos_out = pos_out;
    u.workspace = chipwide ? workspace : nullptr;
    // chip-wide path: rank by counting (every CU), then ordered emit
    if (chipwide) return select_units(&u, 1, 0, 0, 0, L, keep, pos ? P : 0, reforge, pos_out_stride, st);
    RTK_CHECK_ARG(rank, "rtk_pivotkv_select: the one-workgroup path needs the rank buffer");
    const int per = (L + PSEL_BLOCK - 1) / PSEL_BLOCK;
    if (per <= SEL_LDS_MAX_PER) {
        select_lds_opt_in();
        RTK_LAUNCH(KID_PSEL, pivotkv_select_lds_units_kernel, dim3(1), dim3(PSEL_BLOCK), select_lds_bytes(L, keep), st,
                   pad_units<SelUnits>(&u, 1), L, keep, pos ? P : 0, reforge, pos_out_stride);
    } else   // longer rows: keys re-read from memory on every pass
        RTK_LAUNCH(KID_PSEL, pivotkv_select_kernel, dim3(1), dim3(PSEL_BLOCK), 0, st, score, mask, L, keep, pos, P,
                   reforge, keep_idx, rank, pos_out, pos_out_stride);
    RTK_LAUNCH_CHECK("pivotkv_select_kernel");
    return RTK_OK;
}

// score_mfma.cuh — building blocks of the head_dim-128 score kernels (score_f32.cuh, score_dma.cuh,
// score_refround.cuh) and of the kernels that write their operands (pivotkv_prepare.hip): vector types, the 16-bit
// packing helpers, the matrix-instruction wrappers with their operand layout, the XOR-swizzled LDS tile and the
// per-block softmax helpers.  No kernels here.
#pragma once
#include "common.cuh"

// LLVM sched_group_barrier mask
#define SGB_MFMA 0x8

namespace rtk {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int HD = 128;       // head_dim of the MFMA path
constexpr int TILE_ROWS = 64; // rows of the streamed LDS tile
constexpr int REG_ROWS = 128; // rows held in registers per workgroup (32 per wave)
constexpr int SC_BLOCK = 256;
constexpr int NXCD = 8;      // MI355X: 8 XCDs, workgroup b is dispatched to XCD b % 8

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
// RTK_BF16_FAST operands of a 16-byte chunk (bf_lo / bf_hi / pack2_f16: common.cuh)
__device__ __forceinline__ u32x4 bf16x8_to_f16x8(const u32x4& v, float scale) {
    return u32x4{pack2_f16(bf_lo(v.x) * scale, bf_hi(v.x) * scale), pack2_f16(bf_lo(v.y) * scale, bf_hi(v.y) * scale),
                 pack2_f16(bf_lo(v.z) * scale, bf_hi(v.z) * scale), pack2_f16(bf_lo(v.w) * scale, bf_hi(v.w) * scale)};
}

// ------------------------------------------------------------------------------------------------
// MFMA building blocks (head_dim 128).  A "chunk" is 16 bytes of a row.
//   bf16: 16 chunks/row; MFMA step s (K=16) uses chunk 2s + half   (half = lane >> 5)
//   fp32: 32 chunks/row; the k axis is re-associated so that half `hf` owns k in [64hf, 64hf+64):
//         chunk 16hf + c feeds MFMAs 4c..4c+3 (K=2 each).  The same permutation is applied to both
//         operands, so every product a_k*b_k still meets its partner; only the summation order
//         differs from index order, which fp32 parity tolerates.
// ------------------------------------------------------------------------------------------------
template <int DT> struct MM;

template <> struct MM<RTK_BF16> {
    static constexpr int ESIZE = 2;
    static constexpr int CHUNKS = 16;            // per row
    static constexpr int NREG = 8;               // 16-byte registers per lane for a 32-row fragment
    __device__ static __forceinline__ int chunk_of(int r, int hf) { return 2 * r + hf; }
    __device__ static __forceinline__ void mma(f32x16& acc, const u32x4& a, const u32x4& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                      acc, 0, 0, 0);
    }
};

template <> struct MM<RTK_F32> {
    static constexpr int ESIZE = 4;
    static constexpr int CHUNKS = 32;
    static constexpr int NREG = 16;
    __device__ static __forceinline__ int chunk_of(int r, int hf) { return 16 * hf + r; }
    __device__ static __forceinline__ void mma(f32x16& acc, const u32x4& a, const u32x4& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
};

template <int DT> struct Tile {
    using M = MM<DT>;
    static constexpr int ROWB = M::CHUNKS * 16;                    // bytes per row (256 / 512)
    static constexpr int BYTES = TILE_ROWS * ROWB;                 // one LDS tile
    static constexpr int STAGE = (TILE_ROWS * M::CHUNKS) / SC_BLOCK;  // 16-byte chunks per thread per tile (4 / 8)
    static constexpr int ROWS_PER_STEP = SC_BLOCK / M::CHUNKS;     // rows between a thread's consecutive chunks (16 / 8)
};

// accumulator register r of lane (half hf) holds output row  m = (r&3) + 8*(r>>2) + 4*hf
__device__ __forceinline__ int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

// Register fragment: row (lane & 31) of a 32-row block starting at `row0` of a contiguous [rows,128] matrix.
template <int DT>
__device__ __forceinline__ void load_reg_frag(const char* __restrict__ base, int row0, int nrows, int lane,
                                              u32x4* rf, int pitch = HD * MM<DT>::ESIZE) {
    using M = MM<DT>;
    const int row = row0 + (lane & 31), hf = lane >> 5;
    const bool ok = row < nrows;
    const u32x4* p = (const u32x4*)(base + (size_t)row * pitch);   // pitch: bytes between rows (a strided projection)
#pragma unroll
    for (int r = 0; r < M::NREG; ++r) rf[r] = ok ? p[M::chunk_of(r, hf)] : u32x4{0, 0, 0, 0};
}

// Per-thread constants of the streamed-tile pipeline, computed once per kernel:
//   frag_off[r]  LDS byte offset (inside a tile, block 0) of this lane's r-th A-fragment chunk
//   st_off[u]    LDS byte offset where this thread stores its u-th staged chunk
//   voff[u]      byte offset of the u-th staged chunk inside the tile's source rows (buffer-load voffset)
// 16-byte chunks are XOR-swizzled by (row & 15): the 16 lanes of every ds_read_b128 lane group address
// 16 distinct rows (mod 16) => 16 distinct 16-byte bank slots; no bank conflicts (SQ_LDS_BANK_CONFLICT = 0).
template <int DT> struct Pipe {
    using M = MM<DT>;
    using T = Tile<DT>;
    int frag_off[M::NREG];
    int st_off[T::STAGE];
    int voff[T::STAGE];  // byte offsets of this thread's staged chunks inside a tile's source rows
    int srow;            // first staged row of this thread inside the tile
    __device__ __forceinline__ void init(int tid, int lane) {
        const int row = lane & 31, hf = lane >> 5;
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) frag_off[r] = row * T::ROWB + ((M::chunk_of(r, hf) ^ (row & 15)) * 16);
        srow = tid / M::CHUNKS;
        const int ch = tid % M::CHUNKS;
#pragma unroll
        for (int u = 0; u < T::STAGE; ++u) {
            const int rr = srow + u * T::ROWS_PER_STEP;
            st_off[u] = rr * T::ROWB + ((ch ^ (rr & 15)) * 16);
            voff[u] = rr * T::ROWB + ch * 16;
        }
    }
    // global -> registers (issued early, consumed late) through a buffer descriptor: the per-thread byte
    // offsets are precomputed once, the tile offset travels in an SGPR, so a tile costs STAGE
    // buffer_load_dwordx4 and no address arithmetic.  Branch-free: rows past the end of the matrix are out
    // of the descriptor's range and read as zeros; rows past the caller's valid range hold finite filler
    // whose logits the callers mask out.  (A load inside a conditional would force vmcnt(0) at the join.)
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rsrc, int first_row, u32x4* st) const {
        const int soff = first_row * T::ROWB;
#pragma unroll
        for (int u = 0; u < T::STAGE; ++u)
            st[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[u], soff, 0));
    }
    __device__ __forceinline__ void store(char* lds_tile, const u32x4* st) const {
#pragma unroll
        for (int u = 0; u < T::STAGE; ++u) *(u32x4*)(lds_tile + st_off[u]) = st[u];
    }
    // explicit two-step form: fetch all A fragments of a block, then run the MFMAs on them
    __device__ __forceinline__ void read_frags(u32x4* a, const char* lds_tile, int blk) const {
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) a[r] = *(const u32x4*)(lds_tile + blk * 32 * T::ROWB + frag_off[r]);
    }
    __device__ __forceinline__ void mma_frags(f32x16& acc, const u32x4* a, const u32x4* rf) const {
#pragma unroll
        for (int r = 0; r < M::NREG; ++r) M::mma(acc, a[r], rf[r]);
    }
};

__device__ __forceinline__ float max16(const f32x16& a) {
    return fmaxf(fmaxf(fmaxf(fmaxf(a[0], a[1]), a[2]), fmaxf(fmaxf(a[3], a[4]), a[5])),
                 fmaxf(fmaxf(fmaxf(fmaxf(a[6], a[7]), a[8]), fmaxf(fmaxf(a[9], a[10]), a[11])),
                       fmaxf(fmaxf(fmaxf(a[12], a[13]), a[14]), a[15])));
}

// D = A x B + C on the bf16 (exact mode) or fp16 (RTK_BF16_FAST) matrix instruction; D and C may be different registers
template <bool FAST>
__device__ __forceinline__ void mma16(f32x16& d, const u32x4& a, const u32x4& b, const f32x16& c) {
    if constexpr (FAST)
        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// col += sum_r exp2(acc[r] * c2 - ls[r]) for one 32x32 block (16 values per lane), log2 domain (the 16-bit kernels)
__device__ __forceinline__ void colsum_block(float& col, const f32x16& acc, const float* ls, float c2) {
    // scalar fma / exp2 / add per logit: v_pk_fma_f32 / v_pk_add_f32 were measured 5-7 % SLOWER here
    // (packed f32 ops cost extra issue slots beside MFMAs)
#pragma unroll
    for (int r = 0; r < 16; ++r) col += __builtin_amdgcn_exp2f(fmaf(acc[r], c2, -ls[r]));
}
// this lane's 16 row normalisers of block `blk` (rows (r&3) + 8*(r>>2) + 4*hf)
__device__ __forceinline__ void load_ls(float* ls, const float* lcur, int blk, int hf) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) *(float4*)(ls + 4 * r4) = *(const float4*)(lcur + blk * 32 + 8 * r4 + 4 * hf);
}

}  // namespace rtk

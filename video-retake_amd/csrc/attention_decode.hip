// attention_decode.hip — the chunk attention of attention.hip for FEW query rows (decode steps, short trailing text),
// GQA-packed (retake_hip.h "Chunk attention", rtk_attention_decode):
//
//   out[i, h, :] = softmax_j(q[h, i, :] . k[h / G, j, :] * scale) . v[h / G, j, :]      j <= q_offset + i, j < Lk
//
// for bf16 / fp16, head_dim 128 and R = G * Lq <= 16.  attn_decode_d128_kernel:
//   * a workgroup = 4 waves = one kv head x one key range (grid nsplit x Hkv).  The R rows (g, i) of the kv head - packed
//     row g * Lq + i is row i of query head hkv * G + g - are the 16 columns of one 16x16x32 MFMA operand, so a K or V row
//     is fetched from HBM once per call, not once per query head;
//   * the range's 32-key tiles go to the waves round robin (tile u of the range to wave u & 3); a wave's K rows go
//     global -> registers and ARE the A operand of S^T = mfma(K, Q) (lane: key lane & 15, 8 channels per k-step), its V
//     rows global -> registers -> a wave-private LDS image, read back transposed (ds_read_b64_tr_b16) as the A operand of
//     O^T = mfma(V^T, P^T).  No workgroup barrier in the key loop; the next tile's loads are issued as soon as the current
//     tile's registers are consumed and stay in flight under its softmax and PV products;
//   * a lane owns ONE packed row (column lane & 15): 8 of a tile's 32 logits, and 4 channels of each of O's 8 d-blocks, so
//     the running rescale is lane-local and max / sum need the lanes 16 and 32 apart;
//   * causal by index per packed row.  A tile holding keys that only some rows see (j > q_offset) runs its PV products
//     once per query position i with the V rows above i's diagonal zeroed, each lane keeping the pass of its own row: a
//     hidden V row reaches no row that does not see it, whatever it holds;
//   * each wave keeps its own (m, l, acc); the four are folded through LDS in wave order 0, 1, 2, 3 and the workgroup
//     leaves ONE un-normalised partial per packed row in the layout attn_combine_kernel reads, which then runs unchanged.
//     No atomics, no flags; plain vector stores.
// The plan (decode_plan) is a function of the shape alone.  attn_decode_d128_shared_kernel is the same body
// (attention_decode_d128_body.inc) with another buffer's 16-bit rows between the archive and the kernel's own
// (rtk_attention_decode_shared); attn_decode_group_d128_kernel (rtk_attention_decode_group, below) serves one token of
// several branches; attn_decode_wide_d128_kernel (attention_decode_wide.cuh, rtk_attention_decode_wide*) serves
// 16 < R <= 64 packed rows as two to four column groups; attn_decode_paged_d128_kernel (attention_decode_paged.cuh,
// rtk_attention_decode_paged / _sparse) reads the middle of ONE buffer through a per-kv-head page list, and
// attn_decode_paged_fp8kv_d128_kernel (the same file, rtk_attention_decode_paged_fp8kv / _sparse_fp8kv) the e4m3 archive;
// attn_decode_paged_wide_d128_kernel (the same file, rtk_attention_decode_paged_wide / _sparse_wide) is the wide kernel's
// body over the 16-bit page walk.  The body, the group kernel and the wide kernel share
// dec_step_off, dec_v_frag and dec_softmax_step; their tile loads, dequantise-and-stage step and four-wave fold are
// written in each (as shared functions they compile the existing kernels differently).  Host side: the entry
// points of the narrow and the wide family are decode_call with their family and segments - its checks and fall-throughs,
// then decode_forward (operands, plan, workspace, dtype) -> decode_launch -> decode_launch_d128, the one launcher; the
// six page-sparse entry points are paged_call with their family, their names, their kind (16-bit rows / fp8 archive) and
// a page list or summaries - one shape check, one operand check, one bound -> select -> paged chain, one launcher.
// FP8 = true: the keys are [e4m3 archive | 16-bit rows], counted in a key space where the archive is padded to whole
// 32-key tiles (a tile is of one kind).  Archive tiles are dequantised (fp8_dequant16) into the registers / the LDS image
// a 16-bit tile of the dequantised rows would have left, so with L8 % 32 == 0 every fp32 sum is grouped as in the 16-bit
// call over the concatenation.  (The k-steps of S^T take channels 64 a + 16 g + 8 b + j, step 2 a + b, lane group g: 16
// consecutive codes of a row dequantise into one lane's operands of two steps.)
#include <algorithm>
#include <vector>

#include "attention_shared.cuh"

namespace rtk {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using i16x4 = __attribute__((ext_vector_type(4))) short;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

constexpr int DEC_R = 16;                 // packed rows a workgroup serves: the MFMA's columns
constexpr int DEC_T = 32;                 // keys per wave tile: the key tile T of retake_hip.h
constexpr int DEC_STEP = 4 * DEC_T;       // keys the four waves take side by side: the granularity of a split
constexpr int DEC_TARGET_WG = 512;        // workgroups wanted (2 per CU; a constant, not a device query)
constexpr int DEC_VPITCH = 288;           // bytes per V row in LDS: 256 + 32, so the 8 rows a 32-lane half reads tile the banks
constexpr int DEC_WAVE_LDS = DEC_T * DEC_VPITCH;
constexpr int DEC_OPITCH = 132;           // floats per packed row of a wave's O image (the fold)
static_assert(DEC_R * DEC_OPITCH * 4 <= DEC_WAVE_LDS, "a wave's O image reuses its V image");

template <int DT> __device__ __forceinline__ f32x4 mma32(const u32x4& a, const u32x4& b, const f32x4& c) {
    if constexpr (DT == RTK_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// the wave's LDS writes before, its LDS reads after (the image is wave-private: no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the byte offset, within a 256-byte row, of the 16-byte chunk a lane of group g feeds to k-step s
__device__ __forceinline__ int dec_step_off(int s, int g) { return 128 * (s >> 1) + 32 * g + 16 * (s & 1); }

// The A operand of O^T = mfma(V^T, P^T) for d-block db, read transposed from a wave's V image: `vrd` = the image + the
// lane's v_rd
__device__ __forceinline__ u32x4 dec_v_frag(const char* vrd, int db) {
    u32x2 h2[2];
#pragma unroll
    for (int jh = 0; jh < 2; ++jh) {
        const i16x4 t4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) i16x4*)(vrd + DEC_VPITCH * 16 * jh + 32 * db));
        h2[jh] = __builtin_bit_cast(u32x2, t4);
    }
    return u32x4{h2[0][0], h2[0][1], h2[1][0], h2[1][1]};
}

// One tile's step of the online softmax of the lane's packed row: s0 / s1 are its 8 raw logits (masked ones -inf), the
// other 24 sit in the lanes 16 and 32 apart.  Rescales the running (m, l, oacc) and returns the probabilities packed as
// the B operand of O^T = mfma(V^T, P^T).
template <int DT>
__device__ __forceinline__ u32x4 dec_softmax_step(f32x4 s0, f32x4 s1, float c2, float& m, float& l, f32x4 (&oacc)[8]) {
    using Hh = H16<DT>;
    float mx = fmaxf(fmaxf(fmaxf(s0[0], s1[0]), fmaxf(s0[1], s1[1])), fmaxf(fmaxf(s0[2], s1[2]), fmaxf(s0[3], s1[3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mnew = fmaxf(m, mx * c2);
    const float alpha = __builtin_amdgcn_exp2f(m - safe_max(mnew));
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] *= alpha;
    l *= alpha;
    m = mnew;
    const float nm = -safe_max(m);
    float ls = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s0[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], c2, nm));
        s1[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[e], c2, nm));
        ls += s0[e] + s1[e];
    }
    l += ls;
    return u32x4{Hh::pack2(s0[0], s0[1]), Hh::pack2(s0[2], s0[3]), Hh::pack2(s1[0], s1[1]), Hh::pack2(s1[2], s1[3])};
}

template <int DT, bool FP8>
__global__ __launch_bounds__(256, 2) void attn_decode_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq,
    int G, int Lq, int Lk, int off, float c2, int keys_per_split, Archive8 a8) {
    constexpr bool SHARED = false;
    const Shared16 s16{};
#include "attention_decode_d128_body.inc"
}

// the same body over [e4m3 archive (may be empty) | shared 16-bit rows | own 16-bit rows]: Lk and off describe the own rows
template <int DT>
__global__ __launch_bounds__(256, 2) void attn_decode_d128_shared_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq,
    int G, int Lq, int Lk, int off, float c2, int keys_per_split, Archive8 a8, Shared16 s16) {
    constexpr bool FP8 = true, SHARED = true;
#include "attention_decode_d128_body.inc"
}

#include "attention_decode_wide.cuh"
#include "attention_decode_paged.cuh"

struct DecodePlan {
    int nsplit, keys_per_split;
    size_t ws_bytes;
};

// retake_hip.h states this rule; a function of the shape alone.  `keys`: Lk, plus the archive padded to whole tiles.
DecodePlan decode_plan(int Hq, int Hkv, int Lq, long long keys) {
    long long ns = (DEC_TARGET_WG + Hkv - 1) / Hkv;
    const long long by_keys = (keys + DEC_STEP - 1) / DEC_STEP;
    if (ns > by_keys) ns = by_keys;
    if (ns < 1) ns = 1;
    long long kps = (keys + ns - 1) / ns;
    kps = (kps + DEC_STEP - 1) / DEC_STEP * DEC_STEP;
    ns = (keys + kps - 1) / kps;
    return DecodePlan{(int)ns, (int)kps, (size_t)ns * Hq * Lq * (128 + 2) * sizeof(float)};
}

// The two families of packed entry points, each [plain, _fp8kv, _shared] (`seg` 0, 1, 2): the narrow one (one column group)
// and the wide one (attention_decode_wide.cuh), which at R <= DEC_R IS the narrow one.
struct DecodeFamily {
    const char *who[3], *query[3], *kernel;
    int max_rows;
};
const DecodeFamily DEC_NARROW{
    {"rtk_attention_decode", "rtk_attention_decode_fp8kv", "rtk_attention_decode_shared"},
    {"rtk_attention_decode_workspace_bytes", "rtk_attention_decode_workspace_bytes_fp8kv", "rtk_attention_decode_workspace_bytes_shared"},
    "packed", DEC_R};
const DecodeFamily DEC_WIDE{
    {"rtk_attention_decode_wide", "rtk_attention_decode_wide_fp8kv", "rtk_attention_decode_wide_shared"},
    {"rtk_attention_decode_wide_workspace_bytes", "rtk_attention_decode_wide_workspace_bytes_fp8kv",
     "rtk_attention_decode_wide_workspace_bytes_shared"},
    "wide", WIDE_R};
// the shared rows and the archive as an entry point receives them: zero where its call has none
struct DecodeSegs {
    const void *ks, *vs;
    int Ls;
    int64_t s_sh, s_sl;
    const void *k8, *v8;
    const float *k_scale, *v_scale;
    int L8;
    int64_t sh8, shs;
};

// what a packed kernel takes of the shapes attn_check_shape admits
int decode_check_envelope(const char* who, const DecodeFamily& f, int Hq, int Hkv, int Lq, int D, int dtype) {
    const int rc = d128_check_envelope(who, f.kernel, D, dtype);
    if (rc != RTK_OK) return rc;
    if ((long long)(Hq / Hkv) * Lq > f.max_rows) {
        set_error("%s: unsupported shape: (Hq / Hkv) * Lq = %d * %d packed rows (at most %d)", who, Hq / Hkv, Lq, f.max_rows);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}
// the shape check of the segments the call has, then the family's envelope
int decode_check_shape(const char* who, const DecodeFamily& f, int seg, int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D,
                       int dtype) {
    const int rc = seg == 2   ? shared_check_shape(who, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype, DEC_T)
                   : seg == 1 ? fp8kv_check_shape(who, Hq, Hkv, Lq, Lk, L8, D, dtype)
                              : attn_check_shape(who, Hq, Hkv, Lq, Lk, D, dtype);
    return rc != RTK_OK ? rc : decode_check_envelope(who, f, Hq, Hkv, Lq, D, dtype);
}
// a workspace query: 0 with the error set for a shape the family does not take
size_t decode_query(const DecodeFamily& f, int seg, int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype) {
    if (decode_check_shape(f.query[seg], f, seg, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype) != RTK_OK) return 0;
    return decode_plan(Hq, Hkv, Lq, shared_keys(Lk, L8, Ls, DEC_T)).ws_bytes;
}

// One launch of a packed kernel variant (`tail`: the a8 / s16 it takes after the common parameters), then the combine.
template <int DT, class K, class... Tail>
int decode_launch_d128(K kern, const char* name, const DecodePlan& pl, const AttnArgs& a, const Tail&... tail) {
    const Partials p = split_partials(a.workspace, pl.nsplit, a.Hq, a.Lq, 128);
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.nsplit, (unsigned)a.Hkv), dim3(256), 0, a.st, (const char*)a.q, a.q_sh, a.q_sl,
                       (const char*)a.k, (const char*)a.v, a.kv_sh, (uint32_t)(a.kv_sl * 2), rows_extent(a.Lk, a.kv_sl, 128, 2), p.acc,
                       p.ml, a.Hq, a.Hq / a.Hkv, a.Lq, a.Lk, a.off, base2_scale(a.scale), pl.keys_per_split, tail...);
    RTK_LAUNCH_CHECK(name);
    return attn_combine<DT>(p, a.out, a.Hq, a.Lq, 128, pl.nsplit, a.st);
}

// the wide kernel of the call's column groups
template <int DT, bool FP8, bool SHARED> int wide_launch(const DecodePlan& pl, const AttnArgs& a, const Archive8& a8, const Shared16& s16) {
    const char* name = "attn_decode_wide_d128_kernel";
    switch (((a.Hq / a.Hkv) * a.Lq + DEC_R - 1) / DEC_R) {
    case 2: return decode_launch_d128<DT>(attn_decode_wide_d128_kernel<DT, 2, FP8, SHARED>, name, pl, a, a8, s16);
    case 3: return decode_launch_d128<DT>(attn_decode_wide_d128_kernel<DT, 3, FP8, SHARED>, name, pl, a, a8, s16);
    default: return decode_launch_d128<DT>(attn_decode_wide_d128_kernel<DT, 4, FP8, SHARED>, name, pl, a, a8, s16);
    }
}

// the kernel of the segments the call has: [archive | shared | own], a8 / s16 empty without
template <int DT> int decode_launch(const DecodePlan& pl, const AttnArgs& a, const Archive8& a8, const Shared16& s16, bool wide) {
    if (wide) {
        if (s16.Ls > 0) return wide_launch<DT, true, true>(pl, a, a8, s16);
        if (a8.L8 > 0) return wide_launch<DT, true, false>(pl, a, a8, s16);
        return wide_launch<DT, false, false>(pl, a, a8, s16);
    }
    if (s16.Ls > 0) return decode_launch_d128<DT>(attn_decode_d128_shared_kernel<DT>, "attn_decode_d128_shared_kernel", pl, a, a8, s16);
    if (a8.L8 > 0) return decode_launch_d128<DT>(attn_decode_d128_kernel<DT, true>, "attn_decode_d128_kernel", pl, a, a8);
    return decode_launch_d128<DT>(attn_decode_d128_kernel<DT, false>, "attn_decode_d128_kernel", pl, a, a8);
}

// What the entry points share once their own checks are through: the operands, the plan over the padded key count,
// the workspace (`query`: the entry point that sizes it) and the dtype switch.
int decode_forward(const char* who, const char* query, bool wide, const AttnArgs& a, const Archive8& a8, const Shared16& s16) {
    int rc = attn_check_operands(who, a.q, a.q_sh, a.q_sl, a.k, a.v, a.kv_sh, a.kv_sl, a8.k8, a8.v8, a8.ks, a8.vs, a8.sh8, a8.shs,
                                 a.out, a.Lq, a.Lk, a.off, a.D, a.dtype, a.scale, 0, DEC_T);
    if (rc != RTK_OK) return rc;
    const DecodePlan pl = decode_plan(a.Hq, a.Hkv, a.Lq, shared_keys(a.Lk, a8.L8, s16.Ls, DEC_T));
    rc = attn_check_workspace(who, query, pl.ws_bytes, a.workspace, a.workspace_bytes);
    if (rc != RTK_OK) return rc;
    return a.dtype == RTK_BF16 ? decode_launch<RTK_BF16>(pl, a, a8, s16, wide) : decode_launch<RTK_F16>(pl, a, a8, s16, wide);
}

// An entry point of family f with segments `seg`: its checks, then its fall-throughs - the wide family at R <= DEC_R is
// the narrow call of the same segments; without shared rows the _shared call is the _fp8kv call, which without an archive
// is the plain one - then decode_forward.
int decode_call(const DecodeFamily& f, int seg, const AttnArgs& a, const DecodeSegs& sg) {
    const char* who = f.who[seg];
    RTK_CHECK_ARG(a.q && a.k && a.v && a.out, "%s: NULL q / k / v / out pointer", who);
    int rc = decode_check_shape(who, f, seg, a.Hq, a.Hkv, a.Lq, a.Lk, sg.L8, sg.Ls, a.D, a.dtype);
    if (rc != RTK_OK) return rc;
    if (f.max_rows > DEC_R && (a.Hq / a.Hkv) * a.Lq <= DEC_R) return decode_call(DEC_NARROW, seg, a, sg);
    if (seg == 2 && sg.Ls == 0) return decode_call(f, 1, a, sg);
    if (seg == 1 && sg.L8 == 0) return decode_call(f, 0, a, sg);
    Shared16 s16{};
    Archive8 a8{};
    if (seg == 2) {
        rc = make_shared16(who, sg.ks, sg.vs, sg.Ls, sg.s_sh, sg.s_sl, a.D, DEC_T, s16);
        if (rc != RTK_OK) return rc;
    }
    if (seg >= 1) {
        rc = make_archive8(who, sg.k8, sg.v8, sg.k_scale, sg.v_scale, sg.L8, sg.sh8, sg.shs, a8);
        if (rc != RTK_OK) return rc;
    }
    return decode_forward(who, f.query[seg], f.max_rows > DEC_R, a, a8, s16);
}

// ---- group decode (rtk_attention_decode_group): ONE token of each of B branches that share [archive | shared rows] ----
// attn_decode_group_d128_kernel, grid (ns_sh + B * max_own) x Hkv:
//   * x < ns_sh: a SHARED workgroup - one kv head, one range of the padded [archive L8p | shared Lsp] key space.  Its
//     columns are all R = B * G packed rows, row b * G + g from branch b; with R > 16 (NCG = 2) the K fragments in
//     registers feed a second S^T = mfma(K, Q) against a second set of Q fragments and the V image in LDS a second
//     O^T = mfma(V^T, P^T), so a K or V row is fetched from HBM once per call whatever B is;
//   * x >= ns_sh: an OWN workgroup - branch (x - ns_sh) / max_own, keys [j * GRP_OWN_KEYS, ...) of that branch's own rows,
//     j = (x - ns_sh) % max_own; its columns are that branch's G rows.  A branch with no keys in split j leaves an empty
//     partial (m = -inf), which attn_combine_kernel skips.
// The query is each branch's last own row, so every row sees every key: no diagonal.  The tile loop, the softmax and the
// fold of the four waves are those of attention_decode_d128_body.inc, once per column group; partials go to
// [split][branch * Hq + head] - the layout attn_combine_kernel reads with (branch, head) as the head index - shared
// splits first, then own splits.  A column's arithmetic depends on no other column, so a branch's bits depend neither
// on its position in the group nor on the other members.  No atomics, no flags; plain vector stores.
constexpr int GRP_OWN_KEYS = RTK_DECODE_GROUP_OWN_KEYS;   // keys per own split: retake_hip.h states it

struct GroupBranch {
    const char *q, *k, *v;
    int64_t q_sh, kv_sh;                // head strides, elements
    uint32_t kv_row_bytes, kv_bytes;    // row stride; extent of one head: the descriptor's bound
    int Lk, pad;
};
struct GroupArgs {
    GroupBranch br[RTK_DECODE_GROUP_MAX];
    int B, G, Hq, ns_sh, kps_sh, max_own;
};

template <int DT, int NCG>
__global__ __launch_bounds__(256, 2) void attn_decode_group_d128_kernel(GroupArgs ga, Archive8 a8, Shared16 s16,
                                                                        float* __restrict__ part_acc,
                                                                        float* __restrict__ part_ml, float c2) {
    constexpr int NR = NCG * DEC_R;                                                   // columns of the workgroup
    constexpr int WAVE_LDS = NR * DEC_OPITCH * 4 > DEC_WAVE_LDS ? NR * DEC_OPITCH * 4 : DEC_WAVE_LDS;
    __shared__ __attribute__((aligned(16))) char lds[4 * WAVE_LDS];   // [wave]: V tile, then the wave's O
    __shared__ float ml_s[4][NR][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // column within a group and lane group
    const int hkv = blockIdx.y, G = ga.G;
    const bool own = (int)blockIdx.x >= ga.ns_sh;
    const int ox = own ? (int)blockIdx.x - ga.ns_sh : 0, ob = ox / ga.max_own, oj = ox % ga.max_own;
    GroupBranch me = ga.br[0];   // (selected, not indexed: the array stays in the kernel argument segment)
#pragma unroll
    for (int b = 1; b < RTK_DECODE_GROUP_MAX; ++b)
        if (ob == b) me = ga.br[b];
    const int nrows = own ? G : ga.B * G;
    // the key space of this workgroup: [archive tiles [0, archp) | 16-bit rows from archp on]
    const int L8 = a8.L8, L8p = (L8 + DEC_T - 1) / DEC_T * DEC_T;
    const int Lsp = (s16.Ls + DEC_T - 1) / DEC_T * DEC_T;
    const int archp = own ? 0 : L8p;
    const int keys = own ? me.Lk : L8p + Lsp;
    const int vis16 = own ? me.Lk - 1 : L8p + s16.Ls - 1;   // last key of the 16-bit segment
    const int span = own ? GRP_OWN_KEYS : ga.kps_sh;
    const int k_lo = (own ? oj : (int)blockIdx.x) * span, k_hi = min(keys, k_lo + span);
    const uint32_t row_bytes = own ? me.kv_row_bytes : s16.row_bytes;

    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(own ? me.k + (int64_t)hkv * me.kv_sh * 2 : s16.k + (int64_t)hkv * s16.sh * 2,
                                                   own ? me.kv_bytes : s16.bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(own ? me.v + (int64_t)hkv * me.kv_sh * 2 : s16.v + (int64_t)hkv * s16.sh * 2,
                                                   own ? me.kv_bytes : s16.bytes);
    const __amdgpu_buffer_rsrc_t rk8 = bounded_rsrc(a8.k8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
    const __amdgpu_buffer_rsrc_t rv8 = bounded_rsrc(a8.v8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
    const __amdgpu_buffer_rsrc_t rks = bounded_rsrc(a8.ks + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
    const __amdgpu_buffer_rsrc_t rvs = bounded_rsrc(a8.vs + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);

    // Q fragments (B operand) of column group cg: packed row 16 cg + c, zero past the workgroup's rows
    u32x4 qf[NCG][4];
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[cg][s] = u32x4{0u, 0u, 0u, 0u};
        const int r = 16 * cg + c;
        if (r < nrows) {
            const int bi = own ? ob : r / G, gi = own ? r : r % G;
            const char* qb = ga.br[0].q;
            int64_t qsh = ga.br[0].q_sh;
#pragma unroll
            for (int b = 1; b < RTK_DECODE_GROUP_MAX; ++b)
                if (bi == b) {
                    qb = ga.br[b].q;
                    qsh = ga.br[b].q_sh;
                }
            const char* qr = qb + (int64_t)(hkv * G + gi) * qsh * 2;
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[cg][s] = *(const u32x4*)(qr + dec_step_off(s, g));
        }
    }

    // one tile's operands, laid out as in attention_decode_d128_body.inc
    u32x4 kr[8], vr[8];
    auto load_k = [&](int kb) {
        if (kb < archp) {   // rows >= L8 of the last archive tile: zero codes, zero scales
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const uint32_t row = (uint32_t)(kb + 16 * b + c);
#pragma unroll
                for (int a = 0; a < 2; ++a) kr[2 * b + a] = load16(rk8, row * 128u + 16u * (4 * a + g));
                kr[4][b] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rks, row * 4u, 0, 0);
            }
            return;
        }
        kb -= archp;   // rows past the segment's end read as zero
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s) kr[4 * b + s] = load16(rk, (uint32_t)(kb + 16 * b + c) * row_bytes + (uint32_t)dec_step_off(s, g));
    };
    auto load_v = [&](int kb) {
        if (kb < archp) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t row = (uint32_t)(kb + 8 * u + (lane >> 3));
                vr[u] = load16(rv8, row * 128u + 16u * (lane & 7));
                vr[4][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rvs, row * 4u, 0, 0);
            }
            return;
        }
        kb -= archp;
#pragma unroll
        for (int u = 0; u < 8; ++u) vr[u] = load16(rv, (uint32_t)(kb + 4 * u + g) * row_bytes + 16u * c);
    };

    char* vt = lds + wave * WAVE_LDS;
    const int v_rd = DEC_VPITCH * (4 * g + (c >> 2)) + 8 * (c & 3);

    f32x4 oacc[NCG][8];
    float m[NCG], l[NCG];
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
#pragma unroll
        for (int db = 0; db < 8; ++db) oacc[cg][db] = f32x4{0.f, 0.f, 0.f, 0.f};
        m[cg] = -INFINITY;
        l[cg] = 0.f;
    }

    auto process = [&](int kb, bool next) {
        const bool arch = kb < archp;
        u32x4 ka[8];
        if (arch) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    fp8_dequant16<DT>(kr[2 * b + a], __uint_as_float(kr[4][b]), ka[4 * b + 2 * a], ka[4 * b + 2 * a + 1]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                u32x4 x, y;
                fp8_dequant16<DT>(vr[u], __uint_as_float(vr[4][u]), x, y);
                char* w = vt + DEC_VPITCH * (8 * u + (lane >> 3)) + 32 * (lane & 7);
                *(u32x4*)w = x;
                *(u32x4*)(w + 16) = y;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ka[e] = kr[e];
#pragma unroll
            for (int u = 0; u < 8; ++u) *(u32x4*)(vt + DEC_VPITCH * (4 * u + g) + 16 * c) = vr[u];
        }
        if (next) load_v(kb + DEC_STEP);
        wave_lds_sync();
        // logits of column group cg: s0[e] = key 4 g + e, s1[e] = key 16 + 4 g + e of the tile
        f32x4 s0[NCG], s1[NCG];
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
            s0[cg] = f32x4{0.f, 0.f, 0.f, 0.f};
            s1[cg] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                s0[cg] = mma32<DT>(ka[s], qf[cg][s], s0[cg]);
                s1[cg] = mma32<DT>(ka[4 + s], qf[cg][s], s1[cg]);
            }
        }
        if (next) load_k(kb + DEC_STEP);
        const int lim = (arch ? L8 - 1 : vis16) - kb;   // the last key of the tile that exists; every row sees it
        u32x4 pf[NCG];
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (4 * g + e > lim) s0[cg][e] = -INFINITY;
                if (16 + 4 * g + e > lim) s1[cg][e] = -INFINITY;
            }
            pf[cg] = dec_softmax_step<DT>(s0[cg], s1[cg], c2, m[cg], l[cg], oacc[cg]);
        }
#pragma unroll
        for (int db = 0; db < 8; ++db) {   // one transposed read of the V image feeds every column group
            const u32x4 vf = dec_v_frag(vt + v_rd, db);
#pragma unroll
            for (int cg = 0; cg < NCG; ++cg) oacc[cg][db] = mma32<DT>(vf, pf[cg], oacc[cg][db]);
        }
        wave_lds_sync();   // the reads above before the next tile's writes
    };

    // this wave's tiles: u = wave, wave + 4, ... of the range
    const int kb0 = k_lo + DEC_T * wave;
    if (kb0 < k_hi) {
        load_k(kb0);
        load_v(kb0);
    }
    for (int kb = kb0; kb < k_hi; kb += DEC_STEP) process(kb, kb + DEC_STEP < k_hi);

    // fold the four waves in wave order; the workgroup leaves one partial per packed row
    {
        float* ow = (float*)vt;
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
            float lc = l[cg];
            lc += __shfl_xor(lc, 16, WAVE);
            lc += __shfl_xor(lc, 32, WAVE);
#pragma unroll
            for (int db = 0; db < 8; ++db) *(f32x4*)(ow + (16 * cg + c) * DEC_OPITCH + 16 * db + 4 * g) = oacc[cg][db];
            if (g == 0) {
                ml_s[wave][16 * cg + c][0] = m[cg];
                ml_s[wave][16 * cg + c][1] = lc;
            }
        }
    }
    __syncthreads();
    const int ch = tid & 15;   // channels 8 ch .. 8 ch + 7
    const size_t split = own ? (size_t)(ga.ns_sh + oj) : (size_t)blockIdx.x;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
        const int row = 16 * cg + (tid >> 4);   // packed row
        if (row >= nrows) continue;
        float mg = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mg = fmaxf(mg, ml_s[w][row][0]);
        f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = {0.f, 0.f, 0.f, 0.f};
        float den = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = ml_s[w][row][0];
            if (mw == -INFINITY) continue;   // the wave had no tile
            const float wt = __builtin_amdgcn_exp2f(mw - mg);
            const float* ow = (const float*)(lds + w * WAVE_LDS) + row * DEC_OPITCH + 8 * ch;
            const f32x4 a = *(const f32x4*)ow, b = *(const f32x4*)(ow + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                n0[e] = __builtin_fmaf(wt, a[e], n0[e]);
                n1[e] = __builtin_fmaf(wt, b[e], n1[e]);
            }
            den = __builtin_fmaf(wt, ml_s[w][row][1], den);
        }
        const int bi = own ? ob : row / G, gi = own ? row : row % G;
        const size_t prow = (split * ga.B + bi) * ga.Hq + (size_t)(hkv * G + gi);
        float* pa = part_acc + prow * 128 + 8 * ch;
        *(f32x4*)pa = n0;
        *(f32x4*)(pa + 4) = n1;
        if (ch == 0) *(float2*)(part_ml + 2 * prow) = make_float2(mg, den);
    }
}

// retake_hip.h states this rule: the shared split from (Hkv, L8, Ls) alone, the own split from a branch's Lk alone
struct GroupPlan {
    int ns_sh, kps_sh, max_own;
    size_t ws_bytes;
};
GroupPlan group_plan(const int* own_rows, int B, int Hq, int Hkv, int L8, int Ls) {
    GroupPlan gp{0, DEC_STEP, 1, 0};
    const long long keys = shared_keys(0, L8, Ls, DEC_T);
    if (keys > 0) {
        const DecodePlan pl = decode_plan(Hq, Hkv, 1, keys);
        gp.ns_sh = pl.nsplit;
        gp.kps_sh = pl.keys_per_split;
    }
    for (int b = 0; b < B; ++b) gp.max_own = std::max(gp.max_own, (own_rows[b] + GRP_OWN_KEYS - 1) / GRP_OWN_KEYS);
    gp.ws_bytes = (size_t)(gp.ns_sh + gp.max_own) * B * Hq * (128 + 2) * sizeof(float);
    return gp;
}

// what the group kernel takes: dtype, head_dim, the number of branches and of packed rows
int group_check_envelope(const char* who, int n_branches, int Hq, int Hkv, int D, int dtype) {
    const int rc = d128_check_envelope(who, "group", D, dtype);
    if (rc != RTK_OK) return rc;
    if (n_branches > RTK_DECODE_GROUP_MAX) {
        set_error("%s: unsupported group of %d branches (at most %d)", who, n_branches, RTK_DECODE_GROUP_MAX);
        return RTK_EUNSUPPORTED;
    }
    if ((long long)n_branches * (Hq / Hkv) > 2 * DEC_R) {
        set_error("%s: unsupported shape: n_branches * (Hq / Hkv) = %d * %d packed rows (at most %d)", who, n_branches, Hq / Hkv,
                  2 * DEC_R);
        return RTK_EUNSUPPORTED;
    }
    return RTK_OK;
}

template <int DT>
int group_launch(const GroupPlan& gp, const GroupArgs& ga, const Archive8& a8, const Shared16& s16, void* out, int Hkv, float c2,
                 void* ws, hipStream_t st) {
    const int nsplit = gp.ns_sh + gp.max_own, heads = ga.B * ga.Hq;
    const Partials p = split_partials(ws, nsplit, heads, 1, 128);
    const dim3 grid((unsigned)(gp.ns_sh + ga.B * gp.max_own), (unsigned)Hkv);
    const auto kern = ga.B * ga.G > DEC_R ? attn_decode_group_d128_kernel<DT, 2> : attn_decode_group_d128_kernel<DT, 1>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, ga, a8, s16, p.acc, p.ml, c2);
    RTK_LAUNCH_CHECK("attn_decode_group_d128_kernel");
    return attn_combine<DT>(p, out, heads, 1, 128, nsplit, st);
}

// ---- page-sparse decode (rtk_attention_decode_{paged,sparse}{,_fp8kv,_wide}; the kernels: attention_decode_paged.cuh) ----
// The six calls are paged_call (below) with their family, their names and what they take: `arch8` - the pages are the e4m3
// archive's (first = 0, ve = L8: the region is the archive), else rows [first, ve) of k / v - and a page list or, `sparse`,
// summaries.  The family is that of the packed entry points: DEC_WIDE (16-bit rows only) admits up to 64 packed rows and
// at R <= DEC_R IS the narrow call.
struct PagedGeom {
    int first, ve, keep_pages;
    int pages;             // ceil((ve - first) / 32)
    long long keys;        // the virtual key count: head padded to whole tiles + keep_pages tiles + the rows after the pages
};
// the shape checks of the paged calls, before anything is launched: those of rtk_attention_decode / _fp8kv, then the
// pages; `g` is filled on success
int paged_check_shape(const char* who, const DecodeFamily& f, bool arch8, int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype, int first, int ve,
                      int keep_pages, PagedGeom& g) {
    const int rc = decode_check_shape(who, f, arch8, Hq, Hkv, Lq, Lk, L8, 0, D, dtype);
    if (rc != RTK_OK) return rc;
    if (arch8) {
        RTK_CHECK_ARG(L8 >= 1, "%s: L8 %d: the call needs an archive (rtk_attention_decode serves a cache without one)", who, L8);
        first = 0, ve = L8;
    } else {
        RTK_CHECK_ARG(first >= 0 && first <= ve, "%s: first %d is not in [0, ve = %d]", who, first, ve);
        RTK_CHECK_ARG(ve <= Lk, "%s: ve %d exceeds Lk %d", who, ve, Lk);
    }
    const int pages = (int)(((long long)ve - first + DEC_T - 1) / DEC_T);
    RTK_CHECK_ARG(keep_pages >= 1 && keep_pages <= pages, "%s: keep_pages %d is not in [1, pages = %d]", who, keep_pages, pages);
    if (!arch8 && Lk > 0x3fffffff - 2 * DEC_T) {
        set_error("%s: unsupported extent: %d keys", who, Lk);
        return RTK_EUNSUPPORTED;
    }
    g = PagedGeom{first, ve, keep_pages, pages,
                  ((long long)first + DEC_T - 1) / DEC_T * DEC_T + (long long)keep_pages * DEC_T + (arch8 ? Lk : Lk - ve)};
    return RTK_OK;
}
// the operand checks: the archive (`a8` stays empty without), layout (RTK_EINVAL here, as retake_hip.h states for these
// calls), then what rtk_attention_decode / _fp8kv checks
int paged_check_operands(const char* who, bool arch8, const AttnArgs& a, const DecodeSegs& sg, const PagedGeom& g, Archive8& a8) {
    if (arch8) {
        const int rc = make_archive8(who, sg.k8, sg.v8, sg.k_scale, sg.v_scale, sg.L8, sg.sh8, sg.shs, a8);
        if (rc != RTK_OK) return rc;
    } else {
        RTK_CHECK_ARG(a.off >= g.ve - 1, "%s: q_offset %d < ve - 1 = %d (every query row sees the whole region)", who, a.off, g.ve - 1);
    }
    RTK_CHECK_ARG((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out | (uintptr_t)sg.k8 | (uintptr_t)sg.v8) & 15) == 0 &&
                      (a.q_sh * 2) % 16 == 0 && (a.q_sl * 2) % 16 == 0 && (a.kv_sh * 2) % 16 == 0 && (a.kv_sl * 2) % 16 == 0 &&
                      sg.sh8 % 16 == 0,
                  "%s: pointers and strides must be multiples of 16 bytes", who);
    RTK_CHECK_ARG((((uintptr_t)sg.k_scale | (uintptr_t)sg.v_scale) & 3) == 0, "%s: the scales must be 4-byte aligned", who);
    return attn_check_operands(who, a.q, a.q_sh, a.q_sl, a.k, a.v, a.kv_sh, a.kv_sl, a8.k8, a8.v8, a8.ks, a8.vs, a8.sh8, a8.shs, a.out,
                               a.Lq, a.Lk, a.off, a.D, a.dtype, a.scale, 0, DEC_T);
}
inline size_t align16(size_t b) { return (b + 15) / 16 * 16; }
// the workspace of a sparse call: [ub fp32 [Hkv, pages] | lists int32 [Hkv, keep_pages] | partials], each part starting at
// a multiple of 16 bytes; a paged call's is the partials alone
struct SparseLayout {
    size_t lists_at, partials_at, bytes;
};
SparseLayout sparse_layout(bool sparse, int Hkv, const PagedGeom& g, const DecodePlan& pl) {
    SparseLayout s{0, 0, pl.ws_bytes};
    if (sparse) {
        s.lists_at = align16((size_t)Hkv * g.pages * sizeof(float));
        s.partials_at = s.lists_at + align16((size_t)Hkv * g.keep_pages * sizeof(int32_t));
        s.bytes = s.partials_at + pl.ws_bytes;
    }
    return s;
}
int paged_check_workspace(const char* who, const char* query, size_t need, const void* workspace, size_t workspace_bytes) {
    RTK_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes; query %s)", who,
                  workspace ? workspace_bytes : (size_t)0, need, query);
    RTK_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    return RTK_OK;
}
// One launch of the paged kernel of the call's kind over `partials`, then the combine.  (The two kernels' parameter lists
// differ in their middle - kv_bytes - so the launch is written per kind, not as decode_launch_d128's trailing pack.)  More
// than DEC_R packed rows (the wide family's 16-bit calls; the checks admit no other) take the wide kernel of their column
// groups, whose parameter list is the 16-bit kind's.
template <int DT>
int paged_launch(bool arch8, const DecodePlan& pl, const AttnArgs& a, const Archive8& a8, const PagedGeom& g, const int32_t* list,
                 void* partials) {
    const Partials p = split_partials(partials, pl.nsplit, a.Hq, a.Lq, 128);
    const dim3 grid((unsigned)pl.nsplit, (unsigned)a.Hkv);
    const char *q = (const char*)a.q, *k = (const char*)a.k, *v = (const char*)a.v;
    const uint32_t row_bytes = (uint32_t)(a.kv_sl * 2);
    const float c2 = base2_scale(a.scale);
    const int ncg = ((a.Hq / a.Hkv) * a.Lq + DEC_R - 1) / DEC_R;
    if (ncg > 1) {
        const auto kern = ncg == 2   ? attn_decode_paged_wide_d128_kernel<DT, 2>
                          : ncg == 3 ? attn_decode_paged_wide_d128_kernel<DT, 3>
                                     : attn_decode_paged_wide_d128_kernel<DT, 4>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, a.st, q, a.q_sh, a.q_sl, k, v, a.kv_sh, row_bytes, p.acc, p.ml, a.Hq,
                           a.Hq / a.Hkv, a.Lq, a.Lk, a.off, c2, pl.keys_per_split, g.first, g.ve, list, g.keep_pages);
        RTK_LAUNCH_CHECK("attn_decode_paged_wide_d128_kernel");
        return attn_combine<DT>(p, a.out, a.Hq, a.Lq, 128, pl.nsplit, a.st);
    }
    if (arch8)
        hipLaunchKernelGGL((attn_decode_paged_fp8kv_d128_kernel<DT>), grid, dim3(256), 0, a.st, q, a.q_sh, a.q_sl, k, v, a.kv_sh,
                           row_bytes, rows_extent(a.Lk, a.kv_sl, 128, 2), p.acc, p.ml, a.Hq, a.Hq / a.Hkv, a.Lq, a.Lk, a.off, c2,
                           pl.keys_per_split, a8, list, g.keep_pages);
    else
        hipLaunchKernelGGL((attn_decode_paged_d128_kernel<DT>), grid, dim3(256), 0, a.st, q, a.q_sh, a.q_sl, k, v, a.kv_sh, row_bytes,
                           p.acc, p.ml, a.Hq, a.Hq / a.Hkv, a.Lq, a.Lk, a.off, c2, pl.keys_per_split, g.first, g.ve, list,
                           g.keep_pages);
    RTK_LAUNCH_CHECK(arch8 ? "attn_decode_paged_fp8kv_d128_kernel" : "attn_decode_paged_d128_kernel");
    return attn_combine<DT>(p, a.out, a.Hq, a.Lq, 128, pl.nsplit, a.st);
}

// A workspace query of the six: 0 with the error set for a shape the call's family does not take
size_t paged_query(const DecodeFamily& f, const char* query, bool arch8, bool sparse, int Hq, int Hkv, int Lq, int Lk, int L8, int first, int ve,
                   int keep_pages, int D, int dtype) {
    PagedGeom g;
    if (paged_check_shape(query, f, arch8, Hq, Hkv, Lq, Lk, L8, D, dtype, first, ve, keep_pages, g) != RTK_OK) return 0;
    return sparse_layout(sparse, Hkv, g, decode_plan(Hq, Hkv, Lq, g.keys)).bytes;
}

// An entry point of the six (`f`: its family; `query`: the one that sizes its workspace; `sg`: its archive, empty for the 16-bit kind;
// `pick`: its page list [Hkv, keep_pages] or, `sparse`, its summaries with head stride summ_sh): the checks in the order
// retake_hip.h states, then the paged kernel and the combine - after, `sparse`, the bound and the selection (one unit per
// kv head: the existing launchers as they are) have written the lists into the workspace.  As among the packed entry
// points, a call of the wide family with at most DEC_R packed rows is the narrow call of the same kind.
int paged_call(const DecodeFamily& f, const char* who, const char* query, bool arch8, bool sparse, const AttnArgs& a, const DecodeSegs& sg, int first, int ve,
               int keep_pages, const void* pick, int64_t summ_sh) {
    RTK_CHECK_ARG(a.q && a.k && a.v && a.out && pick, "%s: NULL q / k / v / out / %s pointer", who, sparse ? "summ" : "list");
    PagedGeom g;
    int rc = paged_check_shape(who, f, arch8, a.Hq, a.Hkv, a.Lq, a.Lk, sg.L8, a.D, a.dtype, first, ve, keep_pages, g);
    if (rc != RTK_OK) return rc;
    if (f.max_rows > DEC_R && (a.Hq / a.Hkv) * a.Lq <= DEC_R)
        return paged_call(DEC_NARROW, sparse ? "rtk_attention_decode_sparse" : "rtk_attention_decode_paged",
                          sparse ? "rtk_attention_decode_sparse_workspace_bytes" : "rtk_attention_decode_paged_workspace_bytes", arch8,
                          sparse, a, sg, first, ve, keep_pages, pick, summ_sh);
    if (sparse)
        RTK_CHECK_ARG(((uintptr_t)pick & 15) == 0 && (summ_sh * 2) % 16 == 0 && summ_sh >= (int64_t)g.pages * 2 * a.D,
                      "%s: summ must be 16-byte aligned with a head stride of at least pages * 2 * D = %lld elements", who,
                      (long long)g.pages * 2 * a.D);
    else
        RTK_CHECK_ARG(((uintptr_t)pick & 3) == 0, "%s: list must be 4-byte aligned", who);
    Archive8 a8{};
    rc = paged_check_operands(who, arch8, a, sg, g, a8);
    if (rc != RTK_OK) return rc;
    const DecodePlan pl = decode_plan(a.Hq, a.Hkv, a.Lq, g.keys);
    const SparseLayout sl = sparse_layout(sparse, a.Hkv, g, pl);
    rc = paged_check_workspace(who, query, sl.bytes, a.workspace, a.workspace_bytes);
    if (rc != RTK_OK) return rc;
    const int32_t* list = (const int32_t*)pick;
    if (sparse) {
        float* ub = (float*)a.workspace;
        int32_t* lists = (int32_t*)((char*)a.workspace + sl.lists_at);
        rc = rtk_attention_page_bound(a.q, a.q_sh, a.q_sl, pick, summ_sh, a.Hq, a.Hkv, a.Lq, g.pages, a.D, a.dtype, ub, (rtk_stream_t)a.st);
        if (rc != RTK_OK) return rc;
        std::vector<rtk_budget_select_unit> sel((size_t)a.Hkv);
        for (int h = 0; h < a.Hkv; ++h)
            sel[h] = rtk_budget_select_unit{ub + (size_t)h * g.pages, lists + (size_t)h * g.keep_pages, g.pages, g.keep_pages};
        rc = rtk_pivotkv_budget_select_batched(sel.data(), a.Hkv, (rtk_stream_t)a.st);
        if (rc != RTK_OK) return rc;
        list = lists;
    }
    void* partials = (char*)a.workspace + sl.partials_at;
    return a.dtype == RTK_BF16 ? paged_launch<RTK_BF16>(arch8, pl, a, a8, g, list, partials)
                               : paged_launch<RTK_F16>(arch8, pl, a, a8, g, list, partials);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" size_t rtk_attention_decode_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype) {
    return decode_query(DEC_NARROW, 0, Hq, Hkv, Lq, Lk, 0, 0, D, dtype);
}

extern "C" int rtk_attention_decode(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                    int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                    int q_offset, int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                    rtk_stream_t stream) {
    return decode_call(DEC_NARROW, 0,
                       AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                scale, workspace, workspace_bytes, (hipStream_t)stream},
                       DecodeSegs{});
}

extern "C" size_t rtk_attention_decode_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype) {
    return decode_query(DEC_NARROW, 1, Hq, Hkv, Lq, Lk, L8, 0, D, dtype);
}

extern "C" int rtk_attention_decode_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                          int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                          const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                          int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                          int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                          rtk_stream_t stream) {
    return decode_call(DEC_NARROW, 1,
                       AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                scale, workspace, workspace_bytes, (hipStream_t)stream},
                       DecodeSegs{nullptr, nullptr, 0, 0, 0, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h});
}

extern "C" size_t rtk_attention_decode_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype) {
    return decode_query(DEC_NARROW, 2, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype);
}

extern "C" int rtk_attention_decode_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                           int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                           int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                           const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                           int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                           int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                           rtk_stream_t stream) {
    return decode_call(DEC_NARROW, 2,
                       AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                scale, workspace, workspace_bytes, (hipStream_t)stream},
                       DecodeSegs{ks, vs, Ls, s_stride_h, s_stride_l, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h});
}

// ---- the wide family (16 < (Hq / Hkv) * Lq <= 64; at most 16 rows: the call above of the same segments) ----
extern "C" size_t rtk_attention_decode_wide_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype) {
    return decode_query(DEC_WIDE, 0, Hq, Hkv, Lq, Lk, 0, 0, D, dtype);
}

extern "C" int rtk_attention_decode_wide(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                    int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                    int q_offset, int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                    rtk_stream_t stream) {
    return decode_call(DEC_WIDE, 0,
                       AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                scale, workspace, workspace_bytes, (hipStream_t)stream},
                       DecodeSegs{});
}

extern "C" size_t rtk_attention_decode_wide_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype) {
    return decode_query(DEC_WIDE, 1, Hq, Hkv, Lq, Lk, L8, 0, D, dtype);
}

extern "C" int rtk_attention_decode_wide_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                          int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                          const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                          int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                          int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                          rtk_stream_t stream) {
    return decode_call(DEC_WIDE, 1,
                       AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                scale, workspace, workspace_bytes, (hipStream_t)stream},
                       DecodeSegs{nullptr, nullptr, 0, 0, 0, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h});
}

extern "C" size_t rtk_attention_decode_wide_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype) {
    return decode_query(DEC_WIDE, 2, Hq, Hkv, Lq, Lk, L8, Ls, D, dtype);
}

extern "C" int rtk_attention_decode_wide_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                           int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                           int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                           const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                           int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                           int D, int dtype, float scale, void* workspace, size_t workspace_bytes,
                                           rtk_stream_t stream) {
    return decode_call(DEC_WIDE, 2,
                       AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                                scale, workspace, workspace_bytes, (hipStream_t)stream},
                       DecodeSegs{ks, vs, Ls, s_stride_h, s_stride_l, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h});
}

extern "C" size_t rtk_attention_decode_group_workspace_bytes(const int* own_rows, int n_branches, int Hq, int Hkv, int L8,
                                                             int Ls, int D, int dtype) {
    const char* who = "rtk_attention_decode_group_workspace_bytes";
    if (!own_rows || n_branches < 1) {
        set_error("%s: NULL own_rows or n_branches %d < 1", who, n_branches);
        return 0;
    }
    if (Hq < 1 || Hkv < 1 || Hq % Hkv != 0 || group_check_envelope(who, n_branches, Hq, Hkv, D, dtype) != RTK_OK) return 0;
    for (int b = 0; b < n_branches; ++b)
        if (shared_check_shape(who, Hq, Hkv, 1, own_rows[b], L8, Ls, D, dtype, DEC_T) != RTK_OK) return 0;
    return group_plan(own_rows, n_branches, Hq, Hkv, L8, Ls).ws_bytes;
}

extern "C" int rtk_attention_decode_group(const rtk_decode_branch* branches, int n_branches, const void* ks, const void* vs,
                                          int Ls, int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                          const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                          int64_t scale_stride_h, void* out, int Hq, int Hkv, int D, int dtype, float scale,
                                          void* workspace, size_t workspace_bytes, rtk_stream_t stream) {
    const char* who = "rtk_attention_decode_group";
    RTK_CHECK_ARG(branches && out, "%s: NULL branches / out pointer", who);
    RTK_CHECK_ARG(n_branches >= 1, "%s: n_branches %d < 1", who, n_branches);
    RTK_CHECK_ARG(Hq >= 1 && Hkv >= 1, "%s: Hq and Hkv must be positive", who);
    RTK_CHECK_ARG(Hq % Hkv == 0, "%s: Hq %d is not a multiple of Hkv %d", who, Hq, Hkv);
    int rc = group_check_envelope(who, n_branches, Hq, Hkv, D, dtype);
    if (rc != RTK_OK) return rc;
    int own_rows[RTK_DECODE_GROUP_MAX];
    for (int b = 0; b < n_branches; ++b) {
        const rtk_decode_branch& br = branches[b];
        RTK_CHECK_ARG(br.q && br.k && br.v, "%s: NULL q / k / v pointer of branch %d", who, b);
        RTK_CHECK_ARG(br.Lk >= 1, "%s: branch %d has Lk %d (its own rows include the new token's: at least 1)", who, b, br.Lk);
        rc = shared_check_shape(who, Hq, Hkv, 1, br.Lk, L8, Ls, D, dtype, DEC_T);
        if (rc != RTK_OK) return rc;
        own_rows[b] = br.Lk;
    }
    Shared16 s16;
    rc = make_shared16(who, ks, vs, Ls, s_stride_h, s_stride_l, D, DEC_T, s16);
    if (rc != RTK_OK) return rc;
    Archive8 a8;
    rc = make_archive8(who, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h, a8);
    if (rc != RTK_OK) return rc;
    GroupArgs ga{};
    for (int b = 0; b < n_branches; ++b) {
        const rtk_decode_branch& br = branches[b];
        rc = attn_check_operands(who, br.q, br.q_stride_h, D, br.k, br.v, br.kv_stride_h, br.kv_stride_l, a8.k8, a8.v8, a8.ks,
                                 a8.vs, a8.sh8, a8.shs, out, 1, br.Lk, br.Lk - 1, D, dtype, scale, 0, DEC_T);
        if (rc != RTK_OK) return rc;
        ga.br[b] = GroupBranch{(const char*)br.q, (const char*)br.k, (const char*)br.v, br.q_stride_h, br.kv_stride_h,
                               (uint32_t)(br.kv_stride_l * 2), rows_extent(br.Lk, br.kv_stride_l, D, 2), br.Lk, 0};
    }
    const GroupPlan gp = group_plan(own_rows, n_branches, Hq, Hkv, L8, Ls);
    rc = attn_check_workspace(who, "rtk_attention_decode_group_workspace_bytes", gp.ws_bytes, workspace, workspace_bytes);
    if (rc != RTK_OK) return rc;
    ga.B = n_branches, ga.G = Hq / Hkv, ga.Hq = Hq, ga.ns_sh = gp.ns_sh, ga.kps_sh = gp.kps_sh, ga.max_own = gp.max_own;
    const float c2 = base2_scale(scale);
    if (dtype == RTK_BF16) return group_launch<RTK_BF16>(gp, ga, a8, s16, out, Hkv, c2, workspace, (hipStream_t)stream);
    return group_launch<RTK_F16>(gp, ga, a8, s16, out, Hkv, c2, workspace, (hipStream_t)stream);
}

// ---- page-sparse decode (retake_hip.h §U): paged_call with the call's names, kind and operands ----
extern "C" size_t rtk_attention_decode_paged_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages,
                                                             int D, int dtype) {
    return paged_query(DEC_NARROW, "rtk_attention_decode_paged_workspace_bytes", false, false, Hq, Hkv, Lq, Lk, 0, first, ve, keep_pages, D, dtype);
}

extern "C" int rtk_attention_decode_paged(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                          int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                          int q_offset, int D, int dtype, float scale, int first, int ve, const int32_t* list,
                                          int keep_pages, void* workspace, size_t workspace_bytes, rtk_stream_t stream) {
    return paged_call(DEC_NARROW, "rtk_attention_decode_paged", "rtk_attention_decode_paged_workspace_bytes", false, false,
                      AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                               scale, workspace, workspace_bytes, (hipStream_t)stream},
                      DecodeSegs{}, first, ve, keep_pages, list, 0);
}

extern "C" size_t rtk_attention_decode_sparse_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages,
                                                              int D, int dtype) {
    return paged_query(DEC_NARROW, "rtk_attention_decode_sparse_workspace_bytes", false, true, Hq, Hkv, Lq, Lk, 0, first, ve, keep_pages, D, dtype);
}

extern "C" int rtk_attention_decode_sparse(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                           int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                           int q_offset, int D, int dtype, float scale, int first, int ve, const void* summ,
                                           int64_t summ_stride_h, int keep_pages, void* workspace, size_t workspace_bytes,
                                           rtk_stream_t stream) {
    return paged_call(DEC_NARROW, "rtk_attention_decode_sparse", "rtk_attention_decode_sparse_workspace_bytes", false, true,
                      AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                               scale, workspace, workspace_bytes, (hipStream_t)stream},
                      DecodeSegs{}, first, ve, keep_pages, summ, summ_stride_h);
}

extern "C" size_t rtk_attention_decode_paged_fp8kv_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int L8, int keep_pages, int D,
                                                                   int dtype) {
    return paged_query(DEC_NARROW, "rtk_attention_decode_paged_fp8kv_workspace_bytes", true, false, Hq, Hkv, Lq, Lk, L8, 0, 0, keep_pages, D, dtype);
}

extern "C" int rtk_attention_decode_paged_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                                int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                                const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                                int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                                int D, int dtype, float scale, const int32_t* list, int keep_pages, void* workspace,
                                                size_t workspace_bytes, rtk_stream_t stream) {
    return paged_call(DEC_NARROW, "rtk_attention_decode_paged_fp8kv", "rtk_attention_decode_paged_fp8kv_workspace_bytes", true, false,
                      AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                               scale, workspace, workspace_bytes, (hipStream_t)stream},
                      DecodeSegs{nullptr, nullptr, 0, 0, 0, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h}, 0, 0,
                      keep_pages, list, 0);
}

extern "C" size_t rtk_attention_decode_sparse_fp8kv_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int L8, int keep_pages, int D,
                                                                    int dtype) {
    return paged_query(DEC_NARROW, "rtk_attention_decode_sparse_fp8kv_workspace_bytes", true, true, Hq, Hkv, Lq, Lk, L8, 0, 0, keep_pages, D, dtype);
}

extern "C" int rtk_attention_decode_sparse_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                                 int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                                 const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                                 int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                                 int D, int dtype, float scale, const void* summ, int64_t summ_stride_h,
                                                 int keep_pages, void* workspace, size_t workspace_bytes, rtk_stream_t stream) {
    return paged_call(DEC_NARROW, "rtk_attention_decode_sparse_fp8kv", "rtk_attention_decode_sparse_fp8kv_workspace_bytes", true, true,
                      AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                               scale, workspace, workspace_bytes, (hipStream_t)stream},
                      DecodeSegs{nullptr, nullptr, 0, 0, 0, k8, v8, k_scale, v_scale, L8, stride8_h, scale_stride_h}, 0, 0,
                      keep_pages, summ, summ_stride_h);
}

// ---- the wide family of the 16-bit page-sparse calls (16 < (Hq / Hkv) * Lq <= 64; at most 16 rows: the call above) ----
extern "C" size_t rtk_attention_decode_paged_wide_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages,
                                                                  int D, int dtype) {
    return paged_query(DEC_WIDE, "rtk_attention_decode_paged_wide_workspace_bytes", false, false, Hq, Hkv, Lq, Lk, 0, first, ve,
                       keep_pages, D, dtype);
}

extern "C" int rtk_attention_decode_paged_wide(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                               int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                               int q_offset, int D, int dtype, float scale, int first, int ve, const int32_t* list,
                                               int keep_pages, void* workspace, size_t workspace_bytes, rtk_stream_t stream) {
    return paged_call(DEC_WIDE, "rtk_attention_decode_paged_wide", "rtk_attention_decode_paged_wide_workspace_bytes", false, false,
                      AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                               scale, workspace, workspace_bytes, (hipStream_t)stream},
                      DecodeSegs{}, first, ve, keep_pages, list, 0);
}

extern "C" size_t rtk_attention_decode_sparse_wide_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages,
                                                                   int D, int dtype) {
    return paged_query(DEC_WIDE, "rtk_attention_decode_sparse_wide_workspace_bytes", false, true, Hq, Hkv, Lq, Lk, 0, first, ve,
                       keep_pages, D, dtype);
}

extern "C" int rtk_attention_decode_sparse_wide(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                                int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                                int q_offset, int D, int dtype, float scale, int first, int ve, const void* summ,
                                                int64_t summ_stride_h, int keep_pages, void* workspace, size_t workspace_bytes,
                                                rtk_stream_t stream) {
    return paged_call(DEC_WIDE, "rtk_attention_decode_sparse_wide", "rtk_attention_decode_sparse_wide_workspace_bytes", false, true,
                      AttnArgs{q, q_stride_h, q_stride_l, k, v, kv_stride_h, kv_stride_l, out, Hq, Hkv, Lq, Lk, q_offset, D, dtype,
                               scale, workspace, workspace_bytes, (hipStream_t)stream},
                      DecodeSegs{}, first, ve, keep_pages, summ, summ_stride_h);
}

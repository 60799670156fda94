// rebase_rotate.cuh - the pieces of the position re-base (pivotkv_rebase.hip: one delta per unit) that the per-row renumbering
// (pivotkv_renumber.hip: one delta per row) needs as well: the geometry of the apply launch, the rotation R(-delta) of one
// row's chunk pair over the heads, and the host's argument checks.  Both are rules of this project's own.
//
// pivotkv_renumber.hip is built on these; pivotkv_rebase.hip still carries its own text of the same code.  Written through
// these functions its three apply kernels compile to different code (other registers, a body a dozen dwords shorter:
// profiles/renumber_kernel_diff.txt), and an existing kernel is not changed on the side of a feature.  The arithmetic here is
// that file's, statement for statement: the kernel tests require the two entry points to agree bit for bit.
#pragma once
#include <algorithm>

#include "common.cuh"

namespace rtk {

constexpr int REBASE_BLOCK = 256;
constexpr int REBASE_WGS = 2048;   // workgroups of a full launch: 256 CUs x 8 resident workgroups of 4 waves
constexpr int REBASE_HB = 4;       // heads whose chunk pairs a thread requests together
constexpr uint32_t REBASE_HAS_PREV = 0x80000000u;   // bit 31 of a unit's slot word: first > 0 (t[-1] is the last pinned id)

// bit e: channel pair (d + e, d + e + D/2) follows id row 0
template <int VE>
__device__ __forceinline__ uint32_t rebase_temporal(const RowSel& rs, int d) {
    uint32_t temporal = 0;
#pragma unroll
    for (int e = 0; e < VE; ++e) temporal |= (rs.row[d + e] == 0 ? 1u : 0u) << e;
    return temporal;
}

// cos / sin of fl32(fd * inv_freq[d + e]); the identity where the pair is not temporal
template <int VE>
__device__ __forceinline__ void rebase_sincos(float fd, const float* __restrict__ inv_freq, int d, uint32_t temporal, float (&c)[VE],
                                              float (&s)[VE]) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        sincos_cr(fd * inv_freq[d + e], s[e], c[e]);
        if (!((temporal >> e) & 1u)) {
            c[e] = 1.f;
            s[e] = 0.f;
        }
    }
}

// which 32-bit words of a chunk take the rotated bits (a chunk that mixes id rows keeps the others' bits as they are)
template <int DT>
__device__ __forceinline__ void rebase_take(uint32_t temporal, uint32_t (&take)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if constexpr (DT != RTK_F32)
            take[w] = (((temporal >> (2 * w)) & 1u) ? 0x0000ffffu : 0u) | (((temporal >> (2 * w + 1)) & 1u) ? 0xffff0000u : 0u);
        else
            take[w] = ((temporal >> w) & 1u) ? 0xffffffffu : 0u;
    }
}

// one row: the chunk at row0 and its partner `half_bytes` further on, of H heads `stride_h` bytes apart, in batches of
// REBASE_HB heads - R(-delta) in fp32, one rounding to the storage dtype in pack()
template <int DT>
__device__ __forceinline__ void rebase_rotate_row(char* row0, int H, int64_t stride_h, int64_t half_bytes,
                                                  const float (&c)[Vec16<DT>::VE], const float (&s)[Vec16<DT>::VE],
                                                  const uint32_t (&take)[4]) {
    using V = Vec16<DT>;
    constexpr int VE = V::VE;
    for (int hb = 0; hb < H; hb += REBASE_HB) {
        u32x4 lo[REBASE_HB], hi[REBASE_HB];
#pragma unroll
        for (int u = 0; u < REBASE_HB; ++u) {   // (a short last batch repeats its last head: loaded, not stored)
            const char* p = row0 + (int64_t)min(hb + u, H - 1) * stride_h;
            lo[u] = *(const u32x4*)p;
            hi[u] = *(const u32x4*)(p + half_bytes);
        }
#pragma unroll
        for (int u = 0; u < REBASE_HB; ++u) {
            if (hb + u >= H) break;
            float x1[VE], x2[VE], o1[VE], o2[VE];
            V::unpack(lo[u], x1);
            V::unpack(hi[u], x2);
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                o1[e] = __builtin_fmaf(x1[e], c[e], __fmul_rn(x2[e], s[e]));
                o2[e] = __builtin_fmaf(x2[e], c[e], -__fmul_rn(x1[e], s[e]));
            }
            u32x4 nlo = V::pack(o1), nhi = V::pack(o2);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                nlo[w] = (nlo[w] & take[w]) | (lo[u][w] & ~take[w]);
                nhi[w] = (nhi[w] & take[w]) | (hi[u][w] & ~take[w]);
            }
            char* p = row0 + (int64_t)(hb + u) * stride_h;
            *(u32x4*)p = nlo;
            *(u32x4*)(p + half_bytes) = nhi;
        }
    }
}

// The host's checks of the shared arguments and of every unit's rtk_rebase_unit fields (Unit: rtk_rebase_unit or a struct
// that has its fields).  > 0: go on (es and ve are set); else what the entry point returns.
template <typename Unit>
inline int rebase_check(const Unit* units, int n_units, int D, int dtype, int P, const float* inv_freq, int64_t limit,
                        const int64_t* offsets, const int64_t* delta, int& es, int& ve, const char* who) {
    int rc = have_units(units, n_units, who);
    if (rc <= 0) return rc;
    RTK_CHECK_ARG(inv_freq && offsets && delta, "%s: NULL pointer (inv_freq / offsets / delta)", who);
    RTK_CHECK_ARG(limit >= 0, "%s: negative limit %lld", who, (long long)limit);
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "%s: unsupported dtype %d", who, dtype);
    RTK_CHECK_ARG(D >= 2, "%s: head_dim %d", who, D);
    RTK_CHECK_ARG(P == 1 || P == 3, "%s: P must be 1 or 3, got %d", who, P);
    for (int i = 0; i < n_units; ++i) {
        const Unit& u = units[i];
        RTK_CHECK_ARG(u.k && u.ids, "%s: unit %d: NULL pointer", who, i);
        RTK_CHECK_ARG(u.H >= 1 && u.first >= 0 && u.rows >= 0 && u.end >= 0 && u.k_stride_h >= 0 && u.ids_stride >= 0 && u.slot >= 0,
                      "%s: unit %d: negative H / first / rows / end / stride / slot", who, i);
        RTK_CHECK_ARG(u.first <= u.end, "%s: unit %d: first %lld > end %lld", who, i, (long long)u.first, (long long)u.end);
        RTK_CHECK_ARG(u.first <= (INT64_MAX >> 12) - u.rows, "%s: unit %d: first + rows overflows a byte offset", who, i);
        RTK_CHECK_ARG(u.H == 1 || u.k_stride_h >= (u.first + u.rows) * (int64_t)D * es,
                      "%s: unit %d: the rows [0, %lld) of a head reach into the next head", who, i, (long long)(u.first + u.rows));
        RTK_CHECK_ARG(P == 1 || u.ids_stride >= u.end, "%s: unit %d: ids_stride %lld < end %lld", who, i, (long long)u.ids_stride,
                      (long long)u.end);
        for (int j = 0; j < i; ++j)
            RTK_CHECK_ARG(units[j].slot != u.slot, "%s: units %d and %d share offset slot %d", who, j, i, u.slot);
    }
    return 1;
}

// ... and the conditions under which the apply kernels' 16-byte accesses do not serve: RTK_EUNSUPPORTED
template <typename Unit>
inline int rebase_supported(const Unit* units, int n_units, int D, int P, const int* sections_host, int nsec, int ve, RowSel& rs,
                            const char* who) {
    bool aligned = D % (2 * ve) == 0 && D <= 256;
    for (int i = 0; i < n_units; ++i)
        aligned = aligned && ((uintptr_t)units[i].k & 15) == 0 && units[i].k_stride_h % 16 == 0 && ((uintptr_t)units[i].ids & 7) == 0;
    if (!aligned) {
        set_error("%s: needs 16-byte aligned rows and head strides and head_dim a multiple of %d (<= 256)", who, 2 * ve);
        return RTK_EUNSUPPORTED;
    }
    int rc;
    if ((rc = make_rowsel(rs, P, D, sections_host, nsec, who)) != RTK_OK) return rc;
    for (int d = 0; d < D / 2; ++d)
        if ((rs.row[d] == 0) != (rs.row[d + D / 2] == 0)) {
            set_error("%s: channel %d and its rotation partner follow different id rows", who, d);
            return RTK_EUNSUPPORTED;
        }
    return RTK_OK;
}

}  // namespace rtk

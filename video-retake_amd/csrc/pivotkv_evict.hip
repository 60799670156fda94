// pivotkv_evict.hip — PivotKV row movement on gfx950: append, batched eviction, place and commit.
// Replaces longvideo_cache.py:238 (the torch.cat of DynamicCache.update) and :278-318 (the three gathers, the forward
// re-rotation of the kept K rows and the two torch.cat cache rebuilds).  Which rows survive is decided in
// pivotkv_select.hip; the one-launch in-place form of the eviction is pivotkv_compact.hip.
//
// Roofline: HBM-bound byte shuffling with 16-byte coalesced accesses - algorithmic bytes per (layer, chunk):
// 2*Hkv*L*D*s read + written by the append (which the reference pays as an O(cache) torch.cat), 2*Hkv*keep*D*s read +
// written for the kept 1/ratio of the rows.
#include <algorithm>

#include "common.cuh"

namespace rtk {


// ------------------------------------------------------------------------------------------------
// Chunk-batched cache maintenance.  `PivotKVCache.update` only has to hand the layer's attention the
// uncompressed [prefix | chunk] view (longvideo_cache.py:238) and to decide which rows survive; the
// gather / re-rotation / compaction of ALL layers of a chunk is flushed in two launches from
// `after_forward` (the hook the reference calls after every video chunk, qwen2_vl.py:715-716):
//   append_kernel          per update: K and V rows of the chunk -> cache tail (pure streaming copy)
//   evict_batched_kernel   per flush : every pending (layer, chunk) unit in one launch (blockIdx.y = unit)
//   commit_batched_kernel  per flush : staged rows -> head of the tail, every unit in one launch
// A single unit is 6.5 MB of traffic (a 10 us launch is ramp-dominated); 28 layers per launch keep every
// CU streaming.
// ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void append_kernel(const char* __restrict__ k, int64_t k_sh, int64_t k_sl,
                                                     const char* __restrict__ v, int64_t v_sh, int64_t v_sl, int Hkv,
                                                     int L, int D, char* __restrict__ k_tail,
                                                     char* __restrict__ v_tail, int64_t tail_sh) {
    constexpr int VE = Vec16<DT>::VE;
    constexpr int ES = 16 / VE;
    constexpr int U = 4;                // 16-byte chunks per thread per tensor, all loads before the stores
    const int cpr = D / VE;             // 16-byte chunks per row
    const size_t total = (size_t)Hkv * L * cpr;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; id < total; id += U * stride) {
        u32x4 kk[U], vv[U];
        size_t dst[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = id + u * stride;
            const size_t ic = i < total ? i : id;
            const int c = (int)(ic % cpr);
            const size_t hl = ic / cpr;
            const int l = (int)(hl % L), h = (int)(hl / L);
            kk[u] = *(const u32x4*)(k + ((size_t)h * k_sh + (size_t)l * k_sl + (size_t)c * VE) * ES);
            vv[u] = *(const u32x4*)(v + ((size_t)h * v_sh + (size_t)l * v_sl + (size_t)c * VE) * ES);
            dst[u] = ((size_t)h * tail_sh + (size_t)l * D + (size_t)c * VE) * ES;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (id + u * stride < total) {
                *(u32x4*)(k_tail + dst[u]) = kk[u];
                *(u32x4*)(v_tail + dst[u]) = vv[u];
            }
        }
    }
}

struct EvictUnits {
    rtk_evict_unit u[RTK_EVICT_MAX_UNITS];
};

// One thread owns, for ONE kept row r of a unit, the 16-byte chunk c of the first half of the row and its
// rotation partner in the second half, and walks the KV heads with it: the row's cos/sin (reforge) are
// loaded once and reused by every head, and all of a head group's loads are issued before its stores.
// NATIVE: the cos/sin of the kept rows' NEW ids are computed here (rope_table_kernel's arithmetic on pos_src, 8 or 16
// sincos_cr per thread, reused by all KV heads) instead of being read from fp32 tables another launch wrote:
// one launch and 2 x keep x D x 4 bytes of write + read per unit less.
template <int DT, int HU, bool NATIVE>
__global__ __launch_bounds__(256) void evict_batched_kernel(EvictUnits units, int Hkv, int D, int keep, int P,
                                                            const float* __restrict__ inv_freq, float scaling,
                                                            RowSel rs, int round_bf16, int low_only) {
    constexpr int VE = Vec16<DT>::VE;
    constexpr int ES = 16 / VE;
    const rtk_evict_unit& un = units.u[blockIdx.y];
    const int h2 = D / 2;
    const int lpr = h2 / VE;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    // position ids of the kept tokens -> the layer's position cache (longvideo_cache.py:308-309)
    if (un.pos_dst && id < P * keep) {
        const int p = id / keep, r = id - p * keep;
        un.pos_dst[(size_t)p * un.pos_dst_stride + r] = un.pos_src[(size_t)p * un.pos_src_stride + r];
    }
    const int r = id / lpr;
    if (r >= keep) return;
    const int d = (id - r * lpr) * VE;
    const int l = (int)un.keep_idx[r];
    const char* ks = (const char*)un.k_src;
    const char* vs = (const char*)un.v_src;
    char* kd = (char*)un.k_dst;
    char* vd = (char*)un.v_dst;
    // a NULL destination skips the tensor: keep-all chunks leave V (and an unchanged K) where the append put them
    const bool reforge = (NATIVE || un.cos_new != nullptr) && kd != nullptr;
    // low_only: rows copied verbatim (V; K without reforge) are staged only when their source lies inside the
    // destination range [0, keep) of the tail they will overwrite; the others are moved in place by place_batched_kernel
    const bool stage_row = !(low_only & 1) || l < keep;
    // low_only bit 1: K comes from a buffer of its own (the un-rotated copy of a deferred re-rotation), not from the
    // tail it is written to: every kept K row is copied
    const bool copy_k = kd != nullptr && !reforge && (stage_row || (low_only & 2)), copy_rows = vd != nullptr && stage_row;
    u32x4 k_lo[HU], k_hi[HU], v_lo[HU], v_hi[HU];
    auto load_batch = [&](int hb) {
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int h = min(hb + u, Hkv - 1);
            const char* kr = ks + ((size_t)h * un.k_src_stride_h + (size_t)l * D) * ES;
            const char* vr = vs + ((size_t)h * un.v_src_stride_h + (size_t)l * D) * ES;
            if (reforge || copy_k) {
                k_lo[u] = *(const u32x4*)(kr + (size_t)d * ES);
                k_hi[u] = *(const u32x4*)(kr + (size_t)(d + h2) * ES);
            }
            if (copy_rows) {
                v_lo[u] = *(const u32x4*)(vr + (size_t)d * ES);
                v_hi[u] = *(const u32x4*)(vr + (size_t)(d + h2) * ES);
            }
        }
    };
    if (!reforge && !copy_k && !copy_rows) return;
    load_batch(0);   // the rows are requested before the table arithmetic / table reads below
    float c1[VE], s1[VE], c2[VE], s2[VE];
    if (NATIVE && reforge) {
        float pid[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) pid[p] = (float)un.pos_src[(size_t)min(p, P - 1) * un.pos_src_stride + r];
        rope_chunk<VE>(inv_freq, rs, d, h2, pid, scaling, round_bf16, c1, s1, c2, s2);
    } else if (reforge) {
        const float* cr = un.cos_new + (size_t)r * D;
        const float* sr = un.sin_new + (size_t)r * D;
#pragma unroll
        for (int e = 0; e < VE; e += 4) {
            *(float4*)(c1 + e) = *(const float4*)(cr + d + e);
            *(float4*)(s1 + e) = *(const float4*)(sr + d + e);
            *(float4*)(c2 + e) = *(const float4*)(cr + d + h2 + e);
            *(float4*)(s2 + e) = *(const float4*)(sr + d + h2 + e);
        }
    }
    for (int hb = 0; hb < Hkv; hb += HU) {
        if (hb > 0) load_batch(hb);
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const int h = hb + u;
            if (h >= Hkv) break;
            char* ko = kd + ((size_t)h * un.k_dst_stride_h + (size_t)r * D) * ES;
            char* vo = vd + ((size_t)h * un.v_dst_stride_h + (size_t)r * D) * ES;
            if (reforge) {  // kept K = un-rotated row rotated forward at its new position (:297-306)
                // (the 16-bit roundings through the packed converts: the integer sequence made this kernel VALU-bound)
                u32x4 olo, ohi;
                rotate_chunk_pair<DT>(k_lo[u], k_hi[u], c1, s1, c2, s2, olo, ohi);
                *(u32x4*)(ko + (size_t)d * ES) = olo;
                *(u32x4*)(ko + (size_t)(d + h2) * ES) = ohi;
            } else if (copy_k) {   // torch.gather(key_states, 2, keep)  (:279)
                *(u32x4*)(ko + (size_t)d * ES) = k_lo[u];
                *(u32x4*)(ko + (size_t)(d + h2) * ES) = k_hi[u];
            }
            if (copy_rows) {
                *(u32x4*)(vo + (size_t)d * ES) = v_lo[u];  // torch.gather(value_states, 2, keep)  (:280)
                *(u32x4*)(vo + (size_t)(d + h2) * ES) = v_hi[u];
            }
        }
    }
}

struct CopyUnits {
    rtk_copy_unit u[RTK_COPY_MAX_UNITS];
};

// dst[h][0:rows] = src[h][0:rows] for every unit (blockIdx.y); each head's row block is contiguous
__global__ __launch_bounds__(256) void commit_batched_kernel(CopyUnits units, int H, size_t row_block_bytes) {
    const rtk_copy_unit& un = units.u[blockIdx.y];
    const char* src = (const char*)un.src;
    char* dst = (char*)un.dst;
    const size_t vec_per_head = row_block_bytes / 16;
    const size_t total = (size_t)H * vec_per_head;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    constexpr int U = 4;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += U * stride) {
        u32x4 t[U];
        size_t o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = id + u * stride;
            const size_t ic = i < total ? i : id;
            const size_t h = ic / vec_per_head, j = ic % vec_per_head;
            t[u] = *(const u32x4*)(src + h * un.src_stride_h_bytes + j * 16);
            o[u] = h * un.dst_stride_h_bytes + j * 16;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (id + u * stride < total) *(u32x4*)(dst + o[u]) = t[u];
    }
}

struct PlaceUnits {
    rtk_place_unit u[RTK_PLACE_MAX_UNITS];
};

// P13 (longvideo_cache.py:313-318) without a full staging copy: kept row r of a unit goes to tail[h][r].  Its source
// is the chunk row keep_idx[r] of the same tail; rows whose source lies below `keep` would race with the rows being
// written there, so an earlier launch (evict_batched_kernel, low_only) parked exactly those in `stage`; every other
// row is read where it sits - beyond the destination range, which nothing writes.  ~ratio of the rows take the hop.
__global__ __launch_bounds__(256) void place_batched_kernel(PlaceUnits units, int H, int keep, int vec_per_row) {
    const rtk_place_unit& un = units.u[blockIdx.y];
    const size_t total = (size_t)H * keep * vec_per_row;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    constexpr int U = 4;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += U * stride) {
        u32x4 t[U];
        size_t o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = id + u * stride;
            const size_t ic = i < total ? i : id;
            const int j = (int)(ic % vec_per_row);
            const size_t hr = ic / vec_per_row;
            const int r = (int)(hr % keep), h = (int)(hr / keep);
            const int64_t l = un.keep_idx[r];
            const char* src = l < keep ? (const char*)un.stage + ((size_t)h * un.stage_stride_h_bytes + (size_t)r * vec_per_row * 16)
                                       : (const char*)un.tail + ((size_t)h * un.tail_stride_h_bytes + (size_t)l * vec_per_row * 16);
            t[u] = *(const u32x4*)(src + (size_t)j * 16);
            o[u] = (size_t)h * un.tail_stride_h_bytes + ((size_t)r * vec_per_row + j) * 16;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (id + u * stride < total) *(u32x4*)((char*)un.tail + o[u]) = t[u];
    }
}

}  // namespace rtk

using namespace rtk;

extern "C" int rtk_pivotkv_append(const void* k, int64_t k_stride_h, int64_t k_stride_l, const void* v,
                                  int64_t v_stride_h, int64_t v_stride_l, int Hkv, int L, int D, int dtype,
                                  void* k_tail, void* v_tail, int64_t tail_stride_h, rtk_stream_t stream) {
    RTK_CHECK_ARG(k && v && k_tail && v_tail, "rtk_pivotkv_append: NULL pointer");
    RTK_CHECK_ARG(Hkv >= 1 && L >= 1 && D >= 1, "rtk_pivotkv_append: bad shape");
    int es, ve;
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "rtk_pivotkv_append: unsupported dtype %d", dtype);
    const bool aligned = D % ve == 0 && (k_stride_h * es) % 16 == 0 && (k_stride_l * es) % 16 == 0 &&
                         (v_stride_h * es) % 16 == 0 && (v_stride_l * es) % 16 == 0 && (tail_stride_h * es) % 16 == 0 &&
                         (((uintptr_t)k | (uintptr_t)v | (uintptr_t)k_tail | (uintptr_t)v_tail) & 15) == 0;
    if (!aligned) {
        set_error("rtk_pivotkv_append: pointers, strides and head_dim rows must be 16-byte aligned");
        return RTK_EUNSUPPORTED;
    }
    const size_t chunks = (size_t)Hkv * L * (D / ve);
    const unsigned grid = (unsigned)std::min<size_t>((chunks + 4 * 256 - 1) / (4 * 256), 4096);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != RTK_F32)   // a pure copy: the 2-byte instantiation serves both 16-bit formats
        RTK_LAUNCH(KID_APPEND, append_kernel<RTK_BF16>, dim3(grid), dim3(256), 0, st, (const char*)k, k_stride_h,
                   k_stride_l, (const char*)v, v_stride_h, v_stride_l, Hkv, L, D, (char*)k_tail, (char*)v_tail,
                   tail_stride_h);
    else
        RTK_LAUNCH(KID_APPEND, append_kernel<RTK_F32>, dim3(grid), dim3(256), 0, st, (const char*)k, k_stride_h,
                   k_stride_l, (const char*)v, v_stride_h, v_stride_l, Hkv, L, D, (char*)k_tail, (char*)v_tail,
                   tail_stride_h);
    RTK_LAUNCH_CHECK("append_kernel");
    return RTK_OK;
}

static int evict_batched_impl(const rtk_evict_unit* units, int n_units, int Hkv, int D, int keep, int P, int dtype,
                              const float* inv_freq, float scaling, const RowSel* rsel, int round_bf16, int low_only,
                              rtk_stream_t stream) {
    const bool native = inv_freq != nullptr;
    RowSel rs;
    if (rsel) rs = *rsel;
    else for (int d = 0; d < 256; ++d) rs.row[d] = 0;
    RTK_CHECK_ARG(units && n_units >= 1, "rtk_pivotkv_evict_batched: no units");
    RTK_CHECK_ARG(Hkv >= 1 && keep >= 1 && D >= 2, "rtk_pivotkv_evict_batched: bad shape");
    int es, ve;
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "rtk_pivotkv_evict_batched: unsupported dtype %d", dtype);
    RTK_CHECK_ARG(P == 0 || P == 1 || P == 3, "rtk_pivotkv_evict_batched: P must be 0, 1 or 3, got %d", P);
    if (D % (2 * ve) != 0) {
        set_error("rtk_pivotkv_evict_batched: head_dim %d must be a multiple of %d for this dtype", D, 2 * ve);
        return RTK_EUNSUPPORTED;
    }
    for (int i = 0; i < n_units; ++i) {
        const rtk_evict_unit& u = units[i];
        RTK_CHECK_ARG(u.k_src && u.v_src && u.keep_idx, "rtk_pivotkv_evict_batched: unit %d: NULL pointer", i);
        RTK_CHECK_ARG((u.cos_new == nullptr) == (u.sin_new == nullptr), "rtk_pivotkv_evict_batched: unit %d: cos_new and sin_new go together", i);
        RTK_CHECK_ARG((u.pos_dst == nullptr) || (u.pos_src != nullptr && P > 0), "rtk_pivotkv_evict_batched: unit %d: pos_dst needs pos_src and P", i);
        RTK_CHECK_ARG(!native || (u.pos_src != nullptr && P > 0 && u.cos_new == nullptr),
                      "rtk_pivotkv_evict_batched_rope: unit %d: needs pos_src (the new ids), P > 0 and no tables", i);
        const bool aligned = (u.k_src_stride_h * es) % 16 == 0 && (u.v_src_stride_h * es) % 16 == 0 &&
                             (u.k_dst_stride_h * es) % 16 == 0 && (u.v_dst_stride_h * es) % 16 == 0 &&
                             (((uintptr_t)u.k_src | (uintptr_t)u.v_src | (uintptr_t)u.k_dst | (uintptr_t)u.v_dst |
                               (uintptr_t)u.cos_new | (uintptr_t)u.sin_new) & 15) == 0;
        if (!aligned) {
            set_error("rtk_pivotkv_evict_batched: unit %d: pointers and strides must be 16-byte aligned", i);
            return RTK_EUNSUPPORTED;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int threads = std::max(keep * (D / 2 / ve), P * keep);
    const unsigned gx = (unsigned)((threads + 255) / 256);
    for (int b = 0; b < n_units; b += RTK_EVICT_MAX_UNITS) {
        const int n = std::min(RTK_EVICT_MAX_UNITS, n_units - b);
        const EvictUnits eu = pad_units<EvictUnits>(units + b, n);
#define RTK_EVB_NAT(DTV, HUV, NAT)                                                                                   \
    RTK_LAUNCH(KID_EVICTB, (evict_batched_kernel<DTV, HUV, NAT>), dim3(gx, n), dim3(256), 0, st, eu, Hkv, D, keep, P, \
               inv_freq, scaling, rs, round_bf16, low_only)
#define RTK_EVB(DTV, HUV)                         \
    do {                                          \
        if (native) RTK_EVB_NAT(DTV, HUV, true);  \
        else RTK_EVB_NAT(DTV, HUV, false);        \
    } while (0)
        if (dtype == RTK_BF16) RTK_EVB(RTK_BF16, 4);
        else if (dtype == RTK_F16) RTK_EVB(RTK_F16, 4);
        else RTK_EVB(RTK_F32, 2);
#undef RTK_EVB
#undef RTK_EVB_NAT
        RTK_LAUNCH_CHECK("evict_batched_kernel");
    }
    return RTK_OK;
}

extern "C" int rtk_pivotkv_evict_batched(const rtk_evict_unit* units, int n_units, int Hkv, int D, int keep, int P,
                                         int dtype, int stage_low_only, rtk_stream_t stream) {
    return evict_batched_impl(units, n_units, Hkv, D, keep, P, dtype, nullptr, 0.f, nullptr, 0, stage_low_only, stream);
}

extern "C" int rtk_pivotkv_evict_batched_rope(const rtk_evict_unit* units, int n_units, int Hkv, int D, int keep, int P,
                                              int dtype, const float* inv_freq, float attention_scaling,
                                              const int* sections_host, int nsec, int round_bf16, int stage_low_only,
                                              rtk_stream_t stream) {
    RTK_CHECK_ARG(inv_freq, "rtk_pivotkv_evict_batched_rope: inv_freq is NULL");
    RTK_CHECK_ARG(P == 1 || P == 3, "rtk_pivotkv_evict_batched_rope: P must be 1 or 3, got %d", P);
    RowSel rs;
    const int rc = make_rowsel(rs, P, D, sections_host, nsec, "rtk_pivotkv_evict_batched_rope");
    if (rc != RTK_OK) return rc;
    return evict_batched_impl(units, n_units, Hkv, D, keep, P, dtype, inv_freq, attention_scaling, &rs, round_bf16,
                              stage_low_only, stream);
}

extern "C" int rtk_pivotkv_place_batched(const rtk_place_unit* units, int n_units, int H, int keep, int D, int dtype,
                                         rtk_stream_t stream) {
    RTK_CHECK_ARG(units && n_units >= 1, "rtk_pivotkv_place_batched: no units");
    RTK_CHECK_ARG(H >= 1 && keep >= 1 && D >= 1, "rtk_pivotkv_place_batched: bad shape");
    int es, ve;
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "rtk_pivotkv_place_batched: unsupported dtype %d", dtype);
    const size_t row = (size_t)D * es;
    for (int i = 0; i < n_units; ++i) {
        const rtk_place_unit& u = units[i];
        RTK_CHECK_ARG(u.stage && u.tail && u.keep_idx, "rtk_pivotkv_place_batched: unit %d: NULL pointer", i);
        if (row % 16 || u.stage_stride_h_bytes % 16 || u.tail_stride_h_bytes % 16 || (((uintptr_t)u.stage | (uintptr_t)u.tail) & 15)) {
            set_error("rtk_pivotkv_place_batched: unit %d: rows must be 16-byte aligned", i);
            return RTK_EUNSUPPORTED;
        }
    }
    const size_t total = (size_t)H * keep * (row / 16);
    const unsigned gx = (unsigned)std::min<size_t>((total + 4 * 256 - 1) / (4 * 256), 1024);
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_units; b += RTK_PLACE_MAX_UNITS) {
        const int n = std::min(RTK_PLACE_MAX_UNITS, n_units - b);
        RTK_LAUNCH(KID_COMMITB, place_batched_kernel, dim3(gx, n), dim3(256), 0, st, pad_units<PlaceUnits>(units + b, n), H,
                   keep, (int)(row / 16));
        RTK_LAUNCH_CHECK("place_batched_kernel");
    }
    return RTK_OK;
}

extern "C" int rtk_pivotkv_commit_batched(const rtk_copy_unit* units, int n_units, int H, int rows, int D, int dtype,
                                          rtk_stream_t stream) {
    RTK_CHECK_ARG(units && n_units >= 1, "rtk_pivotkv_commit_batched: no units");
    RTK_CHECK_ARG(H >= 1 && rows >= 0 && D >= 1, "rtk_pivotkv_commit_batched: bad shape");
    int es, ve;
    RTK_CHECK_ARG(payload_dims(dtype, es, ve), "rtk_pivotkv_commit_batched: unsupported dtype %d", dtype);
    if (rows == 0) return RTK_OK;
    const size_t blk = (size_t)rows * D * es;
    for (int i = 0; i < n_units; ++i) {
        const rtk_copy_unit& u = units[i];
        RTK_CHECK_ARG(u.src && u.dst, "rtk_pivotkv_commit_batched: unit %d: NULL pointer", i);
        if (blk % 16 || u.src_stride_h_bytes % 16 || u.dst_stride_h_bytes % 16 || (((uintptr_t)u.src | (uintptr_t)u.dst) & 15)) {
            set_error("rtk_pivotkv_commit_batched: unit %d: blocks must be 16-byte aligned", i);
            return RTK_EUNSUPPORTED;
        }
    }
    const size_t total = (size_t)H * (blk / 16);
    const unsigned gx = (unsigned)std::min<size_t>((total + 4 * 256 - 1) / (4 * 256), 1024);
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_units; b += RTK_COPY_MAX_UNITS) {
        const int n = std::min(RTK_COPY_MAX_UNITS, n_units - b);
        RTK_LAUNCH(KID_COMMITB, commit_batched_kernel, dim3(gx, n), dim3(256), 0, st, pad_units<CopyUnits>(units + b, n), H,
                   blk);
        RTK_LAUNCH_CHECK("commit_batched_kernel");
    }
    return RTK_OK;
}
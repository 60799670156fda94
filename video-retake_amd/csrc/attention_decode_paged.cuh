// attention_decode_paged.cuh - the packed decode kernel with its MIDDLE segment read through a page list (retake_hip.h §U
// "Page-sparse decode", rtk_attention_decode_paged / rtk_attention_decode_sparse).  Included by attention_decode.hip after
// the narrow kernels, whose constants and helpers (DEC_*, mma32, wave_lds_sync, dec_step_off, dec_v_frag, dec_softmax_step)
// it uses; the tile loads and the four-wave fold are written out here as in attention_decode_d128_body.inc, which stays
// untouched (as shared functions they would compile the existing kernels differently - DESIGN.md).
//
// The keys of one kv head are ONE buffer k [Lk rows]; the kernel walks a VIRTUAL key space of whole 32-key tiles
//     [ rows [0, first), padded to firstp = 32 ceil(first / 32) | page list[0], list[1], .. list[keep_pages - 1] | rows [ve, Lk) ]
// where page p is rows first + [32 p, min(32 p + 32, n)), n = ve - first.  Everything that depends on a tile's place - the
// split it belongs to, the wave that takes it, the order of the fold - is decided in the virtual space, exactly as the
// packed kernel decides it in its physical one, so with first % 32 == 0 and n % 32 == 0 the call IS rtk_attention_decode
// over the concatenation of those rows, bit for bit.
//   * Each segment has a buffer descriptor of its own over exactly its rows - [0, first), [first, ve), [ve, Lk) - so the rows
//     a padded head tile or the partial last page would name beyond its segment READ AS ZERO (K and V alike), whatever the
//     memory there holds, and their logits are set to -inf as the packed kernel does for keys >= Lk.
//   * A list entry is read once per tile as a wave-uniform number and clamped into [0, pages - 1]: a bad list names a wrong
//     page, never a byte outside rows [first, ve).
//   * Only the tail has a diagonal; the launcher admits q_offset >= ve - 1 only, so every packed row sees the head and
//     the pages whole.
// No atomics, no flags, no waiting between workgroups; plain vector stores.

template <int DT>
__global__ __launch_bounds__(256, 2) void attn_decode_paged_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq, int G, int Lq,
    int Lk, int off, float c2, int keys_per_split, int first, int ve, const int32_t* __restrict__ list, int keep_pages) {
    __shared__ __attribute__((aligned(16))) char lds[4 * DEC_WAVE_LDS];   // [wave]: V tile, then the wave's O
    __shared__ float ml_s[4][DEC_R][2];
    // the virtual key space: head tiles [0, firstp) | listed pages [firstp, tv) | tail rows [tv, Lkv)
    const int n = ve - first, pages = (n + DEC_T - 1) / DEC_T;
    const int firstp = (first + DEC_T - 1) / DEC_T * DEC_T, tv = firstp + keep_pages * DEC_T;
    const int Lkv = tv + (Lk - ve), offv = off - ve + tv;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // packed row (column) and lane group
    const int split = blockIdx.x, hkv = blockIdx.y, R = G * Lq;
    const int qi = c % Lq, qg = c / Lq;       // query position and head-in-group of packed row c
    const int k_lo = split * keys_per_split;
    const int k_hi = min(min(Lkv, offv + Lq), k_lo + keys_per_split);   // exclusive: first key no row of the range sees
    const int vis_r = min(offv + qi, Lkv - 1);                          // last (virtual) key packed row c sees
    const int32_t* __restrict__ my_list = list + (int64_t)hkv * keep_pages;

    // a descriptor per segment over exactly its rows (built per tile from these wave-uniform numbers): a row past its
    // segment's last reads as zero
    const char* kh = k + (int64_t)hkv * kv_sh * 2;
    const char* vh = v + (int64_t)hkv * kv_sh * 2;
    const uint32_t head_bytes = first > 0 ? (uint32_t)(first - 1) * kv_row_bytes + 256u : 0u;
    const uint32_t reg_bytes = n > 0 ? (uint32_t)(n - 1) * kv_row_bytes + 256u : 0u;
    const uint32_t tail_bytes = Lk > ve ? (uint32_t)(Lk - ve - 1) * kv_row_bytes + 256u : 0u;
    const int64_t reg_at = (int64_t)first * kv_row_bytes, tail_at = (int64_t)ve * kv_row_bytes;

    // Q fragments (B operand): packed row c, zero for c >= R
    u32x4 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = u32x4{0u, 0u, 0u, 0u};
    if (c < R) {
        const char* qr = q + ((int64_t)(hkv * G + qg) * q_sh + (int64_t)qi * q_sl) * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const u32x4*)(qr + dec_step_off(s, g));
    }

    // Where a virtual tile lies (all wave-uniform): its segment's byte offset in the head and byte extent, its first row
    // within the segment, whether it is a tail tile, and - head and pages - the last key of the tile that exists.  `locate`
    // describes the tile whose loads are issued next; `process` takes its copy before it locates the following one.
    int64_t t_at = 0;
    uint32_t t_bytes = 0;
    int t_row0 = 0, t_last = 0;
    bool t_tail = false;
    auto locate = [&](int kb) {
        if (kb < firstp) {
            t_at = 0, t_bytes = head_bytes, t_row0 = kb, t_last = first - 1 - kb, t_tail = false;
        } else if (kb < tv) {
            const int e = uniform_int(my_list[(kb - firstp) / DEC_T]);
            const int p = min(max(e, 0), pages - 1);   // inside the region whatever the list says
            t_at = reg_at, t_bytes = reg_bytes, t_row0 = DEC_T * p, t_last = min(DEC_T, n - DEC_T * p) - 1, t_tail = false;
        } else {
            t_at = tail_at, t_bytes = tail_bytes, t_row0 = kb - tv, t_last = 0, t_tail = true;
        }
    };

    // One tile's operands, in flight from the moment the previous tile's are consumed: kr[4 b + s] = the step-s chunk of key
    // row 16 b + c; vr[u] = chunk c of V row 4 u + g
    u32x4 kr[8], vr[8];
    auto load_k = [&]() {
        const __amdgpu_buffer_rsrc_t r = bounded_rsrc(kh + t_at, t_bytes);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kr[4 * b + s] = load16(r, (uint32_t)(t_row0 + 16 * b + c) * kv_row_bytes + (uint32_t)dec_step_off(s, g));
    };
    auto load_v = [&]() {
        const __amdgpu_buffer_rsrc_t r = bounded_rsrc(vh + t_at, t_bytes);
#pragma unroll
        for (int u = 0; u < 8; ++u) vr[u] = load16(r, (uint32_t)(t_row0 + 4 * u + g) * kv_row_bytes + 16u * c);
    };

    char* vt = lds + wave * DEC_WAVE_LDS;
    // transposed V reads, as attention_decode_d128_body.inc lays them out
    const int v_rd = DEC_VPITCH * (4 * g + (c >> 2)) + 8 * (c & 3);

    f32x4 oacc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // tile kb (located, its loads in flight); `next`: this wave has a tile at kb + DEC_STEP
    auto process = [&](int kb, bool next) {
        const bool tail = t_tail;
        const int last = t_last;
        u32x4 ka[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) ka[e] = kr[e];
#pragma unroll
        for (int u = 0; u < 8; ++u) *(u32x4*)(vt + DEC_VPITCH * (4 * u + g) + 16 * c) = vr[u];
        if (next) {
            locate(kb + DEC_STEP);
            load_v();
        }
        wave_lds_sync();
        // logits: s0[e] = key 4 g + e, s1[e] = key 16 + 4 g + e of the tile, packed row c
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            s0 = mma32<DT>(ka[s], qf[s], s0);
            s1 = mma32<DT>(ka[4 + s], qf[s], s1);
        }
        if (next) load_k();
        // the last key of the tile this row sees: its diagonal or the end of the keys in the tail, else the last row of
        // the head / of the page, which every row sees
        const int lim = tail ? vis_r - kb : last;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * g + e > lim) s0[e] = -INFINITY;
            if (16 + 4 * g + e > lim) s1[e] = -INFINITY;
        }
        const u32x4 pf = dec_softmax_step<DT>(s0, s1, c2, m, l, oacc);
        if (!tail || kb + DEC_T - 1 <= offv) {   // every row sees every key of the tile that exists (the others read as zero)
#pragma unroll
            for (int db = 0; db < 8; ++db) oacc[db] = mma32<DT>(dec_v_frag(vt + v_rd, db), pf, oacc[db]);
        } else {
            // one pass per query position: V rows above its diagonal zeroed, the lanes of its packed rows keep the result
            for (int i = 0; i < Lq; ++i) {
                const int li = min(offv + i, Lkv - 1) - kb;
                u32x4 keep;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int key = 16 * (w >> 1) + 4 * g + 2 * (w & 1);
                    keep[w] = (key <= li ? 0xffffu : 0u) | (key + 1 <= li ? 0xffff0000u : 0u);
                }
#pragma unroll
                for (int db = 0; db < 8; ++db) {
                    const f32x4 t = mma32<DT>(dec_v_frag(vt + v_rd, db) & keep, pf, oacc[db]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) oacc[db][e] = qi == i ? t[e] : oacc[db][e];
                }
            }
        }
        wave_lds_sync();   // the reads above before the next tile's writes
    };

    // this wave's tiles: u = wave, wave + 4, ... of the range
    const int kb0 = k_lo + DEC_T * wave;
    if (kb0 < k_hi) {
        locate(kb0);
        load_k();
        load_v();
    }
    for (int kb = kb0; kb < k_hi; kb += DEC_STEP) process(kb, kb + DEC_STEP < k_hi);

    // fold the four waves in wave order; the workgroup leaves one partial per packed row
    l += __shfl_xor(l, 16, WAVE);
    l += __shfl_xor(l, 32, WAVE);
    {
        float* ow = (float*)vt;
#pragma unroll
        for (int db = 0; db < 8; ++db) *(f32x4*)(ow + c * DEC_OPITCH + 16 * db + 4 * g) = oacc[db];
        if (g == 0) {
            ml_s[wave][c][0] = m;
            ml_s[wave][c][1] = l;
        }
    }
    __syncthreads();
    const int row = tid >> 4, ch = tid & 15;   // packed row, channels 8 ch .. 8 ch + 7
    if (row >= R) return;
    float mg = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mg = fmaxf(mg, ml_s[w][row][0]);
    f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float mw = ml_s[w][row][0];
        if (mw == -INFINITY) continue;   // the wave had no key this row sees
        const float wt = __builtin_amdgcn_exp2f(mw - mg);
        const float* ow = (const float*)(lds + w * DEC_WAVE_LDS) + row * DEC_OPITCH + 8 * ch;
        const f32x4 a = *(const f32x4*)ow, b = *(const f32x4*)(ow + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            n0[e] = __builtin_fmaf(wt, a[e], n0[e]);
            n1[e] = __builtin_fmaf(wt, b[e], n1[e]);
        }
        den = __builtin_fmaf(wt, ml_s[w][row][1], den);
    }
    const size_t prow = ((size_t)split * Hq + (size_t)(hkv * G + row / Lq)) * Lq + row % Lq;
    float* pa = part_acc + prow * 128 + 8 * ch;
    *(f32x4*)pa = n0;
    *(f32x4*)(pa + 4) = n1;
    if (ch == 0) *(float2*)(part_ml + 2 * prow) = make_float2(mg, den);
}

// attn_decode_paged_fp8kv_d128_kernel - the same walk with the e4m3 ARCHIVE as the paged segment (rtk_attention_decode_paged_fp8kv /
// rtk_attention_decode_sparse_fp8kv).  The virtual key space is
//     [ archive page list[0], list[1], .. list[keep_pages - 1] | 16-bit rows [0, Lk) ]
// where page p is archive rows [32 p, min(32 p + 32, L8)).  A page tile takes the FP8 branch of attention_decode_d128_body.inc:
// codes and scales global -> registers, fp8_dequant16 into the K operand and the V image a 16-bit tile of the dequantised
// rows would have left; with the identity list the call IS rtk_attention_decode_fp8kv over the archive as it lies, bit for bit.
//   * The archive's descriptors are bounded at exactly L8 * 128 and L8 * 4 bytes: the rows the partial last page names
//     beyond L8 read as zero codes and zero scales, and their logits are set to -inf.
//   * A list entry is read once per tile as a wave-uniform number and clamped into [0, pages - 1].
//   * Only the 16-bit rows have a diagonal; `off` counts 16-bit rows (>= Lk - Lq), every packed row sees every archive row.
// No atomics, no flags, no waiting between workgroups; plain vector stores.
template <int DT>
__global__ __launch_bounds__(256, 2) void attn_decode_paged_fp8kv_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq,
    int G, int Lq, int Lk, int off, float c2, int keys_per_split, Archive8 a8, const int32_t* __restrict__ list, int keep_pages) {
    __shared__ __attribute__((aligned(16))) char lds[4 * DEC_WAVE_LDS];   // [wave]: V tile, then the wave's O
    __shared__ float ml_s[4][DEC_R][2];
    // the virtual key space: listed archive pages [0, tv) | 16-bit rows [tv, Lkv)
    const int L8 = a8.L8, pages = (L8 + DEC_T - 1) / DEC_T;
    const int tv = keep_pages * DEC_T;
    const int Lkv = tv + Lk, offv = off + tv;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // packed row (column) and lane group
    const int split = blockIdx.x, hkv = blockIdx.y, R = G * Lq;
    const int qi = c % Lq, qg = c / Lq;       // query position and head-in-group of packed row c
    const int k_lo = split * keys_per_split;
    const int k_hi = min(min(Lkv, offv + Lq), k_lo + keys_per_split);   // exclusive: first key no row of the range sees
    const int vis_r = min(offv + qi, Lkv - 1);                          // last (virtual) key packed row c sees
    const int32_t* __restrict__ my_list = list + (int64_t)hkv * keep_pages;

    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(k + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(v + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rk8 = bounded_rsrc(a8.k8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
    const __amdgpu_buffer_rsrc_t rv8 = bounded_rsrc(a8.v8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
    const __amdgpu_buffer_rsrc_t rks = bounded_rsrc(a8.ks + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
    const __amdgpu_buffer_rsrc_t rvs = bounded_rsrc(a8.vs + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);

    // Q fragments (B operand): packed row c, zero for c >= R
    u32x4 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = u32x4{0u, 0u, 0u, 0u};
    if (c < R) {
        const char* qr = q + ((int64_t)(hkv * G + qg) * q_sh + (int64_t)qi * q_sl) * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const u32x4*)(qr + dec_step_off(s, g));
    }

    // Where a virtual tile lies (all wave-uniform): whether it is an archive page, its first row within its segment and - a
    // page - the last key of the tile that exists.  `locate` describes the tile whose loads are issued next; `process`
    // takes its copy before it locates the following one.
    int t_row0 = 0, t_last = 0;
    bool t_arch = false;
    auto locate = [&](int kb) {
        if (kb < tv) {
            const int e = uniform_int(my_list[kb / DEC_T]);
            const int p = min(max(e, 0), pages - 1);   // inside the archive whatever the list says
            t_row0 = DEC_T * p, t_last = min(DEC_T, L8 - DEC_T * p) - 1, t_arch = true;
        } else {
            t_row0 = kb - tv, t_last = 0, t_arch = false;
        }
    };

    // One tile's operands, laid out as in attention_decode_d128_body.inc.  16-bit tile: kr[4 b + s] = the step-s chunk of key
    // row 16 b + c; vr[u] = chunk c of V row 4 u + g.  Archive tile: kr[2 b + a] = codes 16 (4 a + g) .. + 15 of key row
    // 16 b + c, its scale in kr[4][b]; vr[u] = codes 16 (lane & 7) .. + 15 of V row 8 u + (lane >> 3), its scale in vr[4][u].
    u32x4 kr[8], vr[8];
    auto load_k = [&]() {
        if (t_arch) {   // rows >= L8 of the partial page: zero codes, zero scales
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const uint32_t row = (uint32_t)(t_row0 + 16 * b + c);
#pragma unroll
                for (int a = 0; a < 2; ++a) kr[2 * b + a] = load16(rk8, row * 128u + 16u * (4 * a + g));
                kr[4][b] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rks, row * 4u, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kr[4 * b + s] = load16(rk, (uint32_t)(t_row0 + 16 * b + c) * kv_row_bytes + (uint32_t)dec_step_off(s, g));
    };
    auto load_v = [&]() {
        if (t_arch) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t row = (uint32_t)(t_row0 + 8 * u + (lane >> 3));
                vr[u] = load16(rv8, row * 128u + 16u * (lane & 7));
                vr[4][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rvs, row * 4u, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) vr[u] = load16(rv, (uint32_t)(t_row0 + 4 * u + g) * kv_row_bytes + 16u * c);
    };

    char* vt = lds + wave * DEC_WAVE_LDS;
    // transposed V reads, as attention_decode_d128_body.inc lays them out
    const int v_rd = DEC_VPITCH * (4 * g + (c >> 2)) + 8 * (c & 3);

    f32x4 oacc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // tile kb (located, its loads in flight); `next`: this wave has a tile at kb + DEC_STEP
    auto process = [&](int kb, bool next) {
        const bool arch = t_arch;
        const int last = t_last;
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
        if (next) {
            locate(kb + DEC_STEP);
            load_v();
        }
        wave_lds_sync();
        // logits: s0[e] = key 4 g + e, s1[e] = key 16 + 4 g + e of the tile, packed row c
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            s0 = mma32<DT>(ka[s], qf[s], s0);
            s1 = mma32<DT>(ka[4 + s], qf[s], s1);
        }
        if (next) load_k();
        // the last key of the tile this row sees: the last row of the page, which every row sees, else its diagonal or the
        // end of the 16-bit rows
        const int lim = arch ? last : vis_r - kb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * g + e > lim) s0[e] = -INFINITY;
            if (16 + 4 * g + e > lim) s1[e] = -INFINITY;
        }
        const u32x4 pf = dec_softmax_step<DT>(s0, s1, c2, m, l, oacc);
        if (arch || kb + DEC_T - 1 <= offv) {   // every row sees every key of the tile that exists (the others read as zero)
#pragma unroll
            for (int db = 0; db < 8; ++db) oacc[db] = mma32<DT>(dec_v_frag(vt + v_rd, db), pf, oacc[db]);
        } else {
            // one pass per query position: V rows above its diagonal zeroed, the lanes of its packed rows keep the result
            for (int i = 0; i < Lq; ++i) {
                const int li = min(offv + i, Lkv - 1) - kb;
                u32x4 keep;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int key = 16 * (w >> 1) + 4 * g + 2 * (w & 1);
                    keep[w] = (key <= li ? 0xffffu : 0u) | (key + 1 <= li ? 0xffff0000u : 0u);
                }
#pragma unroll
                for (int db = 0; db < 8; ++db) {
                    const f32x4 t = mma32<DT>(dec_v_frag(vt + v_rd, db) & keep, pf, oacc[db]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) oacc[db][e] = qi == i ? t[e] : oacc[db][e];
                }
            }
        }
        wave_lds_sync();   // the reads above before the next tile's writes
    };

    // this wave's tiles: u = wave, wave + 4, ... of the range
    const int kb0 = k_lo + DEC_T * wave;
    if (kb0 < k_hi) {
        locate(kb0);
        load_k();
        load_v();
    }
    for (int kb = kb0; kb < k_hi; kb += DEC_STEP) process(kb, kb + DEC_STEP < k_hi);

    // fold the four waves in wave order; the workgroup leaves one partial per packed row
    l += __shfl_xor(l, 16, WAVE);
    l += __shfl_xor(l, 32, WAVE);
    {
        float* ow = (float*)vt;
#pragma unroll
        for (int db = 0; db < 8; ++db) *(f32x4*)(ow + c * DEC_OPITCH + 16 * db + 4 * g) = oacc[db];
        if (g == 0) {
            ml_s[wave][c][0] = m;
            ml_s[wave][c][1] = l;
        }
    }
    __syncthreads();
    const int row = tid >> 4, ch = tid & 15;   // packed row, channels 8 ch .. 8 ch + 7
    if (row >= R) return;
    float mg = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mg = fmaxf(mg, ml_s[w][row][0]);
    f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float mw = ml_s[w][row][0];
        if (mw == -INFINITY) continue;   // the wave had no key this row sees
        const float wt = __builtin_amdgcn_exp2f(mw - mg);
        const float* ow = (const float*)(lds + w * DEC_WAVE_LDS) + row * DEC_OPITCH + 8 * ch;
        const f32x4 a = *(const f32x4*)ow, b = *(const f32x4*)(ow + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            n0[e] = __builtin_fmaf(wt, a[e], n0[e]);
            n1[e] = __builtin_fmaf(wt, b[e], n1[e]);
        }
        den = __builtin_fmaf(wt, ml_s[w][row][1], den);
    }
    const size_t prow = ((size_t)split * Hq + (size_t)(hkv * G + row / Lq)) * Lq + row % Lq;
    float* pa = part_acc + prow * 128 + 8 * ch;
    *(f32x4*)pa = n0;
    *(f32x4*)(pa + 4) = n1;
    if (ch == 0) *(float2*)(part_ml + 2 * prow) = make_float2(mg, den);
}

// attn_decode_paged_wide_d128_kernel - the 16-bit walk above for 16 < R = G * Lq <= 64 packed rows (rtk_attention_decode_paged_wide /
// rtk_attention_decode_sparse_wide): the body of attn_decode_wide_d128_kernel (FP8 = false, SHARED = false; attention_decode_wide.cuh,
// included before this file, whose WIDE_* constants it uses) over the virtual key space of
// attn_decode_paged_d128_kernel,
//     [ rows [0, first), padded to firstp = 32 ceil(first / 32) | page list[0], list[1], .. list[keep_pages - 1] | rows [ve, Lk) ]
// Packed row r = i * G + g (position-major), the Q image staged once in LDS, (m, l, oacc) per column group, a tile on the
// diagonal judged per group (hidden, whole, or one pass per position), the four waves folded one group at a time in wave
// order - all as the wide kernel has them; `locate`, the descriptor per segment over exactly its rows (a row past its
// segment's last reads as zero, its logit is -inf), the list entry read once per tile as a wave-uniform number and clamped
// into [0, pages - 1] - all as the paged kernel has them.  ALL Lq positions of the call share the kv head's one list.
// Only the tail has a diagonal (the launcher admits q_offset >= ve - 1 only): a head or page tile is the wide kernel's
// `seg` case, seen whole up to the tile's last existing row t_last.  Split, wave and fold order are decided in the virtual
// space, so with first % 32 == 0 and n % 32 == 0 the call IS rtk_attention_decode_wide over the concatenation of those
// rows, bit for bit.  No atomics, no flags, no waiting between workgroups; plain vector stores.
// Compiled for one workgroup per CU at every NCG: beside the wide kernel's registers the walk keeps the located tile's
// numbers, and at wide_occupancy(2, false) = 2 the NCG = 2 variant spills one VGPR to scratch (8 bytes per lane); at 1 no
// variant has scratch (profiles/sparse_decode_wide_kernel_resources.txt).  A sparse call's grid is about one workgroup
// per CU in any case.
template <int DT, int NCG>
__global__ __launch_bounds__(256, 1) void attn_decode_paged_wide_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq, int G, int Lq,
    int Lk, int off, float c2, int keys_per_split, int first, int ve, const int32_t* __restrict__ list, int keep_pages) {
    static_assert(NCG >= 2 && NCG * DEC_R <= WIDE_R, "two to four column groups");
    constexpr int NR = NCG * DEC_R;
    __shared__ __attribute__((aligned(16))) char lds[4 * DEC_WAVE_LDS];   // [wave]: V tile, then the wave's O of one group
    __shared__ __attribute__((aligned(16))) char q_s[NR * WIDE_QPITCH];
    __shared__ float ml_s[4][DEC_R][2];
    // the virtual key space: head tiles [0, firstp) | listed pages [firstp, tv) | tail rows [tv, Lkv)
    const int n = ve - first, pages = (n + DEC_T - 1) / DEC_T;
    const int firstp = (first + DEC_T - 1) / DEC_T * DEC_T, tv = firstp + keep_pages * DEC_T;
    const int Lkv = tv + (Lk - ve), offv = off - ve + tv;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // column within a group and lane group
    const int split = blockIdx.x, hkv = blockIdx.y, R = G * Lq;
    const int k_lo = split * keys_per_split;
    const int k_hi = min(min(Lkv, offv + Lq), k_lo + keys_per_split);   // exclusive: first key no row of the range sees
    const int32_t* __restrict__ my_list = list + (int64_t)hkv * keep_pages;

    // a descriptor per segment over exactly its rows (built per tile from these wave-uniform numbers): a row past its
    // segment's last reads as zero
    const char* kh = k + (int64_t)hkv * kv_sh * 2;
    const char* vh = v + (int64_t)hkv * kv_sh * 2;
    const uint32_t head_bytes = first > 0 ? (uint32_t)(first - 1) * kv_row_bytes + 256u : 0u;
    const uint32_t reg_bytes = n > 0 ? (uint32_t)(n - 1) * kv_row_bytes + 256u : 0u;
    const uint32_t tail_bytes = Lk > ve ? (uint32_t)(Lk - ve - 1) * kv_row_bytes + 256u : 0u;
    const int64_t reg_at = (int64_t)first * kv_row_bytes, tail_at = (int64_t)ve * kv_row_bytes;

    // the Q image: packed row r = i * G + g at r * WIDE_QPITCH, zero for r >= R; thread t stages 64 bytes of row t >> 2
    {
        const int r = tid >> 2, part = 64 * (tid & 3);
        if (r < NR) {
            u32x4 x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = u32x4{0u, 0u, 0u, 0u};
            if (r < R) {
                const char* qr = q + ((int64_t)(hkv * G + r % G) * q_sh + (int64_t)(r / G) * q_sl) * 2 + part;
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = *(const u32x4*)(qr + 16 * e);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) *(u32x4*)(q_s + r * WIDE_QPITCH + part + 16 * e) = x[e];
        }
    }
    __syncthreads();
    // the B operand of S^T = mfma(K, Q) for column group cg, k-step s
    auto q_frag = [&](int cg, int s) { return *(const u32x4*)(q_s + (16 * cg + c) * WIDE_QPITCH + dec_step_off(s, g)); };
    int qi[NCG];   // the query position of the lane's packed row in each group (past Lq - 1 for an idle column)
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) qi[cg] = (16 * cg + c) / G;

    // Where a virtual tile lies (all wave-uniform), as in attn_decode_paged_d128_kernel: `locate` describes the tile whose
    // loads are issued next; `process` takes its copy before it locates the following one.
    int64_t t_at = 0;
    uint32_t t_bytes = 0;
    int t_row0 = 0, t_last = 0;
    bool t_tail = false;
    auto locate = [&](int kb) {
        if (kb < firstp) {
            t_at = 0, t_bytes = head_bytes, t_row0 = kb, t_last = first - 1 - kb, t_tail = false;
        } else if (kb < tv) {
            const int e = uniform_int(my_list[(kb - firstp) / DEC_T]);
            const int p = min(max(e, 0), pages - 1);   // inside the region whatever the list says
            t_at = reg_at, t_bytes = reg_bytes, t_row0 = DEC_T * p, t_last = min(DEC_T, n - DEC_T * p) - 1, t_tail = false;
        } else {
            t_at = tail_at, t_bytes = tail_bytes, t_row0 = kb - tv, t_last = 0, t_tail = true;
        }
    };

    // one tile's operands, laid out as in attention_decode_d128_body.inc
    u32x4 kr[8], vr[8];
    auto load_k = [&]() {
        const __amdgpu_buffer_rsrc_t r = bounded_rsrc(kh + t_at, t_bytes);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kr[4 * b + s] = load16(r, (uint32_t)(t_row0 + 16 * b + c) * kv_row_bytes + (uint32_t)dec_step_off(s, g));
    };
    auto load_v = [&]() {
        const __amdgpu_buffer_rsrc_t r = bounded_rsrc(vh + t_at, t_bytes);
#pragma unroll
        for (int u = 0; u < 8; ++u) vr[u] = load16(r, (uint32_t)(t_row0 + 4 * u + g) * kv_row_bytes + 16u * c);
    };

    char* vt = lds + wave * DEC_WAVE_LDS;
    const int v_rd = DEC_VPITCH * (4 * g + (c >> 2)) + 8 * (c & 3);   // the transposed read of the narrow body

    f32x4 oacc[NCG][8];
    float m[NCG], l[NCG];
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
#pragma unroll
        for (int db = 0; db < 8; ++db) oacc[cg][db] = f32x4{0.f, 0.f, 0.f, 0.f};
        m[cg] = -INFINITY;
        l[cg] = 0.f;
    }

    // tile kb (located, its loads in flight); `next`: this wave has a tile at kb + DEC_STEP
    auto process = [&](int kb, bool next) {
        const bool seg = !t_tail;   // a head or page tile: every row sees it whole, up to its last existing row
        const int seg_vis = t_last;
        u32x4 ka[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) ka[e] = kr[e];
#pragma unroll
        for (int u = 0; u < 8; ++u) *(u32x4*)(vt + DEC_VPITCH * (4 * u + g) + 16 * c) = vr[u];
        if (next) {
            locate(kb + DEC_STEP);
            load_v();
        }
        wave_lds_sync();
        // one column group at a time: its logits (s0[e] = key 4 g + e, s1[e] = key 16 + 4 g + e of the tile), its softmax
        // step; the next tile's K loads go out once the last group's products have consumed the fragments
        u32x4 pf[NCG];
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const u32x4 qb = q_frag(cg, s);
                s0 = mma32<DT>(ka[s], qb, s0);
                s1 = mma32<DT>(ka[4 + s], qb, s1);
            }
            if (cg == NCG - 1 && next) load_k();
            // the last key of the tile this row sees: the last row of the head / of the page, which every row sees, else
            // its diagonal or the end of the keys in the tail
            const int lim = seg ? seg_vis : min(offv + qi[cg], Lkv - 1) - kb;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (4 * g + e > lim) s0[e] = -INFINITY;
                if (16 + 4 * g + e > lim) s1[e] = -INFINITY;
            }
            pf[cg] = dec_softmax_step<DT>(s0, s1, c2, m[cg], l[cg], oacc[cg]);
        }
        if (seg || kb + DEC_T - 1 <= offv) {   // every row sees every key of the tile that exists (the others read as zero)
#pragma unroll
            for (int db = 0; db < 8; ++db) {   // one transposed read of the V image feeds every column group
                const u32x4 vf = dec_v_frag(vt + v_rd, db);
#pragma unroll
                for (int cg = 0; cg < NCG; ++cg) oacc[cg][db] = mma32<DT>(vf, pf[cg], oacc[cg][db]);
            }
        } else {
#pragma unroll
            for (int cg = 0; cg < NCG; ++cg) {
                const int i_lo = 16 * cg / G, i_hi = (min(16 * cg + 15, R - 1)) / G;   // the positions of the group's rows
                if (kb > min(offv + i_hi, Lkv - 1)) continue;   // hidden from every row of the group: its probabilities are 0
                if (kb + DEC_T - 1 <= offv + i_lo) {            // every row of the group sees the tile whole
#pragma unroll
                    for (int db = 0; db < 8; ++db) oacc[cg][db] = mma32<DT>(dec_v_frag(vt + v_rd, db), pf[cg], oacc[cg][db]);
                    continue;
                }
                // one pass per position: V rows above its diagonal zeroed, the lanes of its packed rows keep the result
                for (int i = i_lo; i <= i_hi; ++i) {
                    const int li = min(offv + i, Lkv - 1) - kb;
                    u32x4 keep;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int key = 16 * (w >> 1) + 4 * g + 2 * (w & 1);
                        keep[w] = (key <= li ? 0xffffu : 0u) | (key + 1 <= li ? 0xffff0000u : 0u);
                    }
#pragma unroll
                    for (int db = 0; db < 8; ++db) {
                        const f32x4 t = mma32<DT>(dec_v_frag(vt + v_rd, db) & keep, pf[cg], oacc[cg][db]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) oacc[cg][db][e] = qi[cg] == i ? t[e] : oacc[cg][db][e];
                    }
                }
            }
        }
        wave_lds_sync();   // the reads above before the next tile's writes
    };

    // this wave's tiles: u = wave, wave + 4, ... of the range
    const int kb0 = k_lo + DEC_T * wave;
    if (kb0 < k_hi) {
        locate(kb0);
        load_k();
        load_v();
    }
    for (int kb = kb0; kb < k_hi; kb += DEC_STEP) process(kb, kb + DEC_STEP < k_hi);

    // fold the four waves in wave order, one column group at a time through the waves' 16-row O images; the workgroup
    // leaves one partial per packed row
    const int ch = tid & 15;   // channels 8 ch .. 8 ch + 7
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
        float lc = l[cg];
        lc += __shfl_xor(lc, 16, WAVE);
        lc += __shfl_xor(lc, 32, WAVE);
        {
            float* ow = (float*)vt;
#pragma unroll
            for (int db = 0; db < 8; ++db) *(f32x4*)(ow + c * DEC_OPITCH + 16 * db + 4 * g) = oacc[cg][db];
            if (g == 0) {
                ml_s[wave][c][0] = m[cg];
                ml_s[wave][c][1] = lc;
            }
        }
        __syncthreads();
        const int col = tid >> 4, row = 16 * cg + col;   // packed row
        if (row < R) {
            float mg = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) mg = fmaxf(mg, ml_s[w][col][0]);
            f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = {0.f, 0.f, 0.f, 0.f};
            float den = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float mw = ml_s[w][col][0];
                if (mw == -INFINITY) continue;   // the wave had no key this row sees
                const float wt = __builtin_amdgcn_exp2f(mw - mg);
                const float* ow = (const float*)(lds + w * DEC_WAVE_LDS) + col * DEC_OPITCH + 8 * ch;
                const f32x4 a = *(const f32x4*)ow, b = *(const f32x4*)(ow + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    n0[e] = __builtin_fmaf(wt, a[e], n0[e]);
                    n1[e] = __builtin_fmaf(wt, b[e], n1[e]);
                }
                den = __builtin_fmaf(wt, ml_s[w][col][1], den);
            }
            const size_t prow = ((size_t)split * Hq + (size_t)(hkv * G + row % G)) * Lq + row / G;
            float* pa = part_acc + prow * 128 + 8 * ch;
            *(f32x4*)pa = n0;
            *(f32x4*)(pa + 4) = n1;
            if (ch == 0) *(float2*)(part_ml + 2 * prow) = make_float2(mg, den);
        }
        if (cg + 1 < NCG) __syncthreads();   // the reads above before the next group's images
    }
}

// attention_decode_wide.cuh - attn_decode_wide_d128_kernel: the GQA-packed kernel of attention_decode.hip (which includes
// this file after its shared device functions) for 16 < R = G * Lq <= 64 packed rows (rtk_attention_decode_wide*): the
// verification step of assisted generation, a few-token continuation.  The tile loop is that of
// attention_decode_d128_body.inc - grid nsplit x Hkv, four waves, 32-key tiles round robin, K global -> registers as the A
// operand of S^T = mfma(K, Q), V global -> registers -> a wave-private LDS image read back transposed, no workgroup
// barrier in the key loop - and, as in the group kernel, a tile's K fragments and V image feed NCG = ceil(R / 16) column
// groups, each with its own (m, l, oacc): a K or V row is fetched from HBM once per call.  What differs:
//   * packed row r = i * G + g (position-major): row r is position i = r / G of query head hkv * G + r % G.  A column
//     group then holds ceil(16 / G) + 1 positions at most, and a tile on the diagonal costs one PV pass per position of the
//     group, not one per packed row (the workspace layout is by (head, i), so the order is the kernel's to choose);
//   * the Q rows are staged once in LDS ([NCG * 16][WIDE_QPITCH]) and the B operands of S^T read from there, one column
//     group at a time, so the kernel itself pins no Q fragment to a register beside the NCG * 32 accumulators;
//   * causal by index per packed row.  A tile every row sees whole (the archive, the shared rows, keys <= off) takes the
//     group kernel's PV loop.  Any other tile is judged per column group: hidden from all its rows - skipped, its V rows
//     are not read; seen whole by all its rows - one PV pass; else one pass per position of the group with the V rows
//     above that position's diagonal zeroed, each lane keeping the pass of its own row.  A hidden V row reaches no row
//     that does not see it, whatever it holds; with Lq > 32 the diagonal spans several tiles, of several waves, and each
//     is judged alone;
//   * the four waves are folded one column group at a time through the 16-row O image a wave already has (two workgroup
//     barriers per group, after the key loop), in wave order 0, 1, 2, 3 with the arithmetic of the narrow body.
// Partials in the layout attn_combine_kernel reads; no atomics, no flags, plain vector stores.
#pragma once

constexpr int WIDE_R = 64;         // packed rows the wide kernel serves at most: four column groups
constexpr int WIDE_QPITCH = 272;   // bytes per packed row of the Q image: 256 + 16, so 16 rows' chunks spread over the banks

// Workgroups per CU the kernel is compiled for.  Beside the NCG * 32 accumulators the compiler keeps about 160 registers
// busy with the tile in flight (the narrow kernel: 207 to 214 in all), so only the 16-bit NCG = 2 variant fits the 256 of
// occupancy 2 without scratch; the others take occupancy 1, where what exceeds 256 VGPRs sits in AGPRs
// (profiles/wide_decode_kernel_resources.txt).  The LDS (54 784 bytes at NCG = 4) would allow 2 either way.
constexpr int wide_occupancy(int ncg, bool fp8) { return ncg == 2 && !fp8 ? 2 : 1; }

template <int DT, int NCG, bool FP8, bool SHARED>
__global__ __launch_bounds__(256, wide_occupancy(NCG, FP8)) void attn_decode_wide_d128_kernel(
    const char* __restrict__ q, int64_t q_sh, int64_t q_sl, const char* __restrict__ k, const char* __restrict__ v,
    int64_t kv_sh, uint32_t kv_row_bytes, uint32_t kv_bytes, float* __restrict__ part_acc, float* __restrict__ part_ml, int Hq,
    int G, int Lq, int Lk, int off, float c2, int keys_per_split, Archive8 a8, Shared16 s16) {
    static_assert(NCG >= 2 && NCG * DEC_R <= WIDE_R, "two to four column groups");
    static_assert(FP8 || !SHARED, "the shared variant takes an archive too (it may be empty)");
    constexpr int NR = NCG * DEC_R;
    __shared__ __attribute__((aligned(16))) char lds[4 * DEC_WAVE_LDS];   // [wave]: V tile, then the wave's O of one group
    __shared__ __attribute__((aligned(16))) char q_s[NR * WIDE_QPITCH];
    __shared__ float ml_s[4][DEC_R][2];
    // from here on Lk and off count in the padded key space [archive L8p | shared Lsp | own rows]
    const int L8 = FP8 ? a8.L8 : 0, L8p = (L8 + DEC_T - 1) / DEC_T * DEC_T;
    const int Ls = SHARED ? s16.Ls : 0, Lsp = (Ls + DEC_T - 1) / DEC_T * DEC_T;
    Lk += L8p + Lsp;
    off += L8p + Lsp;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // column within a group and lane group
    const int split = blockIdx.x, hkv = blockIdx.y, R = G * Lq;
    const int k_lo = split * keys_per_split;
    const int k_hi = min(min(Lk, off + Lq), k_lo + keys_per_split);   // exclusive: first key no row of the range sees

    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(k + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(v + (int64_t)hkv * kv_sh * 2, kv_bytes);
    __amdgpu_buffer_rsrc_t rk8 = rk, rv8 = rk, rks = rk, rvs = rk, rsk = rk, rsv = rk;
    if constexpr (FP8) {
        rk8 = bounded_rsrc(a8.k8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rv8 = bounded_rsrc(a8.v8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rks = bounded_rsrc(a8.ks + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
        rvs = bounded_rsrc(a8.vs + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
    }
    if constexpr (SHARED) {
        rsk = bounded_rsrc(s16.k + (int64_t)hkv * s16.sh * 2, s16.bytes);
        rsv = bounded_rsrc(s16.v + (int64_t)hkv * s16.sh * 2, s16.bytes);
    }

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

    // one tile's operands, laid out as in attention_decode_d128_body.inc
    u32x4 kr[8], vr[8];
    auto load_k = [&](int kb) {
        if constexpr (FP8) {
            if (kb < L8p) {   // rows >= L8 of the last archive tile: zero codes, zero scales
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const uint32_t row = (uint32_t)(kb + 16 * b + c);
#pragma unroll
                    for (int a = 0; a < 2; ++a) kr[2 * b + a] = load16(rk8, row * 128u + 16u * (4 * a + g));
                    kr[4][b] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rks, row * 4u, 0, 0);
                }
                return;
            }
            kb -= L8p;
        }
        if constexpr (SHARED) {
            if (kb < Lsp) {   // rows >= Ls of the last shared tile read as zero
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        kr[4 * b + s] = load16(rsk, (uint32_t)(kb + 16 * b + c) * s16.row_bytes + (uint32_t)dec_step_off(s, g));
                return;
            }
            kb -= Lsp;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kr[4 * b + s] = load16(rk, (uint32_t)(kb + 16 * b + c) * kv_row_bytes + (uint32_t)dec_step_off(s, g));
    };
    auto load_v = [&](int kb) {
        if constexpr (FP8) {
            if (kb < L8p) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t row = (uint32_t)(kb + 8 * u + (lane >> 3));
                    vr[u] = load16(rv8, row * 128u + 16u * (lane & 7));
                    vr[4][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rvs, row * 4u, 0, 0);
                }
                return;
            }
            kb -= L8p;
        }
        if constexpr (SHARED) {
            if (kb < Lsp) {
#pragma unroll
                for (int u = 0; u < 8; ++u) vr[u] = load16(rsv, (uint32_t)(kb + 4 * u + g) * s16.row_bytes + 16u * c);
                return;
            }
            kb -= Lsp;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) vr[u] = load16(rv, (uint32_t)(kb + 4 * u + g) * kv_row_bytes + 16u * c);
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

    // tile kb; `next`: this wave has a tile at kb + DEC_STEP, whose loads are issued as soon as the registers are free
    auto process = [&](int kb, bool next) {
        bool arch = false;
        if constexpr (FP8) arch = kb < L8p;
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
        // a tile of the archive or of the shared rows: every row sees it whole, up to the segment's last row
        bool seg = arch;
        int seg_vis = L8 - 1;
        if constexpr (SHARED) {
            if (!arch && kb < L8p + Lsp) {
                seg = true;
                seg_vis = L8p + Ls - 1;
            }
        }
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
            if (cg == NCG - 1 && next) load_k(kb + DEC_STEP);
            // the last key this row sees: its diagonal or the end of the keys
            const int lim = (seg ? seg_vis : min(off + qi[cg], Lk - 1)) - kb;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (4 * g + e > lim) s0[e] = -INFINITY;
                if (16 + 4 * g + e > lim) s1[e] = -INFINITY;
            }
            pf[cg] = dec_softmax_step<DT>(s0, s1, c2, m[cg], l[cg], oacc[cg]);
        }
        if (seg || kb + DEC_T - 1 <= off) {   // every row sees every key of the tile that exists (keys >= Lk read as zero)
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
                if (kb > min(off + i_hi, Lk - 1)) continue;   // hidden from every row of the group: its probabilities are 0
                if (kb + DEC_T - 1 <= off + i_lo) {           // every row of the group sees the tile whole
#pragma unroll
                    for (int db = 0; db < 8; ++db) oacc[cg][db] = mma32<DT>(dec_v_frag(vt + v_rd, db), pf[cg], oacc[cg][db]);
                    continue;
                }
                // one pass per position: V rows above its diagonal zeroed, the lanes of its packed rows keep the result
                for (int i = i_lo; i <= i_hi; ++i) {
                    const int li = min(off + i, Lk - 1) - kb;
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
        load_k(kb0);
        load_v(kb0);
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

// attention_decode_d128_body.inc - the body of attn_decode_d128_kernel / attn_decode_d128_shared_kernel
// (attention_decode.hip), which include it with `constexpr bool FP8, SHARED`, `Archive8 a8` and `Shared16 s16` in scope,
// besides their common parameters.  (The same text compiles the existing instantiations to the same code; a function the
// kernels shared would not - tools/kernel_diff.py.  dec_step_off, dec_v_frag and dec_softmax_step, which the group
// kernel uses too, are functions of attention_decode.hip: those leave this body's code as it was.)
    __shared__ __attribute__((aligned(16))) char lds[4 * DEC_WAVE_LDS];   // [wave]: V tile, then the wave's O
    __shared__ float ml_s[4][DEC_R][2];
    // FP8: from here on Lk and off count in the padded key space
    const int L8 = FP8 ? a8.L8 : 0, L8p = (L8 + DEC_T - 1) / DEC_T * DEC_T;
    if constexpr (FP8) {
        Lk += L8p;
        off += L8p;
    }
    // SHARED: one more padded segment, [L8p, L8p + Lsp), between the archive and the kernel's own rows
    const int Ls = SHARED ? s16.Ls : 0, Lsp = (Ls + DEC_T - 1) / DEC_T * DEC_T;
    if constexpr (SHARED) {
        Lk += Lsp;
        off += Lsp;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int c = lane & 15, g = lane >> 4;   // packed row (column) and lane group
    const int split = blockIdx.x, hkv = blockIdx.y, R = G * Lq;
    const int qi = c % Lq, qg = c / Lq;       // query position and head-in-group of packed row c
    const int k_lo = split * keys_per_split;
    const int k_hi = min(min(Lk, off + Lq), k_lo + keys_per_split);   // exclusive: first key no row of the range sees
    const int vis_r = min(off + qi, Lk - 1);                          // last key packed row c sees

    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(k + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(v + (int64_t)hkv * kv_sh * 2, kv_bytes);
    __amdgpu_buffer_rsrc_t rk8 = rk, rv8 = rk, rks = rk, rvs = rk;
    if constexpr (FP8) {
        rk8 = bounded_rsrc(a8.k8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rv8 = bounded_rsrc(a8.v8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rks = bounded_rsrc(a8.ks + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
        rvs = bounded_rsrc(a8.vs + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
    }

    __amdgpu_buffer_rsrc_t rsk = rk, rsv = rk;
    if constexpr (SHARED) {
        rsk = bounded_rsrc(s16.k + (int64_t)hkv * s16.sh * 2, s16.bytes);
        rsv = bounded_rsrc(s16.v + (int64_t)hkv * s16.sh * 2, s16.bytes);
    }

    // Q fragments (B operand): packed row c, zero for c >= R
    u32x4 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = u32x4{0u, 0u, 0u, 0u};
    if (c < R) {
        const char* qr = q + ((int64_t)(hkv * G + qg) * q_sh + (int64_t)qi * q_sl) * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const u32x4*)(qr + dec_step_off(s, g));
    }

    // One tile's operands, in flight from the moment the previous tile's are consumed.  16-bit tile: kr[4 b + s] = the step-s chunk of key row 16 b + c; vr[u] = chunk c of
    // V row 4 u + g.  Archive tile: kr[2 b + a] = codes 16 (4 a + g) .. + 15 of key row 16 b + c, its scale in kr[4][b];
    // vr[u] = codes 16 (lane & 7) .. + 15 of V row 8 u + (lane >> 3), its scale in vr[4][u].
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
    // transposed V reads: lane 4 q_ + p_ of a 16-lane group supplies row q_ of a 4-key block, columns 4 p_ .. 4 p_ + 3 of a
    // d-block; it receives column c of the block's 4 rows.  Group g takes the blocks at keys 4 g and 16 + 4 g: the keys of
    // the lane's own logits, in the order they are packed below.
    const int v_rd = DEC_VPITCH * (4 * g + (c >> 2)) + 8 * (c & 3);

    f32x4 oacc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

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
        // logits: s0[e] = key 4 g + e, s1[e] = key 16 + 4 g + e of the tile, packed row c
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            s0 = mma32<DT>(ka[s], qf[s], s0);
            s1 = mma32<DT>(ka[4 + s], qf[s], s1);
        }
        if (next) load_k(kb + DEC_STEP);
        // the last key this row sees: its diagonal or the end of the keys - of an archive tile, which every row sees
        // whole, the last archive row
        // (a shared tile likewise: the last shared row)
        int vis = arch ? L8 - 1 : vis_r;
        if constexpr (SHARED) {
            if (!arch && kb < L8p + Lsp) vis = L8p + Ls - 1;
        }
        const int lim = vis - kb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * g + e > lim) s0[e] = -INFINITY;
            if (16 + 4 * g + e > lim) s1[e] = -INFINITY;
        }
        const u32x4 pf = dec_softmax_step<DT>(s0, s1, c2, m, l, oacc);
        if (arch || kb + DEC_T - 1 <= off) {   // every row sees every key of the tile that exists (keys >= Lk read as zero)
#pragma unroll
            for (int db = 0; db < 8; ++db) oacc[db] = mma32<DT>(dec_v_frag(vt + v_rd, db), pf, oacc[db]);
        } else {
            // one pass per query position: V rows above its diagonal zeroed, the lanes of its packed rows keep the result
            for (int i = 0; i < Lq; ++i) {
                const int li = min(off + i, Lk - 1) - kb;
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
        load_k(kb0);
        load_v(kb0);
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

// attention_d128_body.inc - the body of attn_fwd_d128_kernel / attn_fwd_d128_fp8kv_kernel / attn_fwd_d128_shared_kernel
// (attention.hip), which include it with `constexpr bool FP8, SHARED`, `Archive8 a8` and `Shared16 s16` in scope, besides
// their common parameters.
    using Hh = H16<DT>;
    __shared__ __attribute__((aligned(16))) char lds[4 * AT_TILE];   // [buffer][K | V]
    // FP8: from here on Lk and off count in the padded key space (see attention.hip)
    const int L8 = FP8 ? a8.L8 : 0, L8p = (L8 + AT_KT - 1) / AT_KT * AT_KT;
    if constexpr (FP8) {
        Lk += L8p;
        off += L8p;
    }
    // SHARED: one more padded segment, [L8p, L8p + Lsp), between the archive and the kernel's own rows
    const int Ls = SHARED ? s16.Ls : 0, Lsp = (Ls + AT_KT - 1) / AT_KT * AT_KT;
    if constexpr (SHARED) {
        Lk += Lsp;
        off += Lsp;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_int(tid >> 6);
    const int r = lane & 31, hf = lane >> 5;
    const int nqb = (Lq + AT_QB - 1) / AT_QB;
    const int qb = nqb - 1 - (int)blockIdx.x / Hq;   // heaviest (last) query block first
    const int hq = (int)blockIdx.x % Hq, hkv = hq / G;
    const int row_base = qb * AT_QB, wrow0 = row_base + 32 * wave, qrow = wrow0 + r;
    int k_lo = 0, k_hi = min(Lk, off + min(row_base + AT_QB, Lq));   // exclusive: first key no row of the block sees
    if constexpr (SPLIT) {
        k_lo = (int)blockIdx.y * keys_per_split;
        k_hi = min(k_hi, k_lo + keys_per_split);
    }
    const int ntiles = k_hi > k_lo ? (k_hi - k_lo + AT_KT - 1) / AT_KT : 0;
    const bool wave_rows = wrow0 < Lq;
    const int wave_hi = min(Lk, off + min(wrow0 + 32, Lq));   // first key no row of this wave sees

    const __amdgpu_buffer_rsrc_t rq = bounded_rsrc(q + (int64_t)hq * q_sh * 2, q_bytes);
    const __amdgpu_buffer_rsrc_t rk = bounded_rsrc(k + (int64_t)hkv * kv_sh * 2, kv_bytes);
    const __amdgpu_buffer_rsrc_t rv = bounded_rsrc(v + (int64_t)hkv * kv_sh * 2, kv_bytes);
    __amdgpu_buffer_rsrc_t rsk = rk, rsv = rk;
    if constexpr (SHARED) {
        rsk = bounded_rsrc(s16.k + (int64_t)hkv * s16.sh * 2, s16.bytes);
        rsv = bounded_rsrc(s16.v + (int64_t)hkv * s16.sh * 2, s16.bytes);
    }
    // archive tiles: thread -> rows arow, arow + 32, codes 16 acc_ .. 16 acc_ + 15 (the row's chunks 2 acc_, 2 acc_ + 1).
    // Consecutive 8-lane groups take rows r, r + 4, r + 1, r + 5, ...: the swizzle's parity alternates, so the 16 lanes of
    // an LDS write hold the even chunks of one row and the odd chunks of another - every bank once.
    __amdgpu_buffer_rsrc_t rk8 = rk, rv8 = rk, rks = rk, rvs = rk;
    // (register budget: one global offset, one LDS offset; the rows' scales ride in kst[2] / vst[2], which an archive tile
    // does not load)
    int a8_off = 0, l8_a = 0;
    if constexpr (FP8) {
        rk8 = bounded_rsrc(a8.k8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rv8 = bounded_rsrc(a8.v8 + (int64_t)hkv * a8.sh8, (uint32_t)L8 * 128u);
        rks = bounded_rsrc(a8.ks + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
        rvs = bounded_rsrc(a8.vs + (int64_t)hkv * a8.shs, (uint32_t)L8 * 4u);
        const int rs_ = tid >> 3, acc_ = tid & 7;
        const int arow = (rs_ & ~7) | ((rs_ & 1) << 2) | ((rs_ >> 1) & 3);
        a8_off = 128 * arow + 16 * acc_;                              // codes; the row's scale is at (a8_off >> 7) * 4
        l8_a = 256 * arow + 16 * ((2 * acc_) ^ swz(arow));            // chunk 2 acc; chunk 2 acc + 1 is at l8_a ^ 16
    }

    // Q fragments: k-step s holds q[qrow][16 s + 8 hf .. + 8]
    u32x4 qf[8];
    {
        const uint32_t qo = (uint32_t)qrow * q_row_bytes + 16u * hf;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = load16(rq, qo + 32u * s);
    }
    // staging: thread -> rows (tid >> 4) + 16 u, chunk tid & 15
    const int srow = tid >> 4, sch = tid & 15;
    const uint32_t g_off = (uint32_t)srow * kv_row_bytes + 16u * sch;
    const int l_off = 256 * srow + 16 * (sch ^ swz(srow));   // + 4096 u (rows 16 apart share the swizzle)
    u32x4 kst[4], vst[4];
    auto issue = [&](int kbase) {
        if constexpr (FP8) {
            if (kbase < L8p) {   // rows >= L8 of the last archive tile: zero codes, zero scales
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t o = (uint32_t)(kbase + 32 * u) * 128u + (uint32_t)a8_off, so = (o >> 7) * 4u;
                    kst[u] = load16(rk8, o);
                    vst[u] = load16(rv8, o);
                    kst[2][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rks, so, 0, 0);
                    vst[2][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rvs, so, 0, 0);
                }
                return;
            }
            kbase -= L8p;
        }
        if constexpr (SHARED) {
            if (kbase < Lsp) {   // rows >= Ls of the last shared tile read as zero
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t o = (uint32_t)(kbase + srow + 16 * u) * s16.row_bytes + 16u * sch;
                    kst[u] = load16(rsk, o);
                    vst[u] = load16(rsv, o);
                }
                return;
            }
            kbase -= Lsp;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t o = g_off + (uint32_t)(kbase + 16 * u) * kv_row_bytes;
            kst[u] = load16(rk, o);
            vst[u] = load16(rv, o);
        }
    };
    auto commit = [&](int buf, int kbase) {
        if constexpr (FP8) {
            if (kbase < L8p) {   // the image a 16-bit tile of the dequantised rows would have left
                char* t8 = lds + buf * 2 * AT_TILE;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    u32x4 a, b;
                    fp8_dequant16<DT>(kst[u], __uint_as_float(kst[2][u]), a, b);
                    *(u32x4*)(t8 + 8192 * u + l8_a) = a;
                    *(u32x4*)(t8 + 8192 * u + (l8_a ^ 16)) = b;
                    fp8_dequant16<DT>(vst[u], __uint_as_float(vst[2][u]), a, b);
                    *(u32x4*)(t8 + AT_TILE + 8192 * u + l8_a) = a;
                    *(u32x4*)(t8 + AT_TILE + 8192 * u + (l8_a ^ 16)) = b;
                }
                return;
            }
        }
        char* t = lds + buf * 2 * AT_TILE + l_off;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *(u32x4*)(t + 4096 * u) = kst[u];
            *(u32x4*)(t + AT_TILE + 4096 * u) = vst[u];
        }
    };
    // K row reads: key row r (+32), chunk 2 s + hf
    const int k_rd = 256 * r, k_x = swz(r);
    // V transposed reads: lane 4 q_ + p_ of a 16-lane group supplies row q_ of the 4-key block, columns 4 p_ .. 4 p_ + 3
    const int g16 = lane >> 4, q_ = (lane & 15) >> 2, p_ = lane & 3;
    const int v_rd = 256 * (4 * hf + q_) + 8 * (p_ & 1);
    const int v_cl = 2 * (g16 & 1) + (p_ >> 1);   // low bits of the chunk: which 16 of a d-block's 32 columns, which half

    f32x16 oacc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[db][e] = 0.f;
    float m = -INFINITY, l = 0.f;

    if (ntiles > 0) {
        issue(k_lo);
        commit(0, k_lo);
    }
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int kbase = k_lo + t * AT_KT;
        const bool more = t + 1 < ntiles;
        if (more) issue(kbase + AT_KT);
        if (wave_rows && kbase < wave_hi) {
            const char* kt = lds + (t & 1) * 2 * AT_TILE;
            const char* vt = kt + AT_TILE;
            f32x16 s0, s1;
#pragma unroll
            for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int co = 16 * ((2 * s + hf) ^ k_x);
                const u32x4 a0 = *(const u32x4*)(kt + k_rd + co);
                const u32x4 a1 = *(const u32x4*)(kt + k_rd + 32 * 256 + co);
                mma16<DT>(s0, a0, qf[s]);
                mma16<DT>(s1, a1, qf[s]);
            }
            // the last key the whole wave / this row sees: the diagonal or the end of the keys - of an archive tile, which
            // every row sees whole, the last archive row (the last such tile may hold fewer than 64)
            int vis_w = min(off + wrow0, Lk - 1), vis_r = min(off + qrow, Lk - 1);
            if constexpr (FP8) {
                if (kbase < L8p) vis_w = vis_r = L8 - 1;
            }
            if constexpr (SHARED) {   // likewise a shared tile: the last shared row
                if (kbase >= L8p && kbase < L8p + Lsp) vis_w = vis_r = L8p + Ls - 1;
            }
            if (kbase + AT_KT - 1 > vis_w) {   // the tile straddles one of them
                const int lim = vis_r - kbase;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = acc_row(e, hf);
                    if (j > lim) s0[e] = -INFINITY;
                    if (j + 32 > lim) s1[e] = -INFINITY;
                }
            }
            float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmaxf(mx, fmaxf(s0[e], s1[e]));
            mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
            const float mnew = fmaxf(m, mx * c2);
            if (!__all(mnew == m)) {   // some row's maximum grew: bring O and l to the new one (exact, no threshold)
                const float alpha = __builtin_amdgcn_exp2f(m - safe_max(mnew));
#pragma unroll
                for (int db = 0; db < 4; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) oacc[db][e] *= alpha;
                l *= alpha;
                m = mnew;
            }
            const float nm = -safe_max(m);
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s0[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], c2, nm));
                s1[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[e], c2, nm));
                ls += s0[e] + s1[e];
            }
            l += ls;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {   // k-step: keys 16 ks .. 16 ks + 15 of the tile
                const f32x16& p = ks < 2 ? s0 : s1;
                const int e0 = 8 * (ks & 1);
                const u32x4 pf = {Hh::pack2(p[e0], p[e0 + 1]), Hh::pack2(p[e0 + 2], p[e0 + 3]),
                                  Hh::pack2(p[e0 + 4], p[e0 + 5]), Hh::pack2(p[e0 + 6], p[e0 + 7])};
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    u32x2 h2[2];
#pragma unroll
                    for (int jh = 0; jh < 2; ++jh) {
                        // rows 16 ks + 8 jh + 4 hf + q_: (row & 3) = q_, ((row >> 2) & 3) = 2 jh + hf
                        const int x = (q_ << 2) | (2 * jh + hf);
                        const int a = v_rd + 256 * (16 * ks + 8 * jh) + 16 * ((4 * db + v_cl) ^ x);
                        const i16x4 t4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) i16x4*)(vt + a));
                        h2[jh] = __builtin_bit_cast(u32x2, t4);
                    }
                    const u32x4 vf = {h2[0][0], h2[0][1], h2[1][0], h2[1][1]};
                    mma16<DT>(oacc[db], vf, pf);
                }
            }
        }
        if (more) commit((t + 1) & 1, kbase + AT_KT);
        __syncthreads();
    }

    const float l_tot = l + __shfl_xor(l, 32, WAVE);
    if constexpr (SPLIT) {
        if (qrow < Lq) {
            const size_t row = ((size_t)blockIdx.y * Hq + hq) * Lq + qrow;
            if (hf == 0) *(float2*)(part_ml + 2 * row) = make_float2(m, l_tot);
            float* pa = part_acc + row * 128;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(f32x4*)(pa + 32 * db + 8 * g4 + 4 * hf) =
                        f32x4{oacc[db][4 * g4], oacc[db][4 * g4 + 1], oacc[db][4 * g4 + 2], oacc[db][4 * g4 + 3]};
        }
    } else {
        // every wave has left the tile loop (the barrier above): stage this wave's 32 rows, store them as whole rows
        const float inv = 1.f / l_tot;
        char* st = lds + wave * (32 * AT_OPITCH);
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(u32x2*)(st + r * AT_OPITCH + 2 * (32 * db + 8 * g4 + 4 * hf)) =
                    u32x2{Hh::pack2(oacc[db][4 * g4] * inv, oacc[db][4 * g4 + 1] * inv),
                          Hh::pack2(oacc[db][4 * g4 + 2] * inv, oacc[db][4 * g4 + 3] * inv)};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int rr = 4 * it + (lane >> 4), ch = lane & 15;
            const u32x4 x = *(const u32x4*)(st + rr * AT_OPITCH + 16 * ch);
            if (wrow0 + rr < Lq) *(u32x4*)(out + ((size_t)(wrow0 + rr) * Hq + hq) * 256 + 16 * ch) = x;
        }
    }

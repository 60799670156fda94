#!/usr/bin/env python
"""Chunk attention: the native HIP call against the SDPA route of the attention patches, same tensors, same process.

    python tools/bench_attention.py [--out profiles/attention_bench.json] [--reps 20] [--warmup 3] [--shapes chunk|all]
                                    [--routes native,sdpa,fa2]      (--routes native: the run to put under rocprofv3)

Per shape (Hq 28 / Hkv 4 / D 128; bf16, and fp16 once), inputs resident on the device (gaussian, tests/synth.py scale):
  native   PivotKVCache.attention's call (retake.native_attention.chunk_attention) on the patches' own tensors: q the
           transposed view of [1, Lq, Hq*D], k / v the [:P0 + Lq] view of a [1, Hkv, capacity, D] cache buffer;
  sdpa     what retake_Qwen2VLSdpaAttention_forward does with the same tensors when the switch is off: repeat_kv,
           .contiguous(), scaled_dot_product_attention with the [1, 1, Lq, Lk] additive mask, transpose + contiguous;
  fa2      transformers' _flash_attention_forward when the flash_attn package is importable (else recorded as absent).
HIP events around each launch sequence, warm-up, then the median of `reps` launches.  A route that cannot run a shape (out
of memory) is recorded with its error, not skipped.  Reported: microseconds, 4 Hq Lq (P0 + (Lq + 1) / 2) D flop over time
as a fraction of 2.5 PFLOP/s (the dense bf16 MFMA peak), the allocator peak of each route above the resident inputs, and
the ratio sdpa / native.  One JSON document; a markdown table on stdout.

    python tools/bench_attention.py --fp8kv [--out profiles/fp8kv_attention_bench.json]

The same shapes with the first P0 keys as fp8 rows (kv_cache_dtype="fp8_e4m3"): the two-segment call
(rtk_attention_forward_fp8kv: e4m3 archive + 16-bit tail) against the 16-bit kernel on [dequantised archive | tail], same
process, same timing; whether the two outputs are bit-equal (they must be when P0 % 64 == 0) is recorded per shape.

    python tools/bench_attention.py --decode [--fp8kv] [--out profiles/[fp8kv_]decode_attention_bench.json]

The few-row shapes of generation - Lq 1 and 2 over Lk 4 000, 25 088 and 100 352 (bf16, and fp16 once) - through the
GQA-packed kernel (rtk_attention_decode) and through rtk_attention_forward, the call it replaces, on the same tensors in
this same process, beside the SDPA route.  Both native entry points are called directly with a resident output and
workspace (the host cost of chunk_attention, tens of microseconds, would otherwise be most of a packed call), DECODE_INNER
calls back to back between one pair of HIP events, the time divided by DECODE_INNER; the median of `reps` such samples.
Reported per shape: the K/V bytes one call reads once, what fraction of 8 TB/s and of the calibration copy
(rtk_profile_copy over a 2 GiB buffer, read + write bytes) the packed call reaches on them, and the milliseconds per
generated token (x 28 layers).  --fp8kv: all but the last Lq keys as fp8 rows - the packed two-segment call, the packed
16-bit call on [dequantised archive | tail] (their ratio, and whether the outputs are bit-equal: they must be when
L8 % 32 == 0), and rtk_attention_forward_fp8kv.

    python tools/bench_attention.py --group [--out profiles/group_decode_bench.json]

B = 1, 2 and 4 branches of one fork point decoding a token each (Hq 28 / Hkv 4, 100 352 shared rows, 64 own rows per
branch, bf16): ONE rtk_attention_decode_group call against the B successive rtk_attention_decode_shared calls it replaces,
same tensors, same process, every entry point called directly with resident outputs and workspaces.  Once with the shared
rows as 16-bit rows and once as an fp8 archive in their place.  A sample is DECODE_INNER steps between one pair of HIP
events; the samples of the two routes are INTERLEAVED (group, successive, group, ...), the median of `reps` each.
Reported: microseconds per step, their ratio, the shared bytes a step reads once, and what fraction of 8 TB/s the group
call reaches on them.

    python tools/bench_attention.py --wide [--out profiles/wide_decode_bench.json]

The verification step of assisted generation - Lq 3, 6 and 9 new rows (Hq 28 / Hkv 4: 21, 42 and 63 packed rows, bf16) over
100 352 keys held as plain rows, as 100 352 shared rows + 64 own rows, and as an fp8 archive in place of the shared rows:
the wide packed call (rtk_attention_decode_wide / _wide_shared / _wide_fp8kv) against the chunk-kernel call it replaces
(rtk_attention_forward / _forward_shared / _forward_fp8kv, the route without multi_token_attention) and against the packed
call at Lq 1 on the same keys, every entry point called directly with resident outputs and workspaces.  A sample is
DECODE_INNER calls between one pair of HIP events; the samples of the three routes are INTERLEAVED, and each route
reports its median with the quartiles.  `faster_beyond_iqr`: the replaced call's median exceeds the wide call's by more
than the sum of the two interquartile ranges - the condition for the Python dispatcher to send the shape to the wide kernel.
The other geometries the envelope admits (WIDE_OTHER: G = 8, 4, 1 and 16) are timed the same way over the plain rows.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

PEAK_FLOPS = 2.5e15
HQ, HKV, D = 28, 4, 128
CHUNK_SHAPES = [(2304, 0), (2304, 3456), (2304, 7488), (6272, 0), (6272, 50176), (6272, 98784)]
FEW_ROW_SHAPES = [(5, 100352 - 5), (1, 100352 - 1)]   # text segment / decode step over Lk 100 352
DECODE_SHAPES = [(Lq, Lk - Lq) for Lk in (4000, 25088, 100352) for Lq in (1, 2)]
DECODE_INNER = 10     # launches per timed sample of --decode
LAYERS = 28           # attention calls per generated token
HBM_PEAK = 8e12


def flop(Lq, P0):
    return 4.0 * HQ * Lq * (P0 + (Lq + 1) / 2.0) * D


def make(Lq, P0, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    Lk = P0 + Lq
    cap = Lk + 256
    q = (1.7 * torch.randn((1, Lq, HQ * D), generator=g, device=dev)).to(dtype).view(1, Lq, HQ, D).transpose(1, 2)
    kb = (1.7 * torch.randn((1, HKV, cap, D), generator=g, device=dev)).to(dtype)
    vb = (1.7 * torch.randn((1, HKV, cap, D), generator=g, device=dev)).to(dtype)
    mask = torch.zeros((1, 1, Lq, Lk), dtype=dtype, device=dev)
    rows = torch.arange(Lq, device=dev)[:, None]
    mask[0, 0].masked_fill_(torch.arange(Lk, device=dev)[None, :] > P0 + rows, torch.finfo(dtype).min)
    return q, kb[:, :, :Lk], vb[:, :, :Lk], mask


def timed(fn, reps, warmup):
    """(median us, allocator peak in bytes above what was held before, last result)."""
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    del out
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), torch.cuda.max_memory_allocated() - held, out


def main_fp8kv(args):
    import retake.longvideo_cache as lc

    dev = torch.device("cuda:0")
    cases = [(s, torch.bfloat16, "chunk") for s in CHUNK_SHAPES] + [(CHUNK_SHAPES[1], torch.float16, "chunk")]
    if args.shapes == "all":
        cases += [(s, torch.bfloat16, "few rows") for s in FEW_ROW_SHAPES]
    rows = []
    for (Lq, P0), dtype, kind in cases:
        q, k, v, _ = make(Lq, P0, dtype, dev)
        del _
        ak, sk = lc.fp8_quantize_rows(k[:, :, :P0].contiguous())
        av, sv = lc.fp8_quantize_rows(v[:, :, :P0].contiguous())
        kd, vd = k.clone(), v.clone()                   # [dequantised archive | tail]
        lc.fp8_dequantize_rows(ak, sk, dtype, kd[:, :, :P0])
        lc.fp8_dequantize_rows(av, sv, dtype, vd[:, :, :P0])
        kt, vt = k[:, :, P0:], v[:, :, P0:]
        archive = (ak, av, sk, sv)
        ws = {}
        row = {"Lq": Lq, "L8": P0, "Lk16": Lq, "Hq": HQ, "Hkv": HKV, "D": D, "dtype": str(dtype)[6:], "kind": kind,
               "flop": flop(Lq, P0), "reps": args.reps, "kv_bytes_fp8kv": 2 * HKV * (P0 * (D + 4) + Lq * D * 2),
               "kv_bytes_16bit": 2 * HKV * (P0 + Lq) * D * 2}
        outs = {}
        for name, fn in (("fp8kv", lambda: lc.chunk_attention(q, kt, vt, workspace=ws, archive=archive)),
                         ("dense16", lambda: lc.chunk_attention(q, kd, vd, workspace=ws))):
            us, peak, out = timed(fn, args.reps, args.warmup)
            row[name] = {"status": "ok", "us": us, "fraction_of_2.5_PFLOPs": row["flop"] / (us * 1e-6) / PEAK_FLOPS,
                         "allocator_peak_bytes": int(peak)}
            outs[name] = out
        row["ratio_fp8kv_over_dense16"] = row["fp8kv"]["us"] / row["dense16"]["us"]
        row["bit_equal"] = bool(torch.equal(outs["fp8kv"], outs["dense16"]))
        row["max_abs_diff"] = (outs["fp8kv"].float() - outs["dense16"].float()).abs().max().item()
        rows.append(row)
        del q, k, v, kd, vd, kt, vt, archive, ak, av, sk, sv, outs, ws
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "peak_flops": PEAK_FLOPS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("\n| dtype | Lq | L8 | fp8kv us | 16-bit kernel on dequantised rows us | fp8kv / 16-bit | K/V bytes read fp8kv / 16-bit | bit-equal |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dtype']} | {r['Lq']} | {r['L8']} | {r['fp8kv']['us']:.0f} | {r['dense16']['us']:.0f} | "
              f"{r['ratio_fp8kv_over_dense16']:.2f} | {r['kv_bytes_fp8kv'] / r['kv_bytes_16bit']:.2f} | {r['bit_equal']} |")


def copy_rate(dev):
    """bytes / s (read + write) of rtk_profile_copy over a 2 GiB buffer: the calibration of bench.py's hbm_achievable."""
    import retake._native as nv

    n = 1 << 31
    src = torch.empty(n, dtype=torch.uint8, device=dev).random_()
    dst = torch.empty_like(src)
    fn = lambda: nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), n, nv.stream()), "rtk_profile_copy")   # noqa: E731
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 2 * n * 5 / (e0.elapsed_time(e1) * 1e-3)


def main_decode(args):
    import retake._native as nv
    import retake.longvideo_cache as lc

    dev = torch.device("cuda:0")
    G = HQ // HKV
    copy = copy_rate(dev)
    torch.cuda.empty_cache()
    cases = [(s, torch.bfloat16) for s in DECODE_SHAPES] + [(DECODE_SHAPES[-2], torch.float16)]
    rows = []
    for (Lq, P0), dtype in cases:
        q, k, v, mask = make(Lq, P0, dtype, dev)
        Lk, code, stream = P0 + Lq, nv.dtype_code(q), nv.stream()
        out = torch.empty((1, Lq, HQ, D), dtype=dtype, device=dev)
        scale = D ** -0.5
        L8 = P0 // 32 * 32 if args.fp8kv else 0     # whole key tiles: the two packed calls must then agree bit for bit
        kd, vd = k, v
        if args.fp8kv:
            ak, sk = lc.fp8_quantize_rows(k[:, :, :L8].contiguous())
            av, sv = lc.fp8_quantize_rows(v[:, :, :L8].contiguous())
            kd, vd = k.clone(), v.clone()               # [dequantised archive | tail]
            lc.fp8_dequantize_rows(ak, sk, dtype, kd[:, :, :L8])
            lc.fp8_dequantize_rows(av, sv, dtype, vd[:, :, :L8])
            kt, vt = k[:, :, L8:], v[:, :, L8:]
            a8 = (nv.ptr(ak), nv.ptr(av), nv.ptr(sk), nv.ptr(sv), L8, ak.stride(1), sk.stride(1))

        def direct(fn, kk, vv, archive=()):
            """DECODE_INNER back-to-back calls of one entry point on (q, kk, vv), resident output and workspace."""
            sfx = "_fp8kv" if archive else ""
            n8 = archive[4] if archive else 0
            shape = (HQ, HKV, Lq, kk.shape[2]) + ((n8,) if archive else ()) + (D, code)
            need = getattr(nv.lib, fn + "_workspace_bytes" + sfx)(*shape)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            call = getattr(nv.lib, fn + sfx)
            a = (nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(kk), nv.ptr(vv), kk.stride(1), kk.stride(2)) + tuple(archive) + \
                (nv.ptr(out), HQ, HKV, Lq, kk.shape[2], kk.shape[2] - Lq, D, code, scale, nv.ptr(ws), need, stream)

            def run():
                for _ in range(DECODE_INNER):
                    nv.check(call(*a), fn + sfx)
                return out
            return run

        def sdpa():
            for _ in range(DECODE_INNER):
                kk, vv = lc.repeat_kv(kd, G), lc.repeat_kv(vd, G)
                qc, kc, vc = (t.contiguous() for t in (q, kk, vv))
                o = torch.nn.functional.scaled_dot_product_attention(qc, kc, vc, attn_mask=mask, dropout_p=0.0, is_causal=False)
                o = o.transpose(1, 2).contiguous()
            return o

        if args.fp8kv:
            routes = (("packed_fp8kv", direct("rtk_attention_decode", kt, vt, a8)),
                      ("packed_dense16", direct("rtk_attention_decode", kd, vd)),
                      ("forward_fp8kv", direct("rtk_attention_forward", kt, vt, a8)))
            kv_bytes = 2 * HKV * (L8 * (D + 4) + (Lk - L8) * D * 2)
        else:
            routes = (("packed", direct("rtk_attention_decode", k, v)), ("forward", direct("rtk_attention_forward", k, v)),
                      ("sdpa", sdpa))
            kv_bytes = 2 * HKV * Lk * D * 2
        row = {"Lq": Lq, "P0": P0, "Lk": Lk, "Hq": HQ, "Hkv": HKV, "D": D, "dtype": str(dtype)[6:], "reps": args.reps,
               "inner": DECODE_INNER, "kv_bytes": kv_bytes, "copy_bytes_per_s": copy}
        if args.fp8kv:
            row["L8"] = L8
        outs = {}
        for name, fn in routes:
            us, _, o = timed(fn, args.reps, args.warmup)
            outs[name] = o.clone()   # (the native routes share one resident output)
            row[name] = {"us": us / DECODE_INNER, "ms_per_token": us / DECODE_INNER * LAYERS * 1e-3}
        first = routes[0][0]
        t = row[first]["us"] * 1e-6
        row[first].update({"fraction_of_8_TBps": kv_bytes / t / HBM_PEAK, "fraction_of_copy": kv_bytes / t / copy})
        if args.fp8kv:
            row["ratio_fp8kv_over_dense16"] = row["packed_fp8kv"]["us"] / row["packed_dense16"]["us"]
            row["ratio_forward_fp8kv_over_packed_fp8kv"] = row["forward_fp8kv"]["us"] / row["packed_fp8kv"]["us"]
            row["bit_equal"] = bool(torch.equal(outs["packed_fp8kv"], outs["packed_dense16"]))
        else:
            row["ratio_forward_over_packed"] = row["forward"]["us"] / row["packed"]["us"]
            row["ratio_sdpa_over_packed"] = row["sdpa"]["us"] / row["packed"]["us"]
            row["max_abs_diff_packed_vs_forward"] = (outs["packed"].float() - outs["forward"].float()).abs().max().item()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del q, k, v, kd, vd, mask, outs, routes
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK,
           "copy_bytes_per_s": copy, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    if args.fp8kv:
        print("\n| dtype | Lq | L8 | packed fp8kv us | packed 16-bit on dequantised rows us | fp8kv / 16-bit | rtk_attention_forward_fp8kv us "
              "| K/V MB | of 8 TB/s | of the copy | ms / token | bit-equal |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            p = r["packed_fp8kv"]
            print(f"| {r['dtype']} | {r['Lq']} | {r['L8']} | {p['us']:.1f} | {r['packed_dense16']['us']:.1f} | "
                  f"{r['ratio_fp8kv_over_dense16']:.2f} | {r['forward_fp8kv']['us']:.1f} | {r['kv_bytes'] / 1e6:.1f} | "
                  f"{p['fraction_of_8_TBps']:.3f} | {p['fraction_of_copy']:.3f} | {p['ms_per_token']:.2f} | {r['bit_equal']} |")
        return
    print("\n| dtype | Lq | Lk | packed us | rtk_attention_forward us | forward / packed | SDPA route us | K/V MB | of 8 TB/s "
          "| of the copy | packed ms / token | forward ms / token |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        p = r["packed"]
        print(f"| {r['dtype']} | {r['Lq']} | {r['Lk']} | {p['us']:.1f} | {r['forward']['us']:.1f} | {r['ratio_forward_over_packed']:.2f} | "
              f"{r['sdpa']['us']:.1f} | {r['kv_bytes'] / 1e6:.1f} | {p['fraction_of_8_TBps']:.3f} | {p['fraction_of_copy']:.3f} | "
              f"{p['ms_per_token']:.2f} | {r['forward']['ms_per_token']:.2f} |")

GROUP_SHARED, GROUP_OWN, GROUP_BRANCHES = 100352, 64, (1, 2, 4)


def main_group(args):
    import ctypes as C

    import retake._native as nv
    import retake.longvideo_cache as lc

    dev = torch.device("cuda:0")
    dtype, code, scale, stream = torch.bfloat16, nv.RTK_BF16, D ** -0.5, nv.stream()
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: (1.7 * torch.randn(shape, generator=g, device=dev)).to(dtype)   # noqa: E731
    ks, vs = rnd(1, HKV, GROUP_SHARED, D), rnd(1, HKV, GROUP_SHARED, D)
    ak, sk = lc.fp8_quantize_rows(ks)
    av, sv = lc.fp8_quantize_rows(vs)
    Bmax = max(GROUP_BRANCHES)
    qs = [rnd(1, 1, HQ * D).view(1, 1, HQ, D).transpose(1, 2) for _ in range(Bmax)]
    owns = [(rnd(1, HKV, GROUP_OWN + 256, D)[:, :, :GROUP_OWN], rnd(1, HKV, GROUP_OWN + 256, D)[:, :, :GROUP_OWN]) for _ in range(Bmax)]
    rows = []
    for kind in ("shared16", "fp8_archive"):
        if kind == "shared16":
            s16 = (nv.ptr(ks), nv.ptr(vs), GROUP_SHARED, ks.stride(1), ks.stride(2))
            a8 = (None, None, None, None, 0, 0, 0)
            shared_bytes = 2 * HKV * GROUP_SHARED * D * 2
        else:
            s16 = (None, None, 0, 0, 0)
            a8 = (nv.ptr(ak), nv.ptr(av), nv.ptr(sk), nv.ptr(sv), GROUP_SHARED, ak.stride(1), sk.stride(1))
            shared_bytes = 2 * HKV * GROUP_SHARED * (D + 4)
        for B in GROUP_BRANCHES:
            brs, own_rows = (nv.DecodeBranch * B)(), (C.c_int * B)(*([GROUP_OWN] * B))
            for b in range(B):
                br, (k, v) = brs[b], owns[b]
                br.q, br.q_stride_h, br.k, br.v = qs[b].data_ptr(), qs[b].stride(1), k.data_ptr(), v.data_ptr()
                br.kv_stride_h, br.kv_stride_l, br.Lk = k.stride(1), k.stride(2), GROUP_OWN
            need_g = nv.lib.rtk_attention_decode_group_workspace_bytes(own_rows, B, HQ, HKV, a8[4], s16[2], D, code)
            need_s = nv.lib.rtk_attention_decode_workspace_bytes_shared(HQ, HKV, 1, GROUP_OWN, a8[4], s16[2], D, code)
            ws_g = torch.empty(max(need_g, 16), dtype=torch.uint8, device=dev)
            ws_s = torch.empty(max(need_s, 16), dtype=torch.uint8, device=dev)
            out_g = torch.empty((B, 1, HQ, D), dtype=dtype, device=dev)
            out_s = torch.empty((B, 1, HQ, D), dtype=dtype, device=dev)
            succ = [(nv.ptr(qs[b]), qs[b].stride(1), qs[b].stride(2), nv.ptr(owns[b][0]), nv.ptr(owns[b][1]), owns[b][0].stride(1),
                     owns[b][0].stride(2)) + s16 + a8 + (nv.ptr(out_s[b]), HQ, HKV, 1, GROUP_OWN, GROUP_OWN - 1, D, code, scale,
                                                          nv.ptr(ws_s), need_s, stream) for b in range(B)]

            def group():
                for _ in range(DECODE_INNER):
                    nv.check(nv.lib.rtk_attention_decode_group(brs, B, *s16, *a8, nv.ptr(out_g), HQ, HKV, D, code, scale,
                                                               nv.ptr(ws_g), need_g, stream), "rtk_attention_decode_group")

            def successive():
                for _ in range(DECODE_INNER):
                    for a in succ:
                        nv.check(nv.lib.rtk_attention_decode_shared(*a), "rtk_attention_decode_shared")

            for _ in range(args.warmup):
                group()
                successive()
            torch.cuda.synchronize()
            times = {"group": [], "successive": []}
            for _ in range(args.reps):   # interleaved: both routes see the same drift of clocks and cache state
                for name, fn in (("group", group), ("successive", successive)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / DECODE_INNER)
            row = {"kind": kind, "B": B, "Hq": HQ, "Hkv": HKV, "D": D, "dtype": "bfloat16", "shared_rows": GROUP_SHARED,
                   "own_rows": GROUP_OWN, "reps": args.reps, "inner": DECODE_INNER, "shared_bytes": shared_bytes}
            for name, t in times.items():
                us = statistics.median(t)
                row[name] = {"us": us, "min_us": min(t), "max_us": max(t), "ms_per_token": us * LAYERS * 1e-3}
            row["group"]["fraction_of_8_TBps"] = shared_bytes / (row["group"]["us"] * 1e-6) / HBM_PEAK
            row["ratio_successive_over_group"] = row["successive"]["us"] / row["group"]["us"]
            row["max_abs_diff_group_vs_successive"] = (out_g.float() - out_s.float()).abs().max().item()
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("\n| shared rows as | B | group call us | B successive calls us | successive / group | shared MB | group: of 8 TB/s "
          "| group ms / token |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['kind']} | {r['B']} | {r['group']['us']:.1f} | {r['successive']['us']:.1f} | "
              f"{r['ratio_successive_over_group']:.2f} | {r['shared_bytes'] / 1e6:.1f} | {r['group']['fraction_of_8_TBps']:.3f} | "
              f"{r['group']['ms_per_token']:.2f} |")


WIDE_ROWS, WIDE_OWN, WIDE_LQS = 100352, 64, (3, 6, 9)
# the other geometries the envelope admits, over plain rows: (Hq, Hkv, Lq) - G = 8, 4 (NCG 2, 3, 4), 2, 1 (17 and 64 rows), 16
WIDE_OTHER = [(32, 4, 8), (16, 4, 5), (16, 4, 10), (16, 4, 16), (8, 4, 32), (8, 8, 17), (8, 8, 64), (16, 1, 4)]


def main_wide(args):
    import retake._native as nv
    import retake.longvideo_cache as lc

    dev = torch.device("cuda:0")
    dtype, code, scale, stream = torch.bfloat16, nv.RTK_BF16, D ** -0.5, nv.stream()
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: (1.7 * torch.randn(shape, generator=g, device=dev)).to(dtype)   # noqa: E731

    def keys(kind, hkv):
        """entry-point suffix, own rows, the segment arguments, the segment shape, K/V bytes a call reads once, keep-alive"""
        kb, vb = rnd(1, hkv, WIDE_ROWS + 256, D), rnd(1, hkv, WIDE_ROWS + 256, D)      # plain rows of a cache buffer
        ks, vs = kb[:, :, :WIDE_ROWS], vb[:, :, :WIDE_ROWS]                            # ... or another buffer's shared rows
        if kind == "plain":
            return "", (ks, vs), (), (), 2 * hkv * WIDE_ROWS * D * 2, ()
        ko, vo = rnd(1, hkv, WIDE_OWN + 256, D)[:, :, :WIDE_OWN], rnd(1, hkv, WIDE_OWN + 256, D)[:, :, :WIDE_OWN]
        if kind == "shared16":
            s16 = (nv.ptr(ks), nv.ptr(vs), WIDE_ROWS, ks.stride(1), ks.stride(2))
            return ("_shared", (ko, vo), s16 + (None, None, None, None, 0, 0, 0), (0, WIDE_ROWS),
                    2 * hkv * (WIDE_ROWS + WIDE_OWN) * D * 2, (ks, vs))
        ak, sk = lc.fp8_quantize_rows(ks.contiguous())
        av, sv = lc.fp8_quantize_rows(vs.contiguous())
        a8 = (nv.ptr(ak), nv.ptr(av), nv.ptr(sk), nv.ptr(sv), WIDE_ROWS, ak.stride(1), sk.stride(1))
        return "_fp8kv", (ko, vo), a8, (WIDE_ROWS,), 2 * hkv * (WIDE_ROWS * (D + 4) + WIDE_OWN * D * 2), (ak, av, sk, sv)

    cases = [(kind, HQ, HKV, WIDE_LQS) for kind in ("plain", "shared16", "fp8_archive")] + \
            [("plain", hq, hkv, (lq,)) for hq, hkv, lq in WIDE_OTHER]
    rows = []
    for kind, hq, hkv, lqs in cases:
        sfx, (k, v), segs, seg_shape, kv_bytes, _alive = keys(kind, hkv)
        Lk = k.shape[2]
        for Lq in lqs:
            q = rnd(1, Lq, hq * D).view(1, Lq, hq, D).transpose(1, 2)

            def direct(fn, n, query=None):
                """DECODE_INNER back-to-back calls of one entry point on the first n query rows; resident output, workspace."""
                qn = q[:, :, :n]
                need = getattr(nv.lib, (query or fn + "_workspace_bytes") + sfx)(hq, hkv, n, Lk, *seg_shape, D, code)
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)   # (0: the chunk kernel needs no split here)
                out = torch.empty((1, n, hq, D), dtype=dtype, device=dev)
                call = getattr(nv.lib, fn + sfx)
                a = (nv.ptr(qn), qn.stride(1), qn.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2)) + tuple(segs) + \
                    (nv.ptr(out), hq, hkv, n, Lk, Lk - n, D, code, scale, nv.ptr(ws), need, stream)

                def run():
                    for _ in range(DECODE_INNER):
                        nv.check(call(*a), fn + sfx)
                return run, out

            routes = {"wide": direct("rtk_attention_decode_wide", Lq),
                      "replaced": direct("rtk_attention_forward", Lq, "rtk_attention_workspace_bytes"),
                      "packed_lq1": direct("rtk_attention_decode", 1)}
            for _ in range(args.warmup):
                for run, _o in routes.values():
                    run()
            torch.cuda.synchronize()
            times = {name: [] for name in routes}
            for _ in range(args.reps):   # interleaved: the routes see the same drift of clocks and cache state
                for name, (run, _o) in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / DECODE_INNER)
            row = {"kind": kind, "Lq": Lq, "packed_rows": hq // hkv * Lq, "Hq": hq, "Hkv": hkv, "D": D, "dtype": "bfloat16",
                   "rows": WIDE_ROWS, "own_rows": Lk if kind != "plain" else 0, "reps": args.reps, "inner": DECODE_INNER,
                   "kv_bytes": kv_bytes}
            for name, t in times.items():
                q1, med, q3 = statistics.quantiles(t, n=4)
                row[name] = {"us": med, "q1_us": q1, "q3_us": q3, "iqr_us": q3 - q1, "min_us": min(t), "max_us": max(t)}
            w, r = row["wide"], row["replaced"]
            w["fraction_of_8_TBps"] = kv_bytes / (w["us"] * 1e-6) / HBM_PEAK
            w["ms_per_step"] = w["us"] * LAYERS * 1e-3
            r["ms_per_step"] = r["us"] * LAYERS * 1e-3
            row["ratio_replaced_over_wide"] = r["us"] / w["us"]
            row["ratio_wide_over_packed_lq1"] = w["us"] / row["packed_lq1"]["us"]
            row["faster_beyond_iqr"] = bool(r["us"] - w["us"] > r["iqr_us"] + w["iqr_us"])
            row["max_abs_diff_wide_vs_replaced"] = (routes["wide"][1].float() - routes["replaced"][1].float()).abs().max().item()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del routes
        del k, v, segs, _alive
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("\n| keys as | Hq / Hkv | Lq | packed rows | wide us (q1 - q3) | replaced chunk call us (q1 - q3) | replaced / wide | packed Lq 1 us "
          "| wide / packed Lq 1 | K/V MB | wide: of 8 TB/s | faster beyond the IQRs |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        w, c, p = r["wide"], r["replaced"], r["packed_lq1"]
        print(f"| {r['kind']} | {r['Hq']} / {r['Hkv']} | {r['Lq']} | {r['packed_rows']} | {w['us']:.1f} ({w['q1_us']:.1f} - {w['q3_us']:.1f}) | "
              f"{c['us']:.1f} ({c['q1_us']:.1f} - {c['q3_us']:.1f}) | {r['ratio_replaced_over_wide']:.2f} | {p['us']:.1f} | "
              f"{r['ratio_wide_over_packed_lq1']:.2f} | {r['kv_bytes'] / 1e6:.1f} | {w['fraction_of_8_TBps']:.3f} | "
              f"{r['faster_beyond_iqr']} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp8kv", action="store_true", help="the two-segment fp8 call against the 16-bit kernel on dequantised rows")
    ap.add_argument("--decode", action="store_true", help="the GQA-packed few-row kernel against the call it replaces")
    ap.add_argument("--group", action="store_true", help="one group-decode call against the B successive per-branch calls it replaces")
    ap.add_argument("--wide", action="store_true", help="the wide packed kernel against the chunk-kernel call it replaces")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", choices=("chunk", "all"), default="all")
    ap.add_argument("--routes", default="native,sdpa,fa2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention.py needs the GPU: a CPU run measures nothing")
    if args.wide:
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "wide_decode_bench.json")
        return main_wide(args)
    if args.out is None and not args.group:
        args.out = os.path.join(ROOT, "profiles", ("fp8kv_" if args.fp8kv else "") + ("decode_" if args.decode else "") +
                                "attention_bench.json")
    if args.group:
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "group_decode_bench.json")
        return main_group(args)
    if args.decode:
        return main_decode(args)
    if args.fp8kv:
        return main_fp8kv(args)
    import retake.longvideo_cache as lc

    try:
        import flash_attn  # noqa: F401
        from transformers.modeling_flash_attention_utils import _flash_attention_forward
    except Exception:  # noqa: BLE001
        _flash_attention_forward = None

    dev = torch.device("cuda:0")
    G = HQ // HKV
    cases = [(s, torch.bfloat16, "chunk") for s in CHUNK_SHAPES] + [(CHUNK_SHAPES[1], torch.float16, "chunk")]
    if args.shapes == "all":
        cases += [(s, torch.bfloat16, "few rows") for s in FEW_ROW_SHAPES]
    rows = []
    for (Lq, P0), dtype, kind in cases:
        q, k, v, mask = make(Lq, P0, dtype, dev)
        ws = {}

        def native():
            return lc.chunk_attention(q, k, v, workspace=ws)

        def sdpa():
            kk, vv = lc.repeat_kv(k, G), lc.repeat_kv(v, G)
            qc, kc, vc = (t.contiguous() for t in (q, kk, vv))
            o = torch.nn.functional.scaled_dot_product_attention(qc, kc, vc, attn_mask=mask, dropout_p=0.0, is_causal=False)
            return o.transpose(1, 2).contiguous()

        def fa2():
            kk, vv = lc.repeat_kv(k, G), lc.repeat_kv(v, G)
            return _flash_attention_forward(q.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2), None, Lq, is_causal=True)

        row = {"Lq": Lq, "P0": P0, "Lk": P0 + Lq, "Hq": HQ, "Hkv": HKV, "D": D, "dtype": str(dtype)[6:], "kind": kind,
               "flop": flop(Lq, P0), "reps": args.reps}
        outs = {}
        for name, fn in (("native", native), ("sdpa", sdpa), ("fa2", fa2)):
            if name not in args.routes.split(","):
                row[name] = {"status": "not requested"}
                continue
            if name == "fa2" and _flash_attention_forward is None:
                row["fa2"] = {"status": "flash_attn package not installed"}
                continue
            try:
                us, peak, out = timed(fn, args.reps, args.warmup)
                row[name] = {"status": "ok", "us": us, "fraction_of_2.5_PFLOPs": row["flop"] / (us * 1e-6) / PEAK_FLOPS,
                             "tflops": row["flop"] / (us * 1e-6) / 1e12, "allocator_peak_bytes": int(peak)}
                outs[name] = out
            except torch.cuda.OutOfMemoryError as e:   # recorded, not skipped
                row[name] = {"status": "out of memory", "error": str(e).split("\n")[0][:200]}
            torch.cuda.empty_cache()
        if "native" in outs and "sdpa" in outs:
            row["max_abs_diff_native_vs_sdpa"] = (outs["native"].float() - outs["sdpa"].float()).abs().max().item()
        if row["native"]["status"] == "ok" and row["sdpa"]["status"] == "ok":
            row["ratio_sdpa_over_native"] = row["sdpa"]["us"] / row["native"]["us"]
        rows.append(row)
        del q, k, v, mask, outs, ws
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "peak_flops": PEAK_FLOPS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("\n| dtype | Lq | P0 | native us | of 2.5 PF/s | native peak MiB | SDPA route us | SDPA peak MiB | SDPA / native |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        n, s = r["native"], r["sdpa"]
        if n["status"] != "ok":
            continue
        s_us = f"{s['us']:.0f}" if s["status"] == "ok" else s["status"]
        s_pk = f"{s['allocator_peak_bytes'] / 2**20:.0f}" if s["status"] == "ok" else "-"
        ratio = f"{r['ratio_sdpa_over_native']:.2f}" if "ratio_sdpa_over_native" in r else "-"
        print(f"| {r['dtype']} | {r['Lq']} | {r['P0']} | {n['us']:.0f} | {n['fraction_of_2.5_PFLOPs']:.3f} | "
              f"{n['allocator_peak_bytes'] / 2**20:.0f} | {s_us} | {s_pk} | {ratio} |")


if __name__ == "__main__":
    main()

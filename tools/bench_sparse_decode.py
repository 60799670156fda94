#!/usr/bin/env python
"""The page-sparse decode (retake/_sparse_decode.py, rtk_attention_decode_sparse) at the headline geometry, beside what it
has to be weighed against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED (so that all see
the same drift of clocks and the same neighbours), medians of `reps` with quartiles.

    python tools/bench_sparse_decode.py [--out profiles/sparse_decode_bench.json] [--reps 15] [--warmup 3] [--parent-lib PATH]

28 layers, Hq 28 / Hkv 4 / D 128, bf16, n = 100 352 region rows per layer behind 37 pinned rows, 64 tail rows; one layer's
call, one query row per head; keep_rows 4 096 / 8 192 / 16 384:
  decode_full        rtk_attention_decode over ALL rows of the layer: the call the sparse chain replaces.  With
                     --parent-lib it is taken from that library (the parent commit's build), else from this build's
                     (tools/kernel_diff.py: the kernel compiles to the same code);
  sparse_K           the whole chain, rtk_attention_decode_sparse: bound, selection, paged attention, combine;
  bound              its first launch alone (rtk_attention_page_bound over the layer's 3 136 pages);
  select_K           its second (rtk_pivotkv_budget_select_batched, one unit per kv head);
  paged_K            its third and fourth (rtk_attention_decode_paged with the chain's lists: paged kernel + combine);
  focused_K          the packed call over a focused cache of the same keep_rows (PivotKVCache.focus): pinned + K + tail rows;
  summary_build      rtk_pivotkv_page_summary_batched over the 28 layers: what arming costs;
  copy_k_bytes       rtk_profile_copy of the K bytes the summary build reads (what a plain copy of them costs).
One JSON document; a summary on stdout.  Needs the GPU: there is no other way to get a time.

    python tools/bench_sparse_decode.py --fp8 [--out profiles/sparse_decode_fp8_bench.json] [--parent-lib PATH]

The same over an fp8 archive (sparse_decode(cache, archive=True), rtk_attention_decode_sparse_fp8kv): 28 layers x 100 352
archive rows, 37 pinned + 64 tail 16-bit rows, the buffers filled directly (layer 0: quantised random rows; the other layers,
which only the summary build reads: random finite codes):
  fp8_full           (a) rtk_attention_decode_fp8kv over the full archive - from --parent-lib (the parent commit's build) when
                     given: the call the chain replaces;
  sparse8_K          the whole chain, rtk_attention_decode_sparse_fp8kv;
  gathered8_K        (b) rtk_attention_decode_fp8kv over a gathered archive of K rows: what a focused fp8 cache pays per token;
  sparse16_K         (c) the 16-bit chain, rtk_attention_decode_sparse, on the dequantised rows;
  summary_build8     rtk_pivotkv_page_summary_fp8k_batched over the 28 layers: what arming costs;
  copy_k_code_bytes  rtk_profile_copy of the K codes' bytes."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import retake._native as nv  # noqa: E402
import retake._sparse_decode as sd  # noqa: E402
from bench_focus import D, Hkv, Hq, KEEPS, LAYERS, N, PINNED, QUESTION, arm, parent, stat  # noqa: E402
from retake.native_attention import chunk_attention  # noqa: E402

PAGES = N // 32


def main_fp8(args):
    from retake.native_attention import fp8_dequantize_rows, fp8_quantize_rows

    dev = torch.device("cuda:0")
    stream = nv.stream()
    g = torch.Generator(device=dev).manual_seed(7)
    Lk = PINNED + QUESTION   # the 16-bit rows: pinned, then everything behind the video
    bf, code, scale = torch.bfloat16, nv.RTK_BF16, D ** -0.5
    rnd = lambda *shape: (1.7 * torch.randn(shape, generator=g, device=dev)).to(bf)   # noqa: E731
    q1, k16, v16 = rnd(1, Hq, 1, D), rnd(1, Hkv, Lk, D), rnd(1, Hkv, Lk, D)
    k8, ks = fp8_quantize_rows(rnd(1, Hkv, N, D))
    v8, vs = fp8_quantize_rows(rnd(1, Hkv, N, D))
    out = torch.empty((1, 1, Hq, D), dtype=bf, device=dev)
    q3 = (nv.ptr(q1), q1.stride(1), q1.stride(2))

    def fp8kv_args(k8, v8, ks, vs):
        return q3 + (nv.ptr(k16), nv.ptr(v16), k16.stride(1), k16.stride(2), nv.ptr(k8), nv.ptr(v8), nv.ptr(ks), nv.ptr(vs),
                     k8.shape[2], k8.stride(1), ks.stride(1), nv.ptr(out), Hq, Hkv, 1, Lk, Lk - 1, D, code, scale)

    # ---- (a) the call the chain replaces: from the parent commit's library when given -----------------------------------
    full_lib = nv.lib
    if args.parent_lib:
        full_lib = C.CDLL(args.parent_lib)
        for name in ("rtk_attention_decode_fp8kv", "rtk_attention_decode_workspace_bytes_fp8kv"):
            fn = getattr(full_lib, name)
            fn.restype, fn.argtypes = nv._SIGNATURES[name]
    need_full = full_lib.rtk_attention_decode_workspace_bytes_fp8kv(Hq, Hkv, 1, Lk, N, D, code)
    ws_full = torch.empty(need_full, dtype=torch.uint8, device=dev)
    full_args = fp8kv_args(k8, v8, ks, vs)

    def run_full(_):
        nv.check(full_lib.rtk_attention_decode_fp8kv(*full_args, nv.ptr(ws_full), need_full, stream), "rtk_attention_decode_fp8kv")

    # ---- the index over the K codes of every layer, and a plain copy of those bytes --------------------------------------
    codes = [k8] + [(torch.randint(0, 127, (1, Hkv, N, D), generator=g, device=dev, dtype=torch.uint8)
                     | (torch.randint(0, 2, (1, Hkv, N, D), generator=g, device=dev, dtype=torch.uint8) << 7)) for _ in range(LAYERS - 1)]
    scales = [ks] + [torch.full((1, Hkv, N), 2.0 ** -6, dtype=torch.float32, device=dev) for _ in range(LAYERS - 1)]
    summs = [torch.empty((Hkv, PAGES, 2, D), dtype=bf, device=dev) for _ in range(LAYERS)]
    units = (nv.PageSummaryFp8kUnit * LAYERS)()
    for u, c8, s8, sm in zip(units, codes, scales, summs):
        u.k8, u.k8_stride_h, u.k_scale, u.scale_stride_h, u.n = c8.data_ptr(), c8.stride(1), s8.data_ptr(), s8.stride(1), N
        u.summ, u.summ_stride_h = sm.data_ptr(), sm.stride(0)

    def run_summary(_):
        nv.check(nv.lib.rtk_pivotkv_page_summary_fp8k_batched(units, LAYERS, Hkv, D, code, stream), "rtk_pivotkv_page_summary_fp8k_batched")

    run_summary(0)
    summ = summs[0]
    code_bytes = LAYERS * Hkv * N * D
    csrc = torch.zeros(code_bytes, dtype=torch.uint8, device=dev)
    cdst = torch.empty_like(csrc)

    def run_copy(_):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(cdst), nv.ptr(csrc), code_bytes, stream), "rtk_profile_copy")

    # ---- the chain ---------------------------------------------------------------------------------------------------------
    keep_pages = {K: min(-(-K // 32), PAGES) for K in KEEPS}
    need = {K: nv.lib.rtk_attention_decode_sparse_fp8kv_workspace_bytes(Hq, Hkv, 1, Lk, N, keep_pages[K], D, code) for K in KEEPS}
    ws = {K: torch.empty(need[K], dtype=torch.uint8, device=dev) for K in KEEPS}

    def run_sparse8(K):
        nv.check(nv.lib.rtk_attention_decode_sparse_fp8kv(*full_args, nv.ptr(summ), summ.stride(0), keep_pages[K], nv.ptr(ws[K]),
                                                          need[K], stream), "rtk_attention_decode_sparse_fp8kv")

    # ---- (b) the packed fp8 call over a gathered archive of keep_rows rows ------------------------------------------------
    gathered, need_g, ws_g = {}, {}, {}
    for K in KEEPS:
        idx = torch.randperm(N, generator=g, device=dev)[:K].sort().values
        a = tuple(t.index_select(2, idx).contiguous() for t in (k8, v8, ks, vs))
        gathered[K] = fp8kv_args(*a) + (a,)   # (the tensors are kept alive beside their pointers)
        need_g[K] = nv.lib.rtk_attention_decode_workspace_bytes_fp8kv(Hq, Hkv, 1, Lk, K, D, code)
        ws_g[K] = torch.empty(need_g[K], dtype=torch.uint8, device=dev)

    def run_gathered8(K):
        nv.check(nv.lib.rtk_attention_decode_fp8kv(*gathered[K][:-1], nv.ptr(ws_g[K]), need_g[K], stream), "rtk_attention_decode_fp8kv")

    # ---- (c) the 16-bit chain on the dequantised rows: [pinned | dequantised archive | tail] in one buffer -----------------
    ve, L16 = PINNED + N, PINNED + N + QUESTION
    kd = torch.cat([k16[:, :, :PINNED], fp8_dequantize_rows(k8, ks, bf), k16[:, :, PINNED:]], dim=2).contiguous()
    vd = torch.cat([v16[:, :, :PINNED], fp8_dequantize_rows(v8, vs, bf), v16[:, :, PINNED:]], dim=2).contiguous()
    summ16 = torch.empty((Hkv, PAGES, 2, D), dtype=bf, device=dev)
    u16 = (nv.PageSummaryUnit * 1)()
    u16[0].k, u16[0].k_stride_h, u16[0].first, u16[0].n = kd.data_ptr(), kd.stride(1), PINNED, N
    u16[0].summ, u16[0].summ_stride_h = summ16.data_ptr(), summ16.stride(0)
    nv.check(nv.lib.rtk_pivotkv_page_summary_batched(u16, 1, Hkv, D, code, stream), "rtk_pivotkv_page_summary_batched")
    need16 = {K: nv.lib.rtk_attention_decode_sparse_workspace_bytes(Hq, Hkv, 1, L16, PINNED, ve, keep_pages[K], D, code) for K in KEEPS}
    ws16 = {K: torch.empty(need16[K], dtype=torch.uint8, device=dev) for K in KEEPS}

    def run_sparse16(K):
        nv.check(nv.lib.rtk_attention_decode_sparse(*q3, nv.ptr(kd), nv.ptr(vd), kd.stride(1), kd.stride(2), nv.ptr(out), Hq, Hkv, 1,
                                                    L16, L16 - 1, D, code, scale, PINNED, ve, nv.ptr(summ16), summ16.stride(0),
                                                    keep_pages[K], nv.ptr(ws16[K]), need16[K], stream), "rtk_attention_decode_sparse")

    work = [("fp8_full", run_full, 0), ("summary_build8", run_summary, 0), ("copy_k_code_bytes", run_copy, 0)]
    for K in KEEPS:
        work += [(f"sparse8_{K}", run_sparse8, K), (f"gathered8_{K}", run_gathered8, K), (f"sparse16_{K}", run_sparse16, K)]
    samples = {name: [] for name, _, _ in work}
    for rep in range(args.warmup + args.reps):
        for name, fn, arg in work:               # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "archive_rows": N, "pages": PAGES,
                           "pinned": PINNED, "tail": QUESTION, "keep_rows": list(KEEPS), "k_code_bytes": code_bytes,
                           "summary_bytes": LAYERS * Hkv * PAGES * 2 * D * 2},
              "fp8_full_from": "parent commit's library" if args.parent_lib else "this build (same kernel code as the parent's)",
              "method": f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up "
                        "rounds; one layer's call, one query row per head"}
    for name in samples:
        report[name] = stat(samples[name])
    iqr = lambda r: r["q3_us"] - r["q1_us"]   # noqa: E731
    for K in KEEPS:
        r, full = report[f"sparse8_{K}"], report["fp8_full"]
        r.update(full_over_sparse=round(full["median_us"] / r["median_us"], 2),
                 sparse_over_gathered=round(r["median_us"] / report[f"gathered8_{K}"]["median_us"], 2),
                 sparse_over_16bit_chain=round(r["median_us"] / report[f"sparse16_{K}"]["median_us"], 2),
                 beats_full_by_more_than_both_iqrs=bool(full["median_us"] - r["median_us"] > max(iqr(full), iqr(r))))
    report["summary_build8"]["time_over_copy"] = round(report["summary_build8"]["median_us"] / report["copy_k_code_bytes"]["median_us"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name in samples:
        print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    for K in KEEPS:
        r = report[f"sparse8_{K}"]
        print(f"keep_rows {K}: the full fp8 call {r['full_over_sparse']:.2f} x the chain; the chain {r['sparse_over_gathered']:.2f} x the "
              f"call over a gathered archive, {r['sparse_over_16bit_chain']:.2f} x the 16-bit chain")
    print(f"summary build {report['summary_build8']['time_over_copy']:.2f} x the plain copy of the K codes' bytes")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default: profiles/sparse_decode_bench.json (--fp8: sparse_decode_fp8_bench.json)")
    ap.add_argument("--fp8", action="store_true", help="the chain over an fp8 archive (rtk_attention_decode_sparse_fp8kv)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libretake_hip.so of the parent commit: decode_full is taken from it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_decode.py measures on the GPU; none is visible (Time: not measured)")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sparse_decode_fp8_bench.json" if args.fp8 else "sparse_decode_bench.json")
    if args.fp8:
        return main_fp8(args)
    dev = torch.device("cuda:0")
    stream = nv.stream()
    g = torch.Generator(device=dev).manual_seed(7)
    cache = parent(dev, g)
    st = cache._layers[0]
    ve, Lk = PINNED + N, PINNED + N + QUESTION
    q1 = (1.7 * torch.randn((1, Hq, 1, D), generator=g, device=dev)).bfloat16()
    k, v = st._k[:, :, :Lk], st._v[:, :, :Lk]
    qkv = (nv.ptr(q1), q1.stride(1), q1.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2))
    out = torch.empty((1, 1, Hq, D), dtype=torch.bfloat16, device=dev)
    scale = D ** -0.5

    # ---- the call the chain replaces: from the parent commit's library when given --------------------------------------
    full_lib = nv.lib
    if args.parent_lib:
        full_lib = C.CDLL(args.parent_lib)
        for name in ("rtk_attention_decode", "rtk_attention_decode_workspace_bytes"):
            fn = getattr(full_lib, name)
            fn.restype, fn.argtypes = nv._SIGNATURES[name]
    need_full = full_lib.rtk_attention_decode_workspace_bytes(Hq, Hkv, 1, Lk, D, nv.RTK_BF16)
    ws_full = torch.empty(need_full, dtype=torch.uint8, device=dev)

    def run_full(_):
        nv.check(full_lib.rtk_attention_decode(*qkv, nv.ptr(out), Hq, Hkv, 1, Lk, Lk - 1, D, nv.RTK_BF16, scale, nv.ptr(ws_full),
                                               need_full, stream), "rtk_attention_decode")

    # ---- the index, the chain and its launches alone -------------------------------------------------------------------
    sd.sparse_decode(cache, max(KEEPS))
    summs = dict(cache._sparse.summ)   # (kept alive here: dense_decode below frees the cache's references)
    summ = summs[0]
    keep_pages = {K: min(-(-K // 32), PAGES) for K in KEEPS}
    need = {K: nv.lib.rtk_attention_decode_sparse_workspace_bytes(Hq, Hkv, 1, Lk, PINNED, ve, keep_pages[K], D, nv.RTK_BF16)
            for K in KEEPS}
    ws = {K: torch.empty(need[K], dtype=torch.uint8, device=dev) for K in KEEPS}

    def run_sparse(K):
        nv.check(nv.lib.rtk_attention_decode_sparse(*qkv, nv.ptr(out), Hq, Hkv, 1, Lk, Lk - 1, D, nv.RTK_BF16, scale, PINNED, ve,
                                                    nv.ptr(summ), summ.stride(0), keep_pages[K], nv.ptr(ws[K]), need[K], stream),
                 "rtk_attention_decode_sparse")

    ub = torch.empty((Hkv, PAGES), dtype=torch.float32, device=dev)

    def run_bound(_):
        nv.check(nv.lib.rtk_attention_page_bound(nv.ptr(q1), q1.stride(1), q1.stride(2), nv.ptr(summ), summ.stride(0), Hq, Hkv, 1,
                                                 PAGES, D, nv.RTK_BF16, nv.ptr(ub), stream), "rtk_attention_page_bound")

    run_bound(0)
    lists = {K: torch.empty((Hkv, keep_pages[K]), dtype=torch.int32, device=dev) for K in KEEPS}
    s_units = {K: (nv.BudgetSelectUnit * Hkv)(*[nv.BudgetSelectUnit(ub[h].data_ptr(), lists[K][h].data_ptr(), PAGES, keep_pages[K])
                                                for h in range(Hkv)]) for K in KEEPS}

    def run_select(K):
        nv.check(nv.lib.rtk_pivotkv_budget_select_batched(s_units[K], Hkv, stream), "rtk_pivotkv_budget_select_batched")

    need_p = {K: nv.lib.rtk_attention_decode_paged_workspace_bytes(Hq, Hkv, 1, Lk, PINNED, ve, keep_pages[K], D, nv.RTK_BF16)
              for K in KEEPS}
    ws_p = {K: torch.empty(need_p[K], dtype=torch.uint8, device=dev) for K in KEEPS}

    def run_paged(K):
        nv.check(nv.lib.rtk_attention_decode_paged(*qkv, nv.ptr(out), Hq, Hkv, 1, Lk, Lk - 1, D, nv.RTK_BF16, scale, PINNED, ve,
                                                   nv.ptr(lists[K]), keep_pages[K], nv.ptr(ws_p[K]), need_p[K], stream),
                 "rtk_attention_decode_paged")

    for K in KEEPS:
        run_select(K)

    # ---- the summary build and a plain copy of the K bytes it reads -----------------------------------------------------
    units = (nv.PageSummaryUnit * LAYERS)()
    for l, (u, s) in enumerate(zip(units, cache._layers)):
        sm = summs[l]
        u.k, u.k_stride_h, u.first, u.n, u.summ, u.summ_stride_h = s._k.data_ptr(), s._k.stride(1), PINNED, N, sm.data_ptr(), sm.stride(0)

    def run_summary(_):
        nv.check(nv.lib.rtk_pivotkv_page_summary_batched(units, LAYERS, Hkv, D, nv.RTK_BF16, stream), "rtk_pivotkv_page_summary_batched")

    k_bytes = LAYERS * Hkv * N * D * 2
    csrc = torch.zeros(k_bytes, dtype=torch.uint8, device=dev)
    cdst = torch.empty_like(csrc)

    def run_copy(_):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(cdst), nv.ptr(csrc), k_bytes, stream), "rtk_profile_copy")

    # ---- the packed call over a focused cache of the same keep_rows -----------------------------------------------------
    queries = [(1.7 * torch.randn((Hq, 64, D), generator=g, device=dev)).bfloat16() for _ in range(LAYERS)]
    sd.dense_decode(cache)
    arm(cache, 64, queries)
    small, fws, route = {}, {}, []
    for K in KEEPS:
        fc = cache.focus(K)
        s0 = fc._layers[0]
        small[K] = (s0._k[:, :, :s0.length].clone(), s0._v[:, :, :s0.length].clone())   # one layer's rows: the caches are freed
        del fc
    cache.unwatch_question()

    def run_focused(K):
        assert chunk_attention(q1, *small[K], workspace=fws, packed_gqa=True, route=route) is not None

    run_focused(KEEPS[0])
    assert route == ["packed"], route

    work = [("decode_full", run_full, 0), ("bound", run_bound, 0), ("summary_build", run_summary, 0), ("copy_k_bytes", run_copy, 0)]
    for K in KEEPS:
        work += [(f"sparse_{K}", run_sparse, K), (f"select_{K}", run_select, K), (f"paged_{K}", run_paged, K),
                 (f"focused_{K}", run_focused, K)]
    samples = {name: [] for name, _, _ in work}
    for rep in range(args.warmup + args.reps):
        for name, fn, arg in work:               # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "n": N, "pages": PAGES, "pinned": PINNED,
                           "tail": QUESTION, "keep_rows": list(KEEPS), "k_bytes": k_bytes,
                           "summary_bytes": LAYERS * Hkv * PAGES * 2 * D * 2},
              "decode_full_from": "parent commit's library" if args.parent_lib else "this build (same kernel code as the parent's)",
              "method": f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up "
                        "rounds; one layer's call, one query row per head; the launches alone run on the chain's own operands"}
    for name in samples:
        report[name] = stat(samples[name])
    for K in KEEPS:
        report[f"sparse_{K}"].update(
            full_over_sparse=round(report["decode_full"]["median_us"] / report[f"sparse_{K}"]["median_us"], 2),
            sparse_over_focused=round(report[f"sparse_{K}"]["median_us"] / report[f"focused_{K}"]["median_us"], 2))
    report["summary_build"]["time_over_copy"] = round(report["summary_build"]["median_us"] / report["copy_k_bytes"]["median_us"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name in samples:
        print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    for K in KEEPS:
        r = report[f"sparse_{K}"]
        print(f"keep_rows {K}: the full call {r['full_over_sparse']:.2f} x the sparse chain, the chain {r['sparse_over_focused']:.2f} x "
              "the call over a focused cache")
    print(f"summary build {report['summary_build']['time_over_copy']:.2f} x the plain copy of K's bytes")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The question-focused decode cache (PivotKVCache.watch_question / focus, rtk_pivotkv_focus_gather_batched) at the headline
geometry, beside what it has to be weighed against - all in ONE process, HIP events, the samples of every measurement
INTERLEAVED (so that all see the same drift of clocks and the same neighbours), medians of `reps` with quartiles.

    python tools/bench_focus.py [--out profiles/focus_bench.json] [--reps 15] [--warmup 3]

28 layers, Hq 28 / Hkv 4 / D 128, bf16, n = 100 352 region rows per layer behind 37 pinned rows, a question of 64 rows behind
them; keep_rows 4 096 / 8 192 / 16 384, watch rows 16 / 64:
  focus_K_W                the whole `cache.focus(K)` of a parent armed with W rows: host work, allocations and its three calls;
  rescore_W                its first call alone: rtk_pivotkv_rescore_batched with alpha = 1 into zeroed scores, 28 units;
  select_K                 its second: rtk_pivotkv_budget_select_batched, 28 units;
  gather_K                 its third: rtk_pivotkv_focus_gather_batched, K, V and ids of 28 layers (84 units);
  copy_K                   rtk_profile_copy of the bytes gather_K moves (what a plain copy of them costs);
  index_select_K           the route the gather replaces: per layer and tensor torch.cat([head, index_select, tail]);
  decode_full / decode_K   ONE packed decode-attention call (rtk_attention_decode, one query row per head) over the full
                           pinned + n + question rows of a layer and over its focused rows: what the feature is for.
One JSON document; a summary on stdout.  Needs the GPU: there is no other way to get a time.

    python tools/bench_focus.py --fp8 [--out profiles/focus_fp8_bench.json] [--reps 15] [--warmup 3]

An fp8 parent (kv_cache_dtype="fp8_e4m3" with archive_rescore=True) at the same geometry - the n region rows are the
archive's, the pinned rows and the question lie in the 16-bit buffers:
  focus_K_W                the whole `cache.focus(K)`: rtk_pivotkv_rescore_fp8k_batched, the selection and the gather of codes,
                           scales, ids and 16-bit rows into an fp8 cache of its own;
  decode_full / decode_K   ONE packed decode-attention call (rtk_attention_decode_fp8kv) over a layer's full archive and over
                           the focused one, each in front of the layer's 16-bit rows."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import retake._native as nv  # noqa: E402
import retake.longvideo_cache as lc  # noqa: E402
from retake.native_attention import chunk_attention  # noqa: E402

LAYERS, Hq, Hkv, D, N, PINNED, QUESTION = 28, 28, 4, 128, 100352, 37, 64
KEEPS, WS = (4096, 8192, 16384), (16, 64)


def parent(dev, g):
    """A PivotKVCache whose layers hold PINNED + N + QUESTION random rows with `video_end` behind the first PINNED + N - filled
    directly: a prefill of 10^5 kept rows per layer would take minutes and measure nothing of this."""
    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    cfg = types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq, num_key_value_heads=Hkv,
                                longvideo_kwargs={"kvcache_compression": True, "attention_kernel": "hip",
                                                  "decode_attention": "packed", "kvcache_compression_kwargs": kw})
    cache = lc.build_kvcache(cfg)
    cap = PINNED + N + QUESTION + 64
    for l in range(LAYERS):
        st = cache._store(l)
        k = torch.empty((1, Hkv, cap, D), dtype=torch.bfloat16, device=dev)
        k.normal_(0.0, 1.7, generator=g)
        st.k, st.v = k, torch.empty_like(k).normal_(0.0, 1.0, generator=g)
        st.pos = torch.arange(cap, device=dev).repeat(3, 1).contiguous()
        st.pos_ndim, st.pinned = 3, PINNED
        st.length = st.pos_len = PINNED + N
    cache._pos_layers = LAYERS
    cache.num_evicted_tokens = [0] * LAYERS
    cache.kvcache_compression = False
    cache.last_compressed_mark = cache._take_mark(True)
    for st in cache._layers:
        st.length = st.pos_len = PINNED + N + QUESTION
    return cache


def parent_fp8(dev, g):
    """The same parent with fp8 rows: the N region rows in the archive (random rows quantised by the library's rule), the
    pinned rows and the question in the 16-bit buffers."""
    from retake.native_attention import fp8_quantize_rows

    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    cfg = types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq, num_key_value_heads=Hkv,
                                longvideo_kwargs={"kvcache_compression": True, "attention_kernel": "hip", "kv_cache_dtype": "fp8_e4m3",
                                                  "archive_rescore": True, "decode_attention": "packed",
                                                  "kvcache_compression_kwargs": kw})
    cache = lc.build_kvcache(cfg)
    cap = PINNED + QUESTION + 64
    rows = torch.empty((1, Hkv, N, D), dtype=torch.bfloat16, device=dev)
    for l in range(LAYERS):
        st = cache._store(l)
        st.k = torch.empty((1, Hkv, cap, D), dtype=torch.bfloat16, device=dev).normal_(0.0, 1.7, generator=g)
        st.v = torch.empty((1, Hkv, cap, D), dtype=torch.bfloat16, device=dev).normal_(0.0, 1.0, generator=g)
        st.k8, st.ks8 = fp8_quantize_rows(rows.normal_(0.0, 1.7, generator=g))
        st.v8, st.vs8 = fp8_quantize_rows(rows.normal_(0.0, 1.0, generator=g))
        st.pos = torch.arange(cap + N, device=dev).repeat(3, 1).contiguous()
        st.pos_ndim, st.pinned, st.archive_at, st.len8 = 3, PINNED, PINNED, N
        st.length, st.pos_len = PINNED, PINNED + N
    cache._pos_layers = LAYERS
    cache.num_evicted_tokens = [0] * LAYERS
    cache.kvcache_compression = False
    cache.last_compressed_mark = cache._take_mark(True)
    for st in cache._layers:
        st.length, st.pos_len = PINNED + QUESTION, PINNED + N + QUESTION
    return cache


def stat(xs):
    q = statistics.quantiles(xs, n=4) if len(xs) > 1 else [xs[0]] * 3
    return {"median_us": round(statistics.median(xs), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1), "samples": len(xs)}


def main_fp8(args):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    cache = parent_fp8(dev, g)
    queries = [(1.7 * torch.randn((Hq, max(WS), D), generator=g, device=dev)).bfloat16() for _ in range(LAYERS)]
    q1 = (1.7 * torch.randn((1, Hq, 1, D), generator=g, device=dev)).bfloat16()
    ws, route = {}, []
    arm(cache, max(WS), queries)
    small = {K: cache.focus(K) for K in KEEPS}         # the caches the focused decode calls read

    def run_decode(K):
        c = cache if K == 0 else small[K]
        st = c._layers[0]
        out = chunk_attention(q1, st.k[:, :, :st.length], st.v[:, :, :st.length], workspace=ws, archive=c.archive(0), packed_gqa=True,
                              route=route)
        assert out is not None

    run_decode(0)
    assert route == ["packed"], route
    names = [("decode_full", 0)] + [(f"decode_{K}", K) for K in KEEPS]
    focus_names = [(f"focus_{K}_W{W}", (K, W)) for W in WS for K in KEEPS]
    samples = {name: [] for name, _ in names + focus_names}

    def timed(name, fn, arg, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(arg)
        e1.record()
        e1.synchronize()
        if keep:
            samples[name].append(e0.elapsed_time(e1) * 1e3)
        del out

    for rep in range(args.warmup + args.reps):
        for name, K in names:                        # interleaved
            timed(name, run_decode, K, rep >= args.warmup)
        for W in WS:
            arm(cache, W, queries)
            for name, (K, w) in focus_names:
                if w == W:
                    timed(name, lambda a: cache.focus(a[0]), (K, W), rep >= args.warmup)
    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "kv_cache_dtype": "fp8_e4m3", "n": N,
                           "pinned": PINNED, "question": QUESTION, "keep_rows": list(KEEPS), "watch_rows": list(WS)},
              "method": f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up "
                        "rounds; focus_* includes the host work and the allocations of the new cache"}
    for name in samples:
        report[name] = stat(samples[name])
    for K in KEEPS:
        report[f"decode_{K}"]["full_over_focused"] = round(report["decode_full"]["median_us"] / report[f"decode_{K}"]["median_us"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name in samples:
        print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    for K in KEEPS:
        print(f"decode over the full archive {report[f'decode_{K}']['full_over_focused']:.1f} x the call over {K} focused rows")
    print("wrote", args.out)


def arm(cache, W, queries):
    cache.watch_question(W)
    for l in range(LAYERS):
        cache._watch.q[l], cache._watch.q_rows[l] = queries[l][:, :W].contiguous(), W


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focus_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fp8", action="store_true", help="an fp8 parent (archive_rescore): the whole focus and the decode calls")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focus.py measures on the GPU; none is visible (Time: not measured)")
    if args.fp8:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "focus_fp8_bench.json")
        return main_fp8(args)
    dev = torch.device("cuda:0")
    stream = nv.stream()
    g = torch.Generator(device=dev).manual_seed(7)
    cache = parent(dev, g)
    queries = [(1.7 * torch.randn((Hq, max(WS), D), generator=g, device=dev)).bfloat16() for _ in range(LAYERS)]
    stores = cache._layers
    cap = stores[0]._k.shape[2]

    # ---- the three calls on their own, on buffers made once ---------------------------------------------------------
    scores = torch.zeros((LAYERS, N), dtype=torch.float32, device=dev)
    stride = max(nv.lib.rtk_pivotkv_rescore_workspace_bytes(Hq, Hkv, W, N, D, nv.RTK_BF16) for W in WS)
    scratch = torch.empty(LAYERS * stride + 256, dtype=torch.uint8, device=dev)
    scratch_p = (scratch.data_ptr() + 255) & ~255
    oq = {W: [q[:, :W].contiguous() for q in queries] for W in WS}
    r_units = {W: (nv.RescoreUnit * LAYERS)(*[nv.RescoreUnit(oq[W][l].data_ptr(), stores[l]._k.data_ptr() + PINNED * D * 2,
                                                             cap * D, scores[l].data_ptr(), N) for l in range(LAYERS)])
               for W in WS}

    def run_rescore(W):
        scores.zero_()
        nv.check(nv.lib.rtk_pivotkv_rescore_batched(r_units[W], LAYERS, Hq, Hkv, W, D, nv.RTK_BF16, 1.0, W * D, D, scratch_p,
                                                    stride, stream), "rtk_pivotkv_rescore_batched")

    run_rescore(max(WS))
    obs = scores.clone()                         # what the selection ranks: one real observation
    idx = {K: torch.empty((LAYERS, K), dtype=torch.int32, device=dev) for K in KEEPS}
    s_units = {K: (nv.BudgetSelectUnit * LAYERS)(*[nv.BudgetSelectUnit(obs[l].data_ptr(), idx[K][l].data_ptr(), N, K)
                                                   for l in range(LAYERS)]) for K in KEEPS}

    def run_select(K):
        nv.check(nv.lib.rtk_pivotkv_budget_select_batched(s_units[K], LAYERS, stream), "rtk_pivotkv_budget_select_batched")

    dst, g_units, moved = {}, {}, {}
    for K in KEEPS:
        run_select(K)
        rows = PINNED + K + QUESTION
        dst[K] = [(torch.empty((1, Hkv, rows, D), dtype=torch.bfloat16, device=dev),
                   torch.empty((1, Hkv, rows, D), dtype=torch.bfloat16, device=dev),
                   torch.empty((3, rows), dtype=torch.int64, device=dev)) for _ in range(LAYERS)]
        us = []
        for l, st in enumerate(stores):
            for src, d, streams, rb in ((st._k, dst[K][l][0], Hkv, D * 2), (st._v, dst[K][l][1], Hkv, D * 2),
                                        (st._pos, dst[K][l][2], 3, 8)):
                us.append(nv.FocusUnit(src.data_ptr(), d.data_ptr(), cap * rb, rows * rb, streams, rb, PINNED, PINNED, N, K,
                                       PINNED + N, QUESTION, idx[K][l].data_ptr()))
        g_units[K] = (nv.FocusUnit * len(us))(*us)
        moved[K] = LAYERS * rows * (2 * Hkv * D * 2 + 3 * 8)
    torch.cuda.synchronize()

    def run_gather(K):
        nv.check(nv.lib.rtk_pivotkv_focus_gather_batched(g_units[K], len(g_units[K]), stream), "rtk_pivotkv_focus_gather_batched")

    csrc = torch.zeros(-(-max(moved.values()) // 16) * 16, dtype=torch.uint8, device=dev)
    cdst = torch.empty_like(csrc)

    def run_copy(K):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(cdst), nv.ptr(csrc), -(-moved[K] // 16) * 16, stream), "rtk_profile_copy")

    def run_index_select(K):
        out = []
        for l, st in enumerate(stores):
            rows = PINNED + idx[K][l].long()
            for t, dim in ((st._k, 2), (st._v, 2), (st._pos, 1)):
                out.append(torch.cat([t.narrow(dim, 0, PINNED), t.index_select(dim, rows), t.narrow(dim, PINNED + N, QUESTION)],
                                     dim=dim))
        return out

    def run_focus(arg):
        K, W = arg
        return cache.focus(K)

    # ---- one decode-attention call over the full rows of a layer and over its focused rows ---------------------------
    q1 = (1.7 * torch.randn((1, Hq, 1, D), generator=g, device=dev)).bfloat16()
    ws, route = {}, []
    full = (stores[0]._k[:, :, :PINNED + N + QUESTION], stores[0]._v[:, :, :PINNED + N + QUESTION])
    run_gather(KEEPS[0]), run_gather(KEEPS[1]), run_gather(KEEPS[2])

    def run_decode(K):
        k, v = full if K == 0 else dst[K][0][:2]
        assert chunk_attention(q1, k, v, workspace=ws, packed_gqa=True, route=route) is not None

    run_decode(0)
    assert route == ["packed"], route

    work = [(f"rescore_W{W}", run_rescore, W) for W in WS] + [(f"select_{K}", run_select, K) for K in KEEPS] + \
           [(f"gather_{K}", run_gather, K) for K in KEEPS] + [(f"copy_{K}", run_copy, K) for K in KEEPS] + \
           [(f"index_select_{K}", run_index_select, K) for K in KEEPS] + \
           [("decode_full", run_decode, 0)] + [(f"decode_{K}", run_decode, K) for K in KEEPS]
    samples = {name: [] for name, _, _ in work}
    focus_names = [(f"focus_{K}_W{W}", (K, W)) for W in WS for K in KEEPS]
    samples.update({name: [] for name, _ in focus_names})

    def timed(name, fn, arg, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(arg)
        e1.record()
        e1.synchronize()
        if keep:
            samples[name].append(e0.elapsed_time(e1) * 1e3)
        del out

    for rep in range(args.warmup + args.reps):
        for name, fn, arg in work:               # interleaved
            timed(name, fn, arg, rep >= args.warmup)
        for W in WS:
            arm(cache, W, queries)
            for name, (K, w) in focus_names:
                if w == W:
                    timed(name, run_focus, (K, W), rep >= args.warmup)

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "n": N, "pinned": PINNED,
                           "question": QUESTION, "keep_rows": list(KEEPS), "watch_rows": list(WS),
                           "gathered_bytes": {str(K): moved[K] for K in KEEPS}},
              "method": f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up "
                        "rounds; focus_* includes the host work and the allocations of the new cache"}
    for name in samples:
        report[name] = stat(samples[name])
    for K in KEEPS:
        gt = report[f"gather_{K}"]
        gt.update(TBps=round(2 * moved[K] / gt["median_us"] / 1e6, 3),
                  time_over_copy=round(gt["median_us"] / report[f"copy_{K}"]["median_us"], 3),
                  index_select_over_gather=round(report[f"index_select_{K}"]["median_us"] / gt["median_us"], 2))
        report[f"decode_{K}"]["full_over_focused"] = round(report["decode_full"]["median_us"] / report[f"decode_{K}"]["median_us"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name in report:
        if isinstance(report[name], dict) and "median_us" in report[name]:
            print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    for K in KEEPS:
        gt = report[f"gather_{K}"]
        print(f"gather_{K}: {gt['TBps']:.2f} TB/s, {gt['time_over_copy']:.2f} x the plain copy, index_select route "
              f"{gt['index_select_over_gather']:.1f} x; decode over the full rows {report[f'decode_{K}']['full_over_focused']:.1f} x "
              "the focused call")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

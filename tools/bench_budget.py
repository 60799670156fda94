#!/usr/bin/env python
"""The video budget's eviction (rtk_pivotkv_budget_select_batched + rtk_pivotkv_squeeze_batched) at the headline geometry,
beside what it has to be weighed against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED
(select, squeeze, slide, copy, ... per repeat, so that all see the same drift of clocks and the same neighbours), the median
of `reps` each.

    python tools/bench_budget.py [--out profiles/budget_bench.json] [--reps 10] [--warmup 3] [--flush-chunks 4]

28 layers, Hkv 4, D 128, bf16, B = 100 352 rows behind 37 pinned rows, evicting d = 1568 rows (one chunk's keep: slack 0) and
d = 8 x 1568 (slack = 7 chunks) out of n = B + d:
  select         one call, 28 units: the survivors of n random scores per layer (a third of them exactly 1.0);
  squeeze        one call that gathers K, V, the [3, n] ids and the scores of all 28 layers down in place along a list that
                 drops d rows at random (runs of ~64 surviving rows); squeeze_fp8 the same on an fp8 archive (codes of 128
                 bytes a row, fp32 scales, ids, scores);
  slide          rtk_pivotkv_slide_batched on the SAME tensors (without the scores) and drop count: the window's move;
  copy           rtk_profile_copy of as many bytes as the squeeze moves, between two buffers;
  flush          the chunk's 28-layer flush (update_pre_rope of every layer, Hq 28, L 6272, ratio 0.25, then the events
                 around after_forward()) on a cache without a bound and on one with a budget it never reaches - the
                 difference is the score gather.
One JSON document; a summary on stdout.  Needs the GPU: there is no other way to get a time."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import retake._native as nv  # noqa: E402
import retake.longvideo_cache as lc  # noqa: E402
import synth  # noqa: E402

LAYERS, Hq, Hkv, D, L, RATIO = 28, 28, 4, 128, 6272, 0.25
KEEP = int(RATIO * L)            # 1568
B, PINNED = 64 * KEEP, 37        # 100 352 rows of video behind the system prompt
DROPS = (KEEP, 8 * KEEP)
SEC = [16, 24, 24]


def _geometry(t):
    rd = 1 if t.ndim == 2 else 2
    row = t.element_size() * (t.shape[3] if t.ndim == 4 else 1)
    return t.shape[rd - 1], t.shape[rd] * row, row     # streams, stream stride, row bytes


def squeeze_units(bufs, idx, rows_in):
    """rtk_squeeze_unit array + bytes moved for (tensor, first row, layer) triples laid out [1, H, cap, D] / [1, H, cap] /
    [P, cap] / [cap]; idx[layer] is the layer's device list."""
    arr = (nv.SqueezeUnit * len(bufs))()
    moved = 0
    for u, (t, first, layer) in zip(arr, bufs):
        streams, stride, row = (1, 0, 4) if t.ndim == 1 else _geometry(t)
        u.base, u.stream_stride, u.streams, u.row_bytes = t.data_ptr(), stride, streams, row
        u.first, u.rows_out, u.rows_in, u.idx = first, B, rows_in, idx[layer].data_ptr()
        moved += streams * B * row
    return arr, moved


def slide_units(bufs, drop):
    arr = (nv.SlideUnit * len(bufs))()
    for u, (t, first, _) in zip(arr, bufs):
        streams, stride, row = _geometry(t)
        u.base, u.stream_stride, u.streams, u.row_bytes, u.first, u.drop, u.rows = t.data_ptr(), stride, streams, row, first, drop, B
    return arr


def flush_samples(dev, chunks, warmup, budget):
    """Milliseconds of after_forward() - the flush of all 28 layers of one chunk."""
    top = {"kvcache_compression": True, "kvcache_compression_kwargs": {
        "compression_ratio": RATIO, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    if budget:
        top["video_budget_rows"] = B
    cfg = types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq, num_key_value_heads=Hkv,
                                longvideo_kwargs=top)
    cache = lc.build_kvcache(cfg, reserve_tokens=(chunks + warmup) * KEEP + L + 64)
    rot = synth.RotaryStub(synth.inv_freq(D), synth.YARN_FACTOR4_ATTENTION_SCALING, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = ((1.7 * torch.randn((1, L, h, D), generator=g, device=dev)).bfloat16().transpose(1, 2) for h in (Hq, Hkv, Hkv))
    out = []
    for c in range(chunks + warmup):
        pos = torch.from_numpy(synth.mrope_position_ids(7 * c, L // 64, 8, 8, hw0=2)).to(dev)
        for layer in range(LAYERS):
            if cache.update_pre_rope(q.clone(), k, v, layer, pos, rot, SEC) is None:
                raise RuntimeError("update_pre_rope declined a video chunk of the benchmark geometry")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cache.after_forward()
        e1.record()
        e1.synchronize()
        if c >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flush-chunks", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_budget.py measures on the GPU; none is visible (Time: not measured)")
    dev = torch.device("cuda:0")
    stream = nv.stream()
    cap = PINNED + B + max(DROPS)
    g = torch.Generator(device=dev).manual_seed(2)
    # 16-bit rows: K, V, ids of every layer; fp8 rows: codes, scales and ids of every layer's archive (ids behind the text)
    rows16, rows8, score_bufs, scores = [], [], [], []
    for layer in range(LAYERS):
        rows16 += [(torch.zeros((1, Hkv, cap, D), dtype=torch.bfloat16, device=dev), PINNED, layer) for _ in range(2)]
        rows16.append((torch.zeros((3, cap), dtype=torch.int64, device=dev), PINNED, layer))
        rows8 += [(torch.zeros((1, Hkv, cap, D), dtype=torch.uint8, device=dev), 0, layer) for _ in range(2)]
        rows8 += [(torch.zeros((1, Hkv, cap), dtype=torch.float32, device=dev), 0, layer) for _ in range(2)]
        rows8.append((torch.zeros((3, cap), dtype=torch.int64, device=dev), PINNED, layer))
        score_bufs.append((torch.zeros(cap, dtype=torch.float32, device=dev), 0, layer))
        s = torch.rand(cap, generator=g, device=dev) * 2.0
        s[torch.rand(cap, generator=g, device=dev) < 0.33] = 1.0
        scores.append(s)
    jobs, selects, keep_alive = {}, {}, []
    for d in DROPS:
        n = B + d
        # a list per layer that drops d of the first n - 1 rows at random
        idx = []
        for layer in range(LAYERS):
            kept = torch.randperm(n - 1, generator=g, device=dev)[:B - 1].sort().values
            idx.append(torch.cat([kept, torch.tensor([n - 1], device=dev)]).to(torch.int32))
        keep_alive.append(idx)
        for name, bufs in (("squeeze", rows16 + score_bufs), ("squeeze_fp8", rows8 + score_bufs)):
            arr, moved = squeeze_units(bufs, idx, n)
            jobs[f"{name}_d{d}"] = {"kind": "squeeze", "units": arr, "n": len(arr), "bytes_moved": moved, "drop": d}
        for name, bufs in (("slide", rows16), ("slide_fp8", rows8)):
            arr = slide_units(bufs, d)
            jobs[f"{name}_d{d}"] = {"kind": "slide", "units": arr, "n": len(arr), "drop": d}
        out = torch.empty((LAYERS, B), dtype=torch.int32, device=dev)
        keep_alive.append(out)
        sel = (nv.BudgetSelectUnit * LAYERS)(*[nv.BudgetSelectUnit(scores[i].data_ptr(), out[i].data_ptr(), n, B)
                                               for i in range(LAYERS)])
        selects[f"select_d{d}"] = {"units": sel, "rows": n}
    biggest = (max(j.get("bytes_moved", 0) for j in jobs.values()) + 15) & ~15
    src = torch.zeros(biggest, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def run_squeeze(j):
        nv.check(nv.lib.rtk_pivotkv_squeeze_batched(j["units"], j["n"], stream), "rtk_pivotkv_squeeze_batched")

    def run_slide(j):
        nv.check(nv.lib.rtk_pivotkv_slide_batched(j["units"], j["n"], stream), "rtk_pivotkv_slide_batched")

    def run_copy(j):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), (j["bytes_moved"] + 15) & ~15, stream), "rtk_profile_copy")

    def run_select(j):
        nv.check(nv.lib.rtk_pivotkv_budget_select_batched(j["units"], LAYERS, stream), "rtk_pivotkv_budget_select_batched")

    work = [(name, run_squeeze if j["kind"] == "squeeze" else run_slide, j) for name, j in jobs.items()] + \
           [("copy_of_" + name, run_copy, j) for name, j in jobs.items() if j["kind"] == "squeeze"] + \
           [(name, run_select, j) for name, j in selects.items()]
    samples = {name: [] for name, _, _ in work}
    for rep in range(args.warmup + args.reps):
        for name, fn, arg in work:           # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)
    del rows16, rows8, score_bufs, scores, src, dst, keep_alive
    torch.cuda.empty_cache()
    flush_ms, flush_budget_ms = [], []
    for _ in range(2):                       # interleaved as well: unbounded, with a budget, unbounded, ...
        flush_ms += flush_samples(dev, args.flush_chunks, 2, False)
        flush_budget_ms += flush_samples(dev, args.flush_chunks, 2, True)
    flush_us = statistics.median(flush_ms) * 1e3

    def stat(xs):
        return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "B": B, "pinned": PINNED, "L": L,
                           "keep": KEEP},
              "method": f"one process, HIP events, interleaved, median of {args.reps} after {args.warmup} warm-up rounds",
              "flush_28_layers": dict(stat([x * 1e3 for x in flush_ms]), chunks=len(flush_ms)),
              "flush_28_layers_with_budget": dict(stat([x * 1e3 for x in flush_budget_ms]), chunks=len(flush_budget_ms)),
              "select": {}, "squeeze": {}}
    for name, j in selects.items():
        report["select"][name] = dict(stat(samples[name]), units=LAYERS, rows=j["rows"], keep=B,
                                      time_over_flush=round(statistics.median(samples[name]) / flush_us, 3))
    for name, j in jobs.items():
        if j["kind"] != "squeeze":
            continue
        s, c = stat(samples[name]), stat(samples["copy_of_" + name])
        sl = stat(samples[name.replace("squeeze", "slide")])
        report["squeeze"][name] = dict(
            s, drop_rows=j["drop"], units=j["n"], launches=-(-j["n"] // nv.SQUEEZE_MAX_UNITS), bytes_moved=j["bytes_moved"],
            read_plus_write_TBps=round(2 * j["bytes_moved"] / s["median_us"] / 1e6, 3),
            slide_median_us=sl["median_us"], time_over_slide=round(s["median_us"] / sl["median_us"], 3),
            copy_median_us=c["median_us"], time_over_copy=round(s["median_us"] / c["median_us"], 3),
            time_over_flush=round(s["median_us"] / flush_us, 3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"flush of 28 layers: {flush_us:.0f} us; with a budget (the score gather): "
          f"{statistics.median(flush_budget_ms) * 1e3:.0f} us")
    for name, r in report["select"].items():
        print(f"{name}: {r['median_us']:.0f} us for {LAYERS} units of {r['rows']} rows")
    for name, r in report["squeeze"].items():
        print(f"{name}: {r['median_us']:.0f} us, {r['bytes_moved'] / 1e9:.2f} GB moved, {r['read_plus_write_TBps']:.2f} TB/s, "
              f"{r['time_over_slide']:.2f} x the slide, {r['time_over_copy']:.2f} x the copy, {r['time_over_flush']:.2f} x the flush")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

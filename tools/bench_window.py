#!/usr/bin/env python
"""The sliding video window's move (rtk_pivotkv_slide_batched) at the headline geometry, beside what it has to be weighed
against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED (slide, copy, slide, ... per repeat, so
that all see the same drift of clocks and the same neighbours), the median of `reps` each.

    python tools/bench_window.py [--out profiles/window_bench.json] [--reps 15] [--warmup 3] [--flush-chunks 6]

28 layers, Hkv 4, D 128, bf16, W = 100 352 rows behind 37 pinned rows:
  slide          one call (84 units: one kernel launch) that moves K, V and the [3, n] ids of all 28 layers down by d rows: d = 1568 (one chunk's keep, the
                 slide of slack 0) and d = 8 x 1568 (slack = 7 chunks);
  slide_fp8      the same with an fp8 archive in place of the 16-bit rows: codes (128 bytes a row), fp32 scales, ids
                 (140 units: two kernel launches);
  copy           rtk_profile_copy (the library's calibration copy, 16-byte non-temporal loads and stores) of as many bytes
                 as the slide moves, between two buffers: the same read + write traffic with nothing to keep in order;
  flush          the chunk's 28-layer flush - update_pre_rope of every layer (Hq 28, L 6272, ratio 0.25), then the events
                 around after_forward() on a cache without the window;
  attention      the chunk's native attention at Lq 6272 over 100 352 prefix rows - what a full window costs every chunk
                 from then on - and over the 200 704 rows an unbounded cache holds after 128 chunks: what the window buys.
Per slide: microseconds, bytes moved, read + write bytes over time (as a fraction of 8 TB/s), its time as a fraction of
the copy's and of the flush's.  One JSON document; a summary on stdout.  Needs the GPU: there is no other way to get a time."""
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
W, PINNED = 64 * KEEP, 37        # 100 352 rows of video behind the system prompt
DROPS = (KEEP, 8 * KEEP)
SEC = [16, 24, 24]


def slide_units(bufs, first, drop, rows):
    """rtk_slide_unit array + bytes moved for tensors laid out [1, H, cap, D] / [1, H, cap] / [P, cap]."""
    arr = (nv.SlideUnit * len(bufs))()
    moved = 0
    for u, (t, f) in zip(arr, bufs):
        rd = 1 if t.ndim == 2 else 2
        row = t.element_size() * (t.shape[3] if t.ndim == 4 else 1)
        u.base, u.stream_stride, u.streams, u.row_bytes = t.data_ptr(), t.shape[rd] * row, t.shape[rd - 1], row
        u.first, u.drop, u.rows = (first if f is None else f), drop, rows
        moved += t.shape[rd - 1] * rows * row
    return arr, moved


def flush_samples(dev, chunks, warmup):
    """Milliseconds of after_forward() - the flush of all 28 layers of one chunk - on a cache without the window."""
    cfg = types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq, num_key_value_heads=Hkv,
                                longvideo_kwargs={"kvcache_compression": True, "kvcache_compression_kwargs": {
                                    "compression_ratio": RATIO, "compression_method": "pivotkv", "pos_embed_reforge": True}})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flush-chunks", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window.py measures on the GPU; none is visible (Time: not measured)")
    dev = torch.device("cuda:0")
    stream = nv.stream()
    cap = PINNED + W + max(DROPS)
    # 16-bit rows: K, V, ids of every layer; fp8 rows: codes, scales and ids of every layer's archive (ids behind the text)
    rows16, rows8 = [], []
    for _ in range(LAYERS):
        rows16 += [(torch.zeros((1, Hkv, cap, D), dtype=torch.bfloat16, device=dev), None) for _ in range(2)]
        rows16.append((torch.zeros((3, cap), dtype=torch.int64, device=dev), None))
        rows8 += [(torch.zeros((1, Hkv, cap, D), dtype=torch.uint8, device=dev), 0) for _ in range(2)]
        rows8 += [(torch.zeros((1, Hkv, cap), dtype=torch.float32, device=dev), 0) for _ in range(2)]
        rows8.append((torch.zeros((3, cap), dtype=torch.int64, device=dev), None))
    jobs = {}
    for name, bufs in (("slide", rows16), ("slide_fp8", rows8)):
        for d in DROPS:
            arr, moved = slide_units(bufs, PINNED, d, W)
            jobs[f"{name}_d{d}"] = {"units": arr, "n": len(arr), "bytes_moved": moved, "drop": d}
    biggest = (max(j["bytes_moved"] for j in jobs.values()) + 15) & ~15
    src = torch.zeros(biggest, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    # the chunk's attention over a full window and over the unbounded prefix after 128 chunks
    g = torch.Generator(device=dev).manual_seed(1)
    prefixes = {"window": W, "unbounded_128_chunks": 128 * KEEP}
    qa = (1.7 * torch.randn((1, L, Hq, D), generator=g, device=dev)).bfloat16().transpose(1, 2)
    ka, va = ((1.7 * torch.randn((1, Hkv, max(prefixes.values()) + L, D), generator=g, device=dev)).bfloat16() for _ in range(2))

    def run_slide(j):
        nv.check(nv.lib.rtk_pivotkv_slide_batched(j["units"], j["n"], stream), "rtk_pivotkv_slide_batched")

    def run_copy(j):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), (j["bytes_moved"] + 15) & ~15, stream), "rtk_profile_copy")

    def run_attention(p):
        if lc.chunk_attention(qa, ka[:, :, :p + L], va[:, :, :p + L]) is None:
            raise RuntimeError("the native attention declined the benchmark shape")

    work = [(name, run_slide, j) for name, j in jobs.items()] + [("copy_of_" + name, run_copy, j) for name, j in jobs.items()] + \
           [("attention_" + name, run_attention, p) for name, p in prefixes.items()]
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
    del rows16, rows8, src, dst, ka, va
    torch.cuda.empty_cache()
    flush_ms = flush_samples(dev, args.flush_chunks, 2)
    flush_us = statistics.median(flush_ms) * 1e3

    def stat(xs):
        return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}

    report = {"device": torch.cuda.get_device_name(0), "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16",
                                                                   "W": W, "pinned": PINNED, "L": L, "keep": KEEP},
              "method": f"one process, HIP events, interleaved, median of {args.reps} after {args.warmup} warm-up rounds",
              "flush_28_layers": dict(stat([x * 1e3 for x in flush_ms]), chunks=len(flush_ms)), "slides": {}, "attention": {}}
    for name, j in jobs.items():
        s, c = stat(samples[name]), stat(samples["copy_of_" + name])
        report["slides"][name] = dict(
            s, drop_rows=j["drop"], units=j["n"], launches=-(-j["n"] // nv.SLIDE_MAX_UNITS), bytes_moved=j["bytes_moved"],
            read_plus_write_TBps=round(2 * j["bytes_moved"] / s["median_us"] / 1e6, 3),
            fraction_of_8TBps=round(2 * j["bytes_moved"] / s["median_us"] / 1e6 / 8.0, 3),
            copy_median_us=c["median_us"], time_over_copy=round(s["median_us"] / c["median_us"], 3),
            time_over_flush=round(s["median_us"] / flush_us, 3))
    for name, p in prefixes.items():
        report["attention"][name] = dict(stat(samples["attention_" + name]), Lq=L, prefix_rows=p)
    a = report["attention"]
    report["attention"]["unbounded_over_window"] = round(a["unbounded_128_chunks"]["median_us"] / a["window"]["median_us"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"flush of 28 layers: {flush_us:.0f} us")
    for name, r in report["slides"].items():
        print(f"{name}: {r['median_us']:.0f} us, {r['bytes_moved'] / 1e9:.2f} GB moved, {r['read_plus_write_TBps']:.2f} TB/s, "
              f"{r['time_over_copy']:.2f} x the copy, {r['time_over_flush']:.2f} x the flush")
    for name in prefixes:
        print(f"attention over {a[name]['prefix_rows']} prefix rows: {a[name]['median_us']:.0f} us per layer")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The position re-base (rtk_pivotkv_rebase_batched, video_position_limit) at the headline geometry, beside what it has to be
weighed against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED (re-base, copy, slide, ... per
repeat, so that all see the same drift of clocks and the same neighbours), medians with quartiles of `reps` each.

    python tools/bench_rebase.py [--out profiles/rebase_bench.json] [--reps 15] [--warmup 3]

28 layers, Hkv 4, D 128, bf16, W = 100 352 region rows behind 37 pinned rows:
  rebase_plain   one call (28 units: a decision launch and an apply launch) that re-bases the [1, n] ids of all layers by
                 delta 1568 and re-rotates every channel pair of their keys;
  rebase_mrope   the same with [3, n] ids and sections [16, 24, 24]: the temporal pairs are chunks 0 - 1 of 8, a quarter of
                 K's bytes; the others are neither loaded nor stored;
  rebase_idle    the plain call with a limit no id reaches: the decision launch, and an apply launch that returns at once;
  copy           rtk_profile_copy (the library's calibration copy, 16-byte non-temporal loads and stores) of as many bytes
                 as the re-base touches (K's temporal chunk pairs + 8 bytes of id a row), between two buffers: the same read
                 + write traffic with no arithmetic;
  slide          rtk_pivotkv_slide_batched on the same K and id tensors, down by 1568 rows: what the move that the re-base
                 rides on costs for these tensors (the real slide moves V as well).
A re-base leaves the ids dense, so a second call would not trigger: the ids are put back (a device copy of 28 small
tensors) before every call, outside the timed events.  The keys keep being rotated: a rotation preserves their magnitude.
Per job: microseconds (median, quartiles, min, max), bytes touched, read + write bytes over time (as a fraction of 8 TB/s),
time over the copy's and over the slide's.  One JSON document; a summary on stdout.  Needs the GPU: there is no other way to
get a time."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import retake._native as nv  # noqa: E402
import synth  # noqa: E402

LAYERS, Hkv, D, KEEP = 28, 4, 128, 1568
W, PINNED, DELTA = 64 * KEEP, 37, KEEP
SEC = [16, 24, 24]
NEVER = 1 << 60


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebase_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rebase.py measures on the GPU; none is visible (Time: not measured)")
    dev = torch.device("cuda:0")
    stream = nv.stream()
    cap = PINNED + W + DELTA
    g = torch.Generator(device=dev).manual_seed(0)
    ks = [(1.7 * torch.randn((1, Hkv, cap, D), generator=g, device=dev)).bfloat16() for _ in range(LAYERS)]
    t = torch.arange(cap, dtype=torch.int64, device=dev)
    t[PINNED:] += DELTA                                   # the gap a slide by DELTA rows leaves behind the pinned rows
    fresh = {1: t.view(1, cap).clone(), 3: torch.stack([t, t + 7, t + 9]).contiguous()}
    ids = {P: [fresh[P].clone() for _ in range(LAYERS)] for P in (1, 3)}
    inv = torch.from_numpy(synth.inv_freq(D)).to(dev)
    sec = (C.c_int * 3)(*SEC)
    offsets = torch.zeros(LAYERS, dtype=torch.int64, device=dev)
    delta = torch.zeros(LAYERS, dtype=torch.int64, device=dev)
    end = PINNED + W
    row = D * 2

    def rebase_units(P):
        return (nv.RebaseUnit * LAYERS)(*[nv.RebaseUnit(ks[l].data_ptr(), cap * row, PINNED, W, ids[P][l].data_ptr(), cap, end,
                                                       Hkv, l) for l in range(LAYERS)])

    def slide_units():
        us = []
        for l in range(LAYERS):
            us.append(nv.SlideUnit(ks[l].data_ptr(), cap * row, Hkv, row, PINNED, DELTA, W))
            us.append(nv.SlideUnit(ids[1][l].data_ptr(), cap * 8, 1, 8, PINNED, DELTA, W))
        return (nv.SlideUnit * len(us))(*us)

    temporal_pairs = {1: D // 2, 3: SEC[0]}
    touched = {P: LAYERS * W * (Hkv * 2 * temporal_pairs[P] * 2 + 8) for P in (1, 3)}   # K's temporal channels + the ids
    jobs = {
        "rebase_plain": {"P": 1, "limit": 0, "units": rebase_units(1), "bytes": touched[1]},
        "rebase_mrope": {"P": 3, "limit": 0, "units": rebase_units(3), "bytes": touched[3]},
        "rebase_idle": {"P": 1, "limit": NEVER, "units": rebase_units(1), "bytes": 0},
    }
    su = slide_units()
    slide_bytes = LAYERS * W * (Hkv * row + 8)
    src = torch.zeros((max(touched.values()) + 15) & ~15, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def put_back(j):
        for x in ids[j["P"]]:
            x.copy_(fresh[j["P"]])

    def run_rebase(j):
        P = j["P"]
        nv.check(nv.lib.rtk_pivotkv_rebase_batched(j["units"], LAYERS, D, nv.RTK_BF16, P, inv.data_ptr(), sec if P == 3 else None,
                                                   3 if P == 3 else 0, j["limit"], offsets.data_ptr(), delta.data_ptr(), stream),
                 "rtk_pivotkv_rebase_batched")

    def run_copy(j):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), (j["bytes"] + 15) & ~15, stream), "rtk_profile_copy")

    def run_slide(_):
        nv.check(nv.lib.rtk_pivotkv_slide_batched(su, len(su), stream), "rtk_pivotkv_slide_batched")

    work = [(name, run_rebase, j, put_back) for name, j in jobs.items()]
    work += [("copy_of_" + name, run_copy, j, None) for name, j in jobs.items() if j["bytes"]]
    work.append(("slide_k_ids", run_slide, None, None))
    samples = {name: [] for name, *_ in work}
    triggered = {}
    for rep in range(args.warmup + args.reps):
        for name, fn, arg, before in work:           # interleaved
            if before is not None:
                before(arg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)
            if fn is run_rebase:
                triggered[name] = int((delta != 0).sum())

    def stat(xs):
        q = statistics.quantiles(xs, n=4)
        return {"median_us": round(statistics.median(xs), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1),
                "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}

    slide = stat(samples["slide_k_ids"])
    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hkv": Hkv, "D": D, "dtype": "bf16", "W": W, "pinned": PINNED, "delta": DELTA,
                           "mrope_section": SEC},
              "method": f"one process, HIP events, interleaved, medians and quartiles of {args.reps} after {args.warmup} warm-up rounds",
              "slide_k_ids": dict(slide, bytes_moved=slide_bytes,
                                  read_plus_write_TBps=round(2 * slide_bytes / slide["median_us"] / 1e6, 3)),
              "rebase": {}}
    for name, j in jobs.items():
        s = stat(samples[name])
        r = dict(s, units=LAYERS, units_triggered=triggered[name], bytes_touched=j["bytes"],
                 time_over_slide=round(s["median_us"] / slide["median_us"], 3))
        if j["bytes"]:
            c = stat(samples["copy_of_" + name])
            r.update(read_plus_write_TBps=round(2 * j["bytes"] / s["median_us"] / 1e6, 3),
                     fraction_of_8TBps=round(2 * j["bytes"] / s["median_us"] / 1e6 / 8.0, 3),
                     copy=c, time_over_copy=round(s["median_us"] / c["median_us"], 3))
        report["rebase"][name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name, r in report["rebase"].items():
        extra = (f", {r['bytes_touched'] / 1e9:.2f} GB touched, {r['read_plus_write_TBps']:.2f} TB/s, {r['time_over_copy']:.2f} x the copy"
                 if r["bytes_touched"] else "")
        print(f"{name}: {r['median_us']:.0f} us [{r['q1_us']:.0f}, {r['q3_us']:.0f}], {r['units_triggered']} of {LAYERS} units "
              f"triggered{extra}, {r['time_over_slide']:.2f} x the slide of K and ids")
    print(f"slide of K and ids: {slide['median_us']:.0f} us, {slide_bytes / 1e9:.2f} GB moved")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

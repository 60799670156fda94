#!/usr/bin/env python
"""The position renumbering (rtk_pivotkv_renumber_batched, video_position_gap) at the headline geometry, beside what it has to
be weighed against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED (every job once per repeat,
so that all see the same drift of clocks and the same neighbours), medians with quartiles of `reps` each.

    python tools/bench_renumber.py [--out profiles/renumber_bench.json] [--reps 15] [--warmup 3]

28 layers, Hkv 4, D 128, bf16, B = 100 352 region rows behind 37 pinned rows, gap 1, plain ids [1, n] and M-RoPE ids [3, n]
with sections [16, 24, 24] (the temporal pairs are a quarter of K's bytes).  Two id patterns of ONE total (18 816):
  holes   a hole of 3 ids in front of every 16th row: the per-row delta changes every 16 rows, and with it a thread's
          cos / sin (fp64 polynomials) - once per 16 adjacent rows;
  front   one hole of 18 816 ids in front of the region: the delta is uniform, the cos / sin are computed once per thread -
          the pattern on which the call does what the re-base does.
Jobs, per id shape: renumber_holes, renumber_front, rebase_front (rtk_pivotkv_rebase_batched, the parent's call, on the same
tensors and the `front` ids), renumber_idle (a limit no id reaches: both launches return at once, nothing is scanned) and copy
(rtk_profile_copy of as many bytes as the apply touches: K's temporal chunk pairs + 8 bytes of id a row; the per-row delta
scratch - 8 bytes a row written by the scan and read twice by the apply - comes on top and is reported).
The scan and the apply are timed SEPARATELY by the library's per-kernel events (rtk_profile_enable_mask: two events around
each launch), the whole call by two events around it.  A renumbering leaves the gaps closed, so a second call would not
trigger: the ids are put back (a device copy of 28 small tensors) before every call, outside the timed events.  The keys
keep being rotated: a rotation preserves their magnitude.  One JSON document; a summary on stdout.  Needs the GPU: there is
no other way to get a time."""
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
B, PINNED, GAP, HOLE, EVERY = 64 * KEEP, 37, 1, 3, 16
TOTAL = (B // EVERY) * HOLE
SEC = [16, 24, 24]
NEVER = 1 << 60
KERNELS = ("renumber_scan", "renumber_apply", "rebase_decide", "rebase_apply")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "renumber_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_renumber.py measures on the GPU; none is visible (Time: not measured)")
    dev = torch.device("cuda:0")
    stream = nv.stream()
    cap = PINNED + B
    g = torch.Generator(device=dev).manual_seed(0)
    ks = [(1.7 * torch.randn((1, Hkv, cap, D), generator=g, device=dev)).bfloat16() for _ in range(LAYERS)]
    dense = torch.arange(cap, dtype=torch.int64, device=dev)
    region = torch.arange(B, dtype=torch.int64, device=dev)
    pattern = {"front": dense.clone(), "holes": dense.clone()}
    pattern["front"][PINNED:] += TOTAL
    pattern["holes"][PINNED:] += HOLE * (region // EVERY + 1)      # (the first hole lies behind the pinned rows)
    fresh = {(p, 1): t.view(1, cap).clone() for p, t in pattern.items()}
    fresh.update({(p, 3): torch.stack([t, t + 7, t + 9]).contiguous() for p, t in pattern.items()})
    ids = {P: [torch.empty_like(fresh[("front", P)]) for _ in range(LAYERS)] for P in (1, 3)}
    scratch = torch.zeros((LAYERS, B), dtype=torch.int64, device=dev)
    inv = torch.from_numpy(synth.inv_freq(D)).to(dev)
    sec = (C.c_int * 3)(*SEC)
    offsets = torch.zeros(LAYERS, dtype=torch.int64, device=dev)
    delta = torch.zeros(LAYERS, dtype=torch.int64, device=dev)
    end, row = PINNED + B, D * 2

    def fields(P, l):
        return (ks[l].data_ptr(), cap * row, PINNED, B, ids[P][l].data_ptr(), cap, end, Hkv, l)

    units = {P: ((nv.RenumberUnit * LAYERS)(*[nv.RenumberUnit(*fields(P, l), scratch[l].data_ptr()) for l in range(LAYERS)]),
                 (nv.RebaseUnit * LAYERS)(*[nv.RebaseUnit(*fields(P, l)) for l in range(LAYERS)])) for P in (1, 3)}
    temporal_pairs = {1: D // 2, 3: SEC[0]}
    touched = {P: LAYERS * B * (Hkv * 2 * temporal_pairs[P] * 2 + 8) for P in (1, 3)}   # K's temporal channels + the ids
    jobs = {}
    for P, tag in ((1, "plain"), (3, "mrope")):
        jobs[f"renumber_holes_{tag}"] = {"P": P, "ids": "holes", "limit": 0, "call": "renumber", "bytes": touched[P]}
        jobs[f"renumber_front_{tag}"] = {"P": P, "ids": "front", "limit": 0, "call": "renumber", "bytes": touched[P]}
        jobs[f"rebase_front_{tag}"] = {"P": P, "ids": "front", "limit": 0, "call": "rebase", "bytes": touched[P]}
    jobs["renumber_idle_plain"] = {"P": 1, "ids": "holes", "limit": NEVER, "call": "renumber", "bytes": 0}
    src = torch.zeros((max(touched.values()) + 15) & ~15, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    kids = nv.profile_kernel_ids()
    mask = 0
    for k in KERNELS:
        mask |= 1 << kids[k]

    def put_back(j):
        for x in ids[j["P"]]:
            x.copy_(fresh[(j["ids"], j["P"])])

    def run_call(j):
        P = j["P"]
        s, n = (sec, 3) if P == 3 else (None, 0)
        if j["call"] == "renumber":
            nv.check(nv.lib.rtk_pivotkv_renumber_batched(units[P][0], LAYERS, D, nv.RTK_BF16, P, inv.data_ptr(), s, n, j["limit"], GAP,
                                                         offsets.data_ptr(), delta.data_ptr(), stream), "rtk_pivotkv_renumber_batched")
        else:
            nv.check(nv.lib.rtk_pivotkv_rebase_batched(units[P][1], LAYERS, D, nv.RTK_BF16, P, inv.data_ptr(), s, n, j["limit"],
                                                       offsets.data_ptr(), delta.data_ptr(), stream), "rtk_pivotkv_rebase_batched")

    def run_copy(j):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), (j["bytes"] + 15) & ~15, stream), "rtk_profile_copy")

    work = [(name, run_call, j, put_back) for name, j in jobs.items()]
    work += [(f"copy_{tag}", run_copy, {"bytes": touched[P]}, None) for P, tag in ((1, "plain"), (3, "mrope"))]
    samples = {name: [] for name, *_ in work}
    kernel_us = {name: {} for name in jobs}
    seen = {}
    for rep in range(args.warmup + args.reps):
        for name, fn, arg, before in work:           # interleaved
            if before is not None:
                before(arg)
            nv.lib.rtk_profile_reset()
            nv.lib.rtk_profile_enable_mask(mask if fn is run_call else 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg)
            e1.record()
            e1.synchronize()
            if fn is run_call:
                got = nv.profile_read()
                nv.lib.rtk_profile_enable(0)
                seen[name] = (int((delta != 0).sum()), sorted(set(delta.tolist())))
                if rep >= args.warmup:
                    for k, (_, ms) in got.items():
                        kernel_us[name].setdefault(k, []).append(ms * 1e3)
            if rep >= args.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)
    nv.lib.rtk_profile_reset()

    def stat(xs):
        q = statistics.quantiles(xs, n=4)
        return {"median_us": round(statistics.median(xs), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1),
                "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hkv": Hkv, "D": D, "dtype": "bf16", "B": B, "pinned": PINNED, "gap": GAP,
                           "total": TOTAL, "hole": HOLE, "rows_per_hole": EVERY, "mrope_section": SEC},
              "method": f"one process, HIP events, interleaved, medians and quartiles of {args.reps} after {args.warmup} warm-up "
                        "rounds; scan / apply from the library's per-kernel events, the call from two events around it",
              "row_delta_bytes_on_top": {"scan_writes": LAYERS * B * 8, "apply_reads": 2 * LAYERS * B * 8},
              "jobs": {}}
    copies = {tag: stat(samples[f"copy_{tag}"]) for tag in ("plain", "mrope")}
    for name, j in jobs.items():
        tag = "plain" if j["P"] == 1 else "mrope"
        s = stat(samples[name])
        r = dict(s, units=LAYERS, units_triggered=seen[name][0], deltas=seen[name][1], bytes_touched=j["bytes"],
                 kernels={k: stat(v) for k, v in kernel_us[name].items()})
        if j["bytes"]:
            r.update(read_plus_write_TBps=round(2 * j["bytes"] / s["median_us"] / 1e6, 3), copy=copies[tag],
                     time_over_copy=round(s["median_us"] / copies[tag]["median_us"], 3))
        report["jobs"][name] = r
    ratios = {}
    for tag in ("plain", "mrope"):
        jb = report["jobs"]
        base = jb[f"rebase_front_{tag}"]["median_us"]
        ratios[tag] = {"renumber_front_over_rebase_front": round(jb[f"renumber_front_{tag}"]["median_us"] / base, 3),
                       "renumber_holes_over_rebase_front": round(jb[f"renumber_holes_{tag}"]["median_us"] / base, 3),
                       "apply_holes_over_apply_front": round(jb[f"renumber_holes_{tag}"]["kernels"]["renumber_apply"]["median_us"]
                                                             / jb[f"renumber_front_{tag}"]["kernels"]["renumber_apply"]["median_us"], 3),
                       "scan_over_apply_holes": round(jb[f"renumber_holes_{tag}"]["kernels"]["renumber_scan"]["median_us"]
                                                      / jb[f"renumber_holes_{tag}"]["kernels"]["renumber_apply"]["median_us"], 3)}
    report["ratios"] = ratios
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name, r in report["jobs"].items():
        ks_ = ", ".join(f"{k} {v['median_us']:.0f}" for k, v in r["kernels"].items())
        extra = f", {r['time_over_copy']:.2f} x the copy, {r['read_plus_write_TBps']:.2f} TB/s" if r["bytes_touched"] else ""
        print(f"{name}: {r['median_us']:.0f} us [{r['q1_us']:.0f}, {r['q3_us']:.0f}] ({ks_}), {r['units_triggered']} of {LAYERS} "
              f"units triggered{extra}")
    print("ratios:", json.dumps(ratios))
    print("wrote", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The budget's re-scoring (rtk_pivotkv_rescore_batched, longvideo_kwargs["video_budget_rescore"]) at the headline geometry,
beside what it has to be weighed against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED
(so that all see the same drift of clocks and the same neighbours), medians of `reps` with quartiles.

    python tools/bench_rescore.py [--out profiles/rescore_bench.json] [--parity profiles/rescore_parity_stats.txt]
                                  [--reps 15] [--warmup 3] [--flush-chunks 4]

28 layers, Hq 28 / Hkv 4 / D 128, bf16, n = 100 352 old region rows per layer behind 37 pinned rows:
  rescore_W64 / rescore_W16   one call, 28 units: the three launches (range pass, merge, column pass) for all layers;
  copy_keys_1pass / _2pass    rtk_profile_copy of the bytes of the region's keys, once and twice: the call reads every key
                              row in each of its two passes, so the two-pass copy (which also WRITES them) bounds it from above
                              at the byte floor;
  query_copies_W64 / _W16     the 28 per-layer slice copies of the capture ([Hq, W, D] out of a chunk's [1, Hq, L, D]);
  select, squeeze             one eviction of a chunk's keep (rtk_pivotkv_budget_select_batched + _squeeze_batched: K, V, ids
                              and scores of all layers), as tools/bench_budget.py measures it;
  flush                       the 28-layer flush of an L 6272 chunk (after_forward() of a cache without a bound).
The parity file gets the error of ONE layer of the W 64 call against float64: a row sum of 10^5 fp32 terms; no bar at that
size, the number is recorded.  One JSON document; a summary on stdout.  Needs the GPU: there is no other way to get a time.

    python tools/bench_rescore.py --fp8 [--out profiles/rescore_fp8_bench.json] [--reps 15] [--warmup 3]

The re-scoring over the e4m3 key rows of an fp8 archive (rtk_pivotkv_rescore_fp8k_batched, longvideo_kwargs
["archive_rescore"]) at the same geometry, the same method, W 64 and W 16:
  fp8k_W*                     the new call: one call, 28 units, codes and scales read where they lie;
  dense16_W*                  rtk_pivotkv_rescore_batched on the same rows dequantised in advance (the same bits);
  dequant_then_dense16_W*     the route without the entry: rtk_fp8kv_dequant of every layer's region into a 16-bit scratch,
                              then the call above;
  copy_read_bytes             rtk_profile_copy of the bytes the new call reads: 2 n Hkv (D + 4) per layer for its two passes."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import bench_budget as bb  # noqa: E402
import rescore_ref as rr  # noqa: E402
import retake._native as nv  # noqa: E402

LAYERS, Hq, Hkv, D, L, KEEP, B, PINNED = bb.LAYERS, bb.Hq, bb.Hkv, bb.D, bb.L, bb.KEEP, bb.B, bb.PINNED
WS = (64, 16)
ALPHA = 0.5


def timed(work, warmup, reps):
    """{name: [us]}: every (name, fn, arg) of `work` once per round, the rounds interleaved, HIP events around each."""
    samples = {name: [] for name, _, _ in work}
    for rep in range(warmup + reps):
        for name, fn, arg in work:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg)
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)
    return samples


def stat(xs):
    q = statistics.quantiles(xs, n=4) if len(xs) > 1 else [xs[0]] * 3
    return {"median_us": round(statistics.median(xs), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1), "samples": len(xs)}


def main_fp8(args):
    from retake.native_attention import fp8_dequantize_rows, fp8_quantize_rows

    dev = torch.device("cuda:0")
    stream = nv.stream()
    n = B
    g = torch.Generator(device=dev).manual_seed(5)
    codes, scales, dense, scores8, scores16, oqs = [], [], [], [], [], []
    for _ in range(LAYERS):
        k = torch.empty((1, Hkv, n, D), dtype=torch.bfloat16, device=dev)
        k.normal_(0.0, 1.7, generator=g)
        c, s = fp8_quantize_rows(k)
        codes.append(c)
        scales.append(s)
        dense.append(fp8_dequantize_rows(c, s, torch.bfloat16))
        scores8.append(torch.rand(n, generator=g, device=dev) * 2.0)
        scores16.append(scores8[-1].clone())
        oqs.append((1.7 * torch.randn((Hq, max(WS), D), generator=g, device=dev)).bfloat16())
        del k
    spare = [torch.empty_like(t) for t in dense]           # where the route without the entry dequantises to
    stride = nv.lib.rtk_pivotkv_rescore_workspace_bytes(Hq, Hkv, max(WS), n, D, nv.RTK_BF16)
    scratch = torch.empty(LAYERS * stride + 256, dtype=torch.uint8, device=dev)
    scratch_p = (scratch.data_ptr() + 255) & ~255
    u8 = (nv.RescoreFp8kUnit * LAYERS)(*[nv.RescoreFp8kUnit(oqs[i].data_ptr(), codes[i].data_ptr(), n * D, scales[i].data_ptr(), n,
                                                            scores8[i].data_ptr(), n) for i in range(LAYERS)])
    u16 = (nv.RescoreUnit * LAYERS)(*[nv.RescoreUnit(oqs[i].data_ptr(), dense[i].data_ptr(), n * D, scores16[i].data_ptr(), n)
                                      for i in range(LAYERS)])
    usp = (nv.RescoreUnit * LAYERS)(*[nv.RescoreUnit(oqs[i].data_ptr(), spare[i].data_ptr(), n * D, scores16[i].data_ptr(), n)
                                      for i in range(LAYERS)])
    read_bytes = LAYERS * 2 * n * Hkv * (D + 4)
    src = torch.zeros(read_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def run_fp8k(W):
        nv.check(nv.lib.rtk_pivotkv_rescore_fp8k_batched(u8, LAYERS, Hq, Hkv, W, D, nv.RTK_BF16, ALPHA, max(WS) * D, D, scratch_p,
                                                         stride, stream), "rtk_pivotkv_rescore_fp8k_batched")

    def run_dense(W, units=u16):
        nv.check(nv.lib.rtk_pivotkv_rescore_batched(units, LAYERS, Hq, Hkv, W, D, nv.RTK_BF16, ALPHA, max(WS) * D, D, scratch_p,
                                                    stride, stream), "rtk_pivotkv_rescore_batched")

    def run_dequant_then_dense(W):
        for i in range(LAYERS):
            nv.check(nv.lib.rtk_fp8kv_dequant(nv.ptr(codes[i]), n * D, nv.ptr(scales[i]), n, nv.ptr(spare[i]), n * D, Hkv, n, D,
                                              nv.RTK_BF16, stream), "rtk_fp8kv_dequant")
        run_dense(W, usp)

    def run_copy(_):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), read_bytes, stream), "rtk_profile_copy")

    # the first calls, on equal scores: the two routes give the same bits
    run_fp8k(max(WS))
    run_dense(max(WS))
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(scores8, scores16))
    work = [(f"fp8k_W{W}", run_fp8k, W) for W in WS] + [(f"dense16_W{W}", run_dense, W) for W in WS] + \
           [(f"dequant_then_dense16_W{W}", run_dequant_then_dense, W) for W in WS] + [("copy_read_bytes", run_copy, 0)]
    samples = timed(work, args.warmup, args.reps)
    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "n": n, "alpha": ALPHA,
                           "read_bytes_two_passes": read_bytes, "dense_key_bytes_two_passes": LAYERS * 2 * n * Hkv * D * 2},
              "method": f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up rounds",
              "first_call_bits_equal_the_16_bit_call": same}
    for name, _, _ in work:
        report[name] = stat(samples[name])
    c = report["copy_read_bytes"]["median_us"]
    for W in WS:
        r = report[f"fp8k_W{W}"]
        r.update(read_TBps=round(read_bytes / r["median_us"] / 1e6, 3), time_over_copy=round(r["median_us"] / c, 3),
                 time_over_dense16=round(r["median_us"] / report[f"dense16_W{W}"]["median_us"], 3),
                 time_over_dequant_then_dense16=round(r["median_us"] / report[f"dequant_then_dense16_W{W}"]["median_us"], 3),
                 tflops=round(2 * 2.0 * Hq * W * n * D * LAYERS / r["median_us"] / 1e6, 1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("first call: the bits of the 16-bit call on the dequantised rows:", same)
    for name, _, _ in work:
        print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    for W in WS:
        r = report[f"fp8k_W{W}"]
        print(f"fp8k_W{W}: {r['time_over_dense16']:.2f} x the 16-bit call on rows dequantised in advance, "
              f"{r['time_over_dequant_then_dense16']:.2f} x dequantise-then-call, {r['time_over_copy']:.2f} x the copy of its bytes, "
              f"{r['read_TBps']:.2f} TB/s read, {r['tflops']:.0f} TFLOP/s")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_bench.json"))
    ap.add_argument("--parity", default=os.path.join(ROOT, "profiles", "rescore_parity_stats.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flush-chunks", type=int, default=4)
    ap.add_argument("--fp8", action="store_true", help="the call over e4m3 archive rows against the 16-bit routes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rescore.py measures on the GPU; none is visible (Time: not measured)")
    if args.fp8:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "rescore_fp8_bench.json")
        return main_fp8(args)
    dev = torch.device("cuda:0")
    stream = nv.stream()
    n, cap = B, PINNED + B + KEEP
    g = torch.Generator(device=dev).manual_seed(5)
    keys, vals, ids, scores, oqs = [], [], [], [], []
    for _ in range(LAYERS):
        k = torch.empty((1, Hkv, cap, D), dtype=torch.bfloat16, device=dev)
        k.normal_(0.0, 1.7, generator=g)
        keys.append(k)
        vals.append(torch.zeros_like(k))
        ids.append(torch.zeros((3, cap), dtype=torch.int64, device=dev))
        scores.append(torch.rand(cap, generator=g, device=dev) * 2.0)
        oqs.append((1.7 * torch.randn((Hq, max(WS), D), generator=g, device=dev)).bfloat16())
    chunk_q = (1.7 * torch.randn((1, L, Hq, D), generator=g, device=dev)).bfloat16().transpose(1, 2)   # the projection layout
    stride = nv.lib.rtk_pivotkv_rescore_workspace_bytes(Hq, Hkv, max(WS), n + KEEP, D, nv.RTK_BF16)
    scratch = torch.empty(LAYERS * stride + 256, dtype=torch.uint8, device=dev)
    scratch_p = (scratch.data_ptr() + 255) & ~255
    units = (nv.RescoreUnit * LAYERS)(*[nv.RescoreUnit(oqs[i].data_ptr(), keys[i].data_ptr() + PINNED * D * 2, cap * D,
                                                       scores[i].data_ptr(), n) for i in range(LAYERS)])
    key_bytes = LAYERS * Hkv * n * D * 2
    src = torch.zeros(2 * key_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def run_rescore(W):
        nv.check(nv.lib.rtk_pivotkv_rescore_batched(units, LAYERS, Hq, Hkv, W, D, nv.RTK_BF16, ALPHA, max(WS) * D, D, scratch_p,
                                                    stride, stream), "rtk_pivotkv_rescore_batched")

    def run_copy(passes):
        nv.check(nv.lib.rtk_profile_copy(nv.ptr(dst), nv.ptr(src), passes * key_bytes, stream), "rtk_profile_copy")

    def run_query_copies(W):
        for i in range(LAYERS):
            oqs[i][:, :W].copy_(chunk_q[0, :, L - W:])

    # one eviction of a chunk's keep: the survivors of n + KEEP scores, then K, V, ids and scores gathered down
    rows = n + KEEP
    idx = [torch.cat([torch.randperm(rows - 1, generator=g, device=dev)[:B - 1].sort().values,
                      torch.tensor([rows - 1], device=dev)]).to(torch.int32) for _ in range(LAYERS)]
    bufs = []
    for i in range(LAYERS):
        bufs += [(keys[i], PINNED, i), (vals[i], PINNED, i), (ids[i], PINNED, i), (scores[i], 0, i)]
    sq_units, moved = bb.squeeze_units(bufs, idx, rows)
    sel_out = torch.empty((LAYERS, B), dtype=torch.int32, device=dev)
    sel = (nv.BudgetSelectUnit * LAYERS)(*[nv.BudgetSelectUnit(scores[i].data_ptr(), sel_out[i].data_ptr(), rows, B)
                                           for i in range(LAYERS)])

    def run_select(_):
        nv.check(nv.lib.rtk_pivotkv_budget_select_batched(sel, LAYERS, stream), "rtk_pivotkv_budget_select_batched")

    def run_squeeze(_):
        nv.check(nv.lib.rtk_pivotkv_squeeze_batched(sq_units, len(sq_units), stream), "rtk_pivotkv_squeeze_batched")

    # parity of one layer, W 64, on the first call (the scores are still the random ones)
    old = scores[0][:n].clone()
    k0 = keys[0][0, :, PINNED:PINNED + n]
    want = rr.rescored(old, oqs[0], k0, n, ALPHA).to(dev)
    m64 = rr.mass(oqs[0], k0, n)
    run_rescore(max(WS))
    torch.cuda.synchronize()
    err = (scores[0][:n].double() - want).abs()
    bar = rr.bar(ALPHA, n, max(WS), 2e-5, m64, want)
    parity = (f"rtk_pivotkv_rescore_batched, one layer of the headline geometry (Hq {Hq} / Hkv {Hkv} / D {D}, bf16, W {max(WS)}, "
              f"n = {n}, alpha {ALPHA}) against float64: max |got - want| = {err.max().item():.3e}, mean {err.mean().item():.3e}; "
              f"as a share of the kernel test's per-row bar (alpha (n / W) 2e-5 max(1, mass) + 4 2^-24 |want|; not asserted at "
              f"this size): max {(err / bar).max().item():.3f}; obs ranges over [{(m64.min().item() * n / max(WS)):.3e}, "
              f"{(m64.max().item() * n / max(WS)):.3e}], a row sum of {n} fp32 terms.")
    del want, m64, err, bar, old

    work = [(f"rescore_W{W}", run_rescore, W) for W in WS] + [(f"copy_keys_{p}pass", run_copy, p) for p in (1, 2)] + \
           [(f"query_copies_W{W}", run_query_copies, W) for W in WS] + [("select", run_select, 0), ("squeeze", run_squeeze, 0)]
    samples = timed(work, args.warmup, args.reps)           # interleaved
    del keys, vals, ids, scores, src, dst, idx, bufs, scratch
    torch.cuda.empty_cache()
    flush_us = [x * 1e3 for x in bb.flush_samples(dev, args.flush_chunks, 2, False)]

    fl = statistics.median(flush_us)
    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "n": n, "pinned": PINNED, "L": L,
                           "keep": KEEP, "alpha": ALPHA, "key_bytes_per_pass": key_bytes, "scratch_bytes": LAYERS * stride},
              "method": f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up rounds",
              "flush_28_layers": stat(flush_us)}
    for name, _, _ in work:
        report[name] = stat(samples[name])
    c1, c2 = report["copy_keys_1pass"]["median_us"], report["copy_keys_2pass"]["median_us"]
    evict = report["select"]["median_us"] + report["squeeze"]["median_us"]
    for W in WS:
        r = report[f"rescore_W{W}"]
        r.update(key_read_TBps=round(2 * key_bytes / r["median_us"] / 1e6, 3), time_over_copy_1pass=round(r["median_us"] / c1, 3),
                 time_over_copy_2pass=round(r["median_us"] / c2, 3), time_over_flush=round(r["median_us"] / fl, 3),
                 time_over_eviction=round(r["median_us"] / evict, 3),
                 tflops=round(2 * 2.0 * Hq * W * n * D * LAYERS / r["median_us"] / 1e6, 1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    with open(args.parity, "a") as f:
        f.write(parity + "\n")
    print(parity)
    for name in report:
        if isinstance(report[name], dict) and "median_us" in report[name]:
            print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    for W in WS:
        r = report[f"rescore_W{W}"]
        print(f"rescore_W{W}: {r['time_over_copy_2pass']:.2f} x the two-pass key copy, {r['time_over_flush']:.2f} x the flush, "
              f"{r['time_over_eviction']:.2f} x one eviction, {r['key_read_TBps']:.2f} TB/s of keys, {r['tflops']:.0f} TFLOP/s")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

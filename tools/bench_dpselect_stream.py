#!/usr/bin/env python3
"""Times DPSelect on a stream (retake/dpselect_stream.py) on the GPU:  tools/bench_dpselect_stream.py [--out FILE]

One process, HIP events, the candidates of a comparison interleaved in every repeat, medians with quartiles.  Per geometry
(N x C, bf16: 144 x 3584 and 196 x 1280):
  ingest      rtk_dpselect_ingest of a 32-frame piece, against the two launches it replaces - rtk_profile_copy of the same
              bytes into a staging buffer behind the halo row, then rtk_dpselect_dis over [prev | piece] (33 rows)
  select      rtk_dpselect_select_ring + rtk_gather_frames of one 32-frame segment (keep 8, sync and async)
  stream      2048 frames through DPSelectStream(32, ratio=0.25) in pushes of 32, against ONE memory_bank_compress_keyframe
              over all 2048 (which needs the whole video resident)
Bytes are computed from the shapes: the fused ingest moves 2 row-passes where the two launches move 3, so by bytes it
should take about two thirds of their time - that is the formula; the table holds what was measured.  Every timed window
repeats its work until it lasts a few milliseconds.  There is no fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-retake_amd"))

GEOMETRIES = ((144, 3584), (196, 1280))
PIECE, SEG, KEEP, STREAM_T = 32, 32, 8, 2048


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"median_us": med, "q1_us": q1, "q3_us": q3, "n": len(v)}


def timed(fn, inner):
    """One window: `inner` calls between two events; microseconds per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def compare(cands, repeats, inner, warmup=3):
    """cands: {name: fn}.  Interleaved: every repeat times each candidate once, in turn."""
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in cands}
    for _ in range(repeats):
        for k, fn in cands.items():
            out[k].append(timed(fn, inner))
    return {k: quartiles(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpselect_stream_bench.json"))
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dpselect_stream: no GPU - nothing is measured on a CPU")
    import retake._native as nv
    import retake.visual_compression as vc
    from retake.dpselect_stream import DPSelectStream

    dev = torch.device("cuda:0")
    lib, ptr, dt = nv.lib, nv.ptr, nv.RTK_BF16
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "piece_frames": PIECE, "segment_frames": SEG,
           "repeats": args.repeats, "geometries": {}}
    for N, C in GEOMETRIES:
        g = torch.Generator(device="cpu").manual_seed(N * C)
        x = torch.randn((PIECE, N, C), generator=g).to(dev).to(torch.bfloat16)
        R = 2 * SEG
        ring = torch.randn((R, N, C), generator=g).to(dev).to(torch.bfloat16)
        dis_ring = torch.empty((R, N), dtype=torch.float32, device=dev)
        stage = torch.empty((PIECE + 1, N, C), dtype=torch.bfloat16, device=dev)
        stage[0].copy_(ring[R - 1])
        dis2 = torch.empty((PIECE + 1, N), dtype=torch.float32, device=dev)
        st = nv.stream()
        row_bytes = N * C * 2
        piece_bytes = PIECE * row_bytes

        def fused():
            nv.check(lib.rtk_dpselect_ingest(ptr(x), ptr(ring[R - 1]), PIECE, N, C, dt, ptr(ring[0]), ptr(dis_ring[0]), st), "ingest")

        def two_launches():
            nv.check(lib.rtk_profile_copy(ptr(stage[1]), ptr(x), piece_bytes, st), "copy")
            nv.check(lib.rtk_dpselect_dis(ptr(stage), PIECE + 1, N, C, dt, ptr(dis2), st), "dis")

        fused(), two_launches()
        torch.cuda.synchronize()
        assert torch.equal(ring[:PIECE].view(torch.int16), x.view(torch.int16))
        assert torch.equal(dis_ring[:PIECE].view(torch.int32), dis2[1:].view(torch.int32)), "the fused distances differ"
        ingest = compare({"ingest": fused, "copy_then_dis": two_launches}, args.repeats, inner=200)
        ingest["bytes"] = {"ingest": 2 * piece_bytes + row_bytes + 4 * PIECE * N,
                           "copy_then_dis": 3 * piece_bytes + row_bytes + 4 * (PIECE + 1) * N}
        ingest["ratio_measured"] = ingest["ingest"]["median_us"] / ingest["copy_then_dis"]["median_us"]
        ingest["ratio_by_bytes"] = ingest["bytes"]["ingest"] / ingest["bytes"]["copy_then_dis"]
        ingest["ingest_GBps"] = ingest["bytes"]["ingest"] / (ingest["ingest"]["median_us"] * 1e-6) / 1e9

        # one segment: rows 32 .. 63 of a ring that holds 64 frames, halo rows on both sides
        nv.check(lib.rtk_dpselect_ingest(ptr(ring[:SEG].clone()), None, SEG, N, C, dt, ptr(ring[0]), ptr(dis_ring[0]), st), "ingest")
        nv.check(lib.rtk_dpselect_ingest(ptr(ring[SEG:].clone()), ptr(ring[SEG - 1]), SEG, N, C, dt, ptr(ring[SEG]),
                                         ptr(dis_ring[SEG]), st), "ingest")
        keys = torch.empty((max(2 * SEG + 2, N * SEG),), dtype=torch.float32, device=dev)
        mask = torch.empty((KEEP, N), dtype=torch.bool, device=dev)
        out = torch.empty((KEEP, N, C), dtype=torch.bfloat16, device=dev)
        sel = {}
        for sync in (1, 0):
            idx = torch.empty((KEEP,) if sync else (KEEP, N), dtype=torch.int64, device=dev)

            def select_gather(sync=sync, idx=idx):
                nv.check(lib.rtk_dpselect_select_ring(ptr(dis_ring), R, N, SEG, SEG, 1, 1, KEEP, 3, sync, ptr(idx), ptr(mask),
                                                      ptr(keys), st), "select_ring")
                nv.check(lib.rtk_gather_frames(ptr(ring[SEG]), SEG, N, C, dt, ptr(idx), KEEP, sync, ptr(out), st), "gather")

            sel["sync" if sync else "async"] = compare({"select_gather": select_gather}, args.repeats, inner=200)["select_gather"]

        # the whole pipeline
        video = torch.randn((STREAM_T, N, C), device=dev, dtype=torch.bfloat16, generator=torch.Generator(device=dev).manual_seed(N))
        stream = DPSelectStream(SEG, ratio=0.25, sync=False)

        def streamed():
            stream.reset()
            n = 0
            for o in range(0, STREAM_T, SEG):
                n += len(stream.push(video[o:o + SEG]))
            n += len(stream.finish())
            assert n == STREAM_T // SEG

        def whole():
            vc.memory_bank_compress_keyframe(video[None], STREAM_T // 4, 3, sync=False)

        pipe = compare({"stream_2048": streamed, "whole_video_2048": whole}, max(5, args.repeats // 3), inner=2)
        pipe["ratio_measured"] = pipe["stream_2048"]["median_us"] / pipe["whole_video_2048"]["median_us"]
        pipe["stream_ring_bytes"] = stream.memory_footprint()
        pipe["whole_video_input_bytes"] = video.numel() * 2
        res["geometries"][f"{N}x{C}"] = {"ingest_32_frames": ingest, "select_gather_32_frames": sel, "frames_2048": pipe}
        del video, stream
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()

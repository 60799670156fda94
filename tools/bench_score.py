#!/usr/bin/env python3
"""Micro-benchmark of rtk_pivotkv_score (and friends) at BASELINE geometry; prints per-kernel avg µs.
    python tools/bench_score.py [--dtype bf16|fp32] [--L 6272] [--iters 20]
    python tools/bench_score.py --prompt-rows 64 [--out profiles/prompt_score_bench.json]
        the flush of a 28-layer chunk, prompt-guided at (Lv, Lp) = (6272, N) and (2304, N), against the same tree with the
        key off on L = Lv + Lp (HIP events, one process)"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import retake._native as nv


def prompt_flush_bench(Lp, iters, out):
    """ms per flush (score + selection + compaction of 28 pending layers; the updates are not timed) of a bf16 Qwen2-VL-shaped
    chunk, prompt_guided_scoring on and off, plus one profiled flush per mode (rtk_profile_*: per-kernel ms)."""
    import json
    import types

    import numpy as np

    import retake.longvideo_cache as lc
    import synth

    dev = torch.device("cuda:0")
    Hq, Hkv, D, layers, ratio, sec = 28, 4, 128, 28, 0.25, [16, 24, 24]
    rot = synth.RotaryStub(synth.inv_freq(D), synth.YARN_FACTOR4_ATTENTION_SCALING, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "layers": layers, "ratio": ratio, "prompt_rows": Lp,
              "iters": iters, "timed": "after_forward(): the flush of 28 pending layers, HIP events, median", "cases": []}
    for Lv in (6272, 2304):
        L = Lv + Lp
        g = torch.Generator(device=dev).manual_seed(0)
        q0, k0, v0 = ((1.7 * torch.randn((1, L, h, D), generator=g, device=dev)).to(torch.bfloat16).transpose(1, 2)
                      for h in (Hq, Hkv, Hkv))
        vid = synth.mrope_position_ids(0, Lv // 64, 8, 8)
        ids = np.concatenate([vid, np.broadcast_to(np.arange(Lp, dtype=np.int64) + vid.max() + 1, (3, 1, Lp))], axis=-1)
        case = {"Lv": Lv, "Lp": Lp, "L": L, "score_flop_ratio": round(L * L / (Lp * Lv), 1)}
        for name, on in (("prompt_guided", True), ("key_off", False)):
            cfg = types.SimpleNamespace(
                hidden_size=Hq * D, num_hidden_layers=layers, num_attention_heads=Hq, num_key_value_heads=Hkv,
                longvideo_kwargs={"kvcache_compression": True, "kvcache_compression_kwargs": {
                    "compression_ratio": ratio, "compression_method": "pivotkv", "pos_embed_reforge": True,
                    "prompt_guided_scoring": on}})
            cache = lc.build_kvcache(cfg, reserve_tokens=(iters + 4) * L)
            times, prof = [], None
            for it in range(iters + 3):   # 2 warm-up chunks, `iters` timed ones, one profiled
                pos = torch.from_numpy(ids).to(dev)
                cache.before_forward(prompt_length=Lp)
                for l in range(layers):
                    cache.shift_temporal_ids_(pos, l)
                    q = synth.rope_forward(q0, pos, rot, sec)
                    k = synth.rope_forward(k0, pos, rot, sec)
                    cache.update(k, v0, l, {"query_states": q, "position_ids": pos, "rotary_emb": rot, "mrope_section": sec})
                profiled = it == iters + 2
                if profiled:
                    nv.lib.rtk_profile_reset()
                    nv.lib.rtk_profile_enable(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cache.after_forward()
                e1.record()
                torch.cuda.synchronize()
                if profiled:
                    nv.lib.rtk_profile_enable(0)
                    prof = {k: round(ms, 4) for k, (n, ms) in nv.profile_read().items()}
                elif it >= 2:
                    times.append(e0.elapsed_time(e1))
            times.sort()
            case[name] = {"flush_ms_median": round(times[len(times) // 2], 4), "flush_ms_min": round(times[0], 4),
                          "flush_ms_max": round(times[-1], 4), "kept_per_chunk": int(cache.get_seq_length(0) // (iters + 3)),
                          "profiled_flush_kernel_ms": prof}
            del cache
            torch.cuda.empty_cache()
        case["speedup"] = round(case["key_off"]["flush_ms_median"] / case["prompt_guided"]["flush_ms_median"], 3)
        result["cases"].append(case)
        print(json.dumps(case))
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--L", type=int, default=6272)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--refround", action="store_true", help="bf16 payloads with the reference's bf16 score chain")
    ap.add_argument("--units", type=int, default=0, help="time rtk_pivotkv_score_passes_batched over this many units")
    ap.add_argument("--prompt-rows", type=int, default=0, help="time the 28-layer flush prompt-guided with this many prompt rows, and with the key off")
    ap.add_argument("--out", default="", help="--prompt-rows: also write the result to this JSON file")
    a = ap.parse_args()
    if a.prompt_rows:
        return prompt_flush_bench(a.prompt_rows, min(a.iters, 5), a.out)
    dev = torch.device("cuda:0")
    td = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    Hq, Hkv, D, L = 28, 4, 128, a.L
    g = torch.Generator(device=dev).manual_seed(0)
    sets = [tuple((1.7 * torch.randn((1, h, L, D), generator=g, device=dev)).to(td) for h in (Hq, Hkv)) for _ in range(6)]
    cos = torch.rand((L, D), generator=g, device=dev)
    sin = (1 - cos * cos).sqrt()
    dt = nv.dtype_code(sets[0][0])
    if a.refround:
        dt = nv.RTK_BF16_REFROUND
    wsb = nv.lib.rtk_pivotkv_score_workspace_bytes(Hq, Hkv, L, D, dt)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
    wsp = (ws.data_ptr() + 255) & ~255
    score = torch.empty(L, dtype=torch.float32, device=dev)
    kun = torch.empty((Hkv, L, D), dtype=td, device=dev)
    st = nv.stream()

    def run(q, k):
        nv.check(nv.lib.rtk_pivotkv_score(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), k.stride(1), k.stride(2), Hq, Hkv,
                                          L, D, dt, nv.ptr(cos), nv.ptr(sin), 1.1386, nv.ptr(score), nv.ptr(kun),
                                          C.c_void_p(wsp), wsb, st), "score")
    if a.units:
        # the chunk-batched launches bench.py times: one launch per kernel over `units` prepared workspaces
        stride = (wsb + 255) & ~255
        big = torch.empty(a.units * stride + 256, dtype=torch.uint8, device=dev)
        base = (big.data_ptr() + 255) & ~255
        kuns = torch.empty((a.units, Hkv, L, D), dtype=td, device=dev)
        rs_n = C.c_int(0)
        pf = nv.lib.rtk_pivotkv_score_partials(Hq, Hkv, L, D, dt, C.byref(rs_n))
        parts = torch.empty((a.units, pf), dtype=torch.float32, device=dev)
        for u in range(a.units):
            q, k = sets[u % len(sets)]
            nv.check(nv.lib.rtk_pivotkv_score_stages(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), k.stride(1), k.stride(2),
                                                     Hq, Hkv, L, D, dt, nv.ptr(cos), nv.ptr(sin), 1.1386, nv.ptr(score),
                                                     nv.ptr(kuns[u]), C.c_void_p(base + u * stride), wsb, nv.SCORE_PREPARE,
                                                     None, st), "prepare")

        def runb():
            nv.check(nv.lib.rtk_pivotkv_score_passes_batched(C.c_void_p(base), stride, nv.ptr(kuns), Hkv * L * D * kuns.element_size(),
                                                             nv.ptr(parts), pf, a.units, Hq, Hkv, L, D, dt, None, None, st), "batched")
        for _ in range(2):
            runb()
        torch.cuda.synchronize()
        nv.lib.rtk_profile_reset()
        nv.lib.rtk_profile_enable(1)
        for _ in range(a.iters):
            runb()
        torch.cuda.synchronize()
        nv.lib.rtk_profile_enable(0)
        prof = nv.profile_read()
        flops = 2.0 * Hq * L * L * D * a.units
        for k, (n, ms) in prof.items():
            us = ms / n * 1e3
            extra = f"  {flops / (us * 1e-6) / 1e12:7.1f} TFLOP/s" if k.startswith("score_pass") else ""
            print(f"{k:16s} n={n:4d} avg={us:9.1f} us{extra}")
        G = Hq // Hkv
        if a.refround:   # per-head partials: the fingerprint below is for the default layout only
            return
        sc = (parts.view(a.units, Hkv, rs_n.value, L).sum(2) / G).mean(1)
        print("units", a.units, "score mean %.7f" % float(sc.mean()), "checksum %.9e" % float((sc.double() * torch.arange(1, L + 1, device=dev).double()).sum()))
        return
    for i in range(3):
        run(*sets[i % len(sets)])
    torch.cuda.synchronize()
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable(1)
    for i in range(a.iters):
        run(*sets[i % len(sets)])
    torch.cuda.synchronize()
    nv.lib.rtk_profile_enable(0)
    prof = nv.profile_read()
    flops = 2.0 * Hq * L * L * D
    for k, (n, ms) in prof.items():
        us = ms / n * 1e3
        extra = f"  {flops / (us * 1e-6) / 1e12:7.1f} TFLOP/s" if k.startswith("score_pass") else ""
        print(f"{k:16s} n={n:4d} avg={us:9.1f} us{extra}")
    print("score mean", float(score.mean()), "min", float(score.min()), "max", float(score.max()))


if __name__ == "__main__":
    main()

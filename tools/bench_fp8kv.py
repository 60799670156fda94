#!/usr/bin/env python
"""kv_cache_dtype="fp8_e4m3" against the 16-bit cache: memory and the cost of the flush, same inputs, same process.

    python tools/bench_fp8kv.py [--out profiles/fp8kv_memory.json] [--chunks 8] [--layers 28] [--geometry real|baseline|all]

Per geometry - real (Qwen2-VL 448 px: L 2304, keep 576) and BASELINE (L 6272, keep 1568), Hq 28 / Hkv 4 / D 128, bf16,
M-RoPE, reforge, key-patch mask - a 17-token text prefix and N chunks x `layers` layers go through
update_pre_rope + PivotKVCache.attention + after_forward, once per cache kind, each cache built with the reserves the
patched forwards pass (_prefill.cache_reserves).  Reported per kind: the allocator peak and what is held at the end (above
the resident inputs), memory_footprint(), milliseconds per chunk of after_forward (HIP events; score passes + selection +
eviction) and, from the library's per-kernel events, the eviction kernel alone: archive_units (reads 2 keep Hkv D s,
writes 2 keep Hkv (D + 4) per unit) against compact_units (4 keep Hkv D s), bytes / time as a fraction of 8 TB/s.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HQ, HKV, D, TEXT = 28, 4, 128, 17
SEC = [16, 24, 24]
HBM = 8e12
GEOMETRIES = {"real": 2304, "baseline": 6272}


def run(kind, L, layers, chunks, pool, tq, dev):
    import types

    import retake._native as nv
    import retake._prefill as pf
    import retake.longvideo_cache as lc
    import synth

    keep = L // 4
    top = {"kvcache_compression": True, "attention_kernel": "hip",
           "kvcache_compression_kwargs": {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    if kind == "fp8_e4m3":
        top["kv_cache_dtype"] = kind
    cfg = types.SimpleNamespace(hidden_size=HQ * D, num_hidden_layers=layers, num_attention_heads=HQ, num_key_value_heads=HKV,
                                longvideo_kwargs=top)
    rot = synth.RotaryStub(synth.inv_freq(D), synth.YARN_FACTOR4_ATTENTION_SCALING, device=dev)
    segs = [(0, TEXT, "text"), (TEXT, TEXT + chunks * L, "video")]
    reserves = pf.cache_reserves(cfg, segs[-1][1], L, segs)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    cache = lc.build_kvcache(cfg, **reserves)
    cache.kvcache_compression = False
    tp = torch.arange(TEXT, device=dev).view(1, 1, TEXT).expand(3, 1, TEXT).contiguous()
    for l in range(layers):
        assert cache.append_pre_rope(tq[0].clone(), tq[1], tq[2], l, tp.clone(), rot, SEC) is not None
    kname = "archive_units" if kind == "fp8_e4m3" else "compact_units"
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable_mask(1 << nv.profile_kernel_ids()[kname])
    flush_ms, call = [], 0
    for c in range(chunks):
        cache.kvcache_compression = True
        cache.keypatches_mask_chunk = torch.from_numpy(np.random.default_rng(c).uniform(size=L) < 0.3).to(dev)
        pos = torch.from_numpy(synth.mrope_position_ids(TEXT + (L // 64) * c, L // 64, 8, 8, hw0=TEXT)).to(dev)
        for l in range(layers):
            q, k, v = pool[call % len(pool)]
            call += 1
            out = cache.update_pre_rope(q.clone(), k, v, l, pos, rot, SEC)
            assert out is not None and cache.attention(*out, layer_idx=l) is not None
            del out
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cache.after_forward()
        b.record()
        b.synchronize()
        flush_ms.append(a.elapsed_time(b))
    cache.keypatches_mask_chunk = None
    del pos, tp, q, k, v
    torch.cuda.synchronize()
    prof = nv.profile_read().get(kname, (0, 0.0))
    nv.lib.rtk_profile_enable_mask(0)
    es = 2
    unit_bytes = 2 * keep * HKV * D * es + (2 * keep * HKV * (D + 4) if kind == "fp8_e4m3" else 2 * keep * HKV * D * es) + 2 * 3 * keep * 8
    us = prof[1] * 1e3 / max(1, prof[0])
    fp = cache.memory_footprint()
    nb = lambda t: 0 if t is None else t.numel() * t.element_size()   # noqa: E731
    res = {"kind": kind, "reserves": reserves, "allocator_peak_bytes": int(torch.cuda.max_memory_allocated() - base),
           "allocator_held_bytes": int(torch.cuda.memory_allocated() - base), "memory_footprint": fp,
           "kv_buffers_bytes": int(sum(nb(st.k) + nb(st.v) + nb(st.k8) + nb(st.v8) + nb(st.ks8) + nb(st.vs8) for st in cache._layers)),
           "flush_ms_per_chunk_median": statistics.median(flush_ms), "flush_ms_per_chunk": flush_ms,
           "eviction_kernel": {"name": kname, "launches": prof[0], "us_per_launch": us, "bytes_per_launch": unit_bytes * layers,
                               "fraction_of_8_TBs": (unit_bytes * layers / (us * 1e-6) / HBM) if us else None},
           "seq_length": cache.get_seq_length(0)}
    del cache
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8kv_memory.json"))
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--geometry", choices=("real", "baseline", "all"), default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp8kv.py needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "layers": args.layers, "chunks": args.chunks,
           "Hq": HQ, "Hkv": HKV, "D": D, "dtype": "bfloat16", "text_prefix": TEXT, "geometries": {}}
    for name, L in GEOMETRIES.items():
        if args.geometry not in ("all", name):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda n: tuple((1.7 * torch.randn((1, n, h, D), generator=g, device=dev)).to(torch.bfloat16).transpose(1, 2)  # noqa: E731
                             for h in (HQ, HKV, HKV))
        pool, tq = [mk(L) for _ in range(4)], mk(TEXT)
        row = {"L": L, "keep": L // 4}
        for kind in ("fp8_e4m3", "bf16"):
            row[kind] = run(kind, L, args.layers, args.chunks, pool, tq, dev)
            print(json.dumps({name: {kind: {k: v for k, v in row[kind].items() if k != "flush_ms_per_chunk"}}}), flush=True)
        row["kv_buffers_ratio"] = row["fp8_e4m3"]["kv_buffers_bytes"] / row["bf16"]["kv_buffers_bytes"]
        row["allocator_peak_ratio"] = row["fp8_e4m3"]["allocator_peak_bytes"] / row["bf16"]["allocator_peak_bytes"]
        doc["geometries"][name] = row
        del pool, tq
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("\n| geometry | cache | K/V buffers MiB | allocator peak MiB | held MiB | flush ms / chunk | eviction kernel us | of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for name, row in doc["geometries"].items():
        for kind in ("fp8_e4m3", "bf16"):
            r = row[kind]
            ek = r["eviction_kernel"]
            print(f"| {name} L {row['L']} | {kind} | {r['kv_buffers_bytes'] / 2**20:.0f} | {r['allocator_peak_bytes'] / 2**20:.0f} | "
                  f"{r['allocator_held_bytes'] / 2**20:.0f} | {r['flush_ms_per_chunk_median']:.3f} | {ek['us_per_launch']:.1f} | "
                  f"{(ek['fraction_of_8_TBs'] or 0):.2f} |")


if __name__ == "__main__":
    main()

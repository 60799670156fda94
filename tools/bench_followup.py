#!/usr/bin/env python3
"""A follow-up question on a prefilled video: rewind + append, against rebuilding the cache.

The reference prefills the video again for every question.  With PivotKVCache.rewind the second question costs what its
own rows cost: `rewind(video_end)` (host only), then per layer `append_pre_rope` of the question's rows and the native
attention over [compressed video | question].  Measured here at the cache level, one process, HIP events, on the same tree
in the same run:

    follow-up   rewind + 28 layers x (append_pre_rope of 64 rows + attention)
    rebuild     a fresh cache for the same video: 8 chunks x 28 layers x (update_pre_rope + attention) + the flushes -
                the existing path, as bench.py's `--pre-rope` loop drives it

at L 2304 (the real Qwen2-VL geometry) and L 6272 (BASELINE.json's).  The model's GEMMs are in neither number.

    python tools/bench_followup.py [--chunks 8 --rows 64 --repeat 20 --out profiles/followup_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)
import torch

import bench as B


def timed(fn):
    """(HIP-event ms, wall ms) of fn(), device idle before and after."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def measure(geometry, n_chunks, rows, repeat, dev, td):
    import retake.longvideo_cache as lc

    B.set_geometry(geometry)
    layers, L = B.LAYERS, B.FRAMES_PER_CHUNK * B.N_PATCH
    keep = max(1, int(B.RATIO * L))
    pool = [B.pool_set(i, dev, td, projection_layout=True) for i in range(4)]
    pos_base = [B.chunk_position_ids(c, dev) for c in range(n_chunks)]
    rotary = B.Rotary(dev)
    q_rot = torch.empty_like(pool[0][0])
    g = torch.Generator(device=dev).manual_seed(11)
    question = [tuple((1.7 * torch.randn((1, rows, h, B.D), generator=g, device=dev)).to(td).transpose(1, 2)
                      for h in (B.Hq, B.Hkv, B.Hkv)) for _ in range(4)]

    def build(attention=True):
        cfg = B.make_cache_config(layers)
        cfg.longvideo_kwargs["attention_kernel"] = "hip"
        cache = lc.build_kvcache(cfg, reserve_tokens=n_chunks * keep + L + 2048)
        call = 0
        for c in range(n_chunks):
            cache.kvcache_compression = True
            pos = pos_base[c].clone()
            for layer in range(layers):
                q, k, v = pool[call % len(pool)]
                call += 1
                out = cache.update_pre_rope(q, k, v, layer, pos, rotary, B.MROPE, query_out=q_rot)
                if out is None:
                    raise RuntimeError("update_pre_rope declined a video chunk of the benchmark geometry")
                if attention and cache.attention(*out, layer_idx=layer) is None:
                    raise RuntimeError("the native attention declined a chunk of the benchmark geometry")
            cache.after_forward()
        cache.kvcache_compression = False
        return cache

    holder = {}

    def rebuild(attention):
        holder.pop("cache", None)   # a rebuild starts from nothing, as a second `generate` does
        holder["cache"] = build(attention)

    rebuild(True)                   # warm-up: batch scratch, attention workspaces, the allocator
    res = {"geometry": geometry, "L": L, "chunks": n_chunks, "layers": layers, "question_rows": rows,
           "cache_rows_per_layer": n_chunks * keep}
    for name, attention in (("rebuild_ms", True), ("rebuild_without_attention_ms", False)):
        ev, wall = timed(lambda: rebuild(attention))
        res[name], res[name.replace("_ms", "_wall_ms")] = ev, wall
    cache = holder["cache"]
    mark = cache.video_end
    assert mark is not None and cache.get_seq_length(0) == n_chunks * keep
    last = int(cache.position_cache[0][0, 0, -1].item())
    ids = (torch.arange(rows, device=dev) + last + 1).view(1, 1, rows).expand(3, 1, rows).contiguous()

    def followup():
        cache.rewind(mark)
        pos = ids.clone()
        for layer in range(layers):
            q, k, v = question[layer % len(question)]
            out = cache.append_pre_rope(q.clone(), k, v, layer, pos, rotary, B.MROPE)
            if out is None or cache.attention(*out, layer_idx=layer) is None:
                raise RuntimeError("the follow-up path declined the question's rows")

    followup()
    pointers = [(st.k.data_ptr(), st.v.data_ptr(), st.pos.data_ptr()) for st in cache._layers]
    runs = [timed(followup) for _ in range(repeat)]
    assert pointers == [(st.k.data_ptr(), st.v.data_ptr(), st.pos.data_ptr()) for st in cache._layers]
    assert cache.get_seq_length(0) == n_chunks * keep + rows
    t0 = time.perf_counter()
    for _ in range(1000):
        cache.rewind(mark)
    res["rewind_host_us"] = (time.perf_counter() - t0) * 1e3
    res["followup_ms"] = statistics.median(r[0] for r in runs)
    res["followup_wall_ms"] = statistics.median(r[1] for r in runs)
    res["rebuild_over_followup"] = res["rebuild_ms"] / res["followup_ms"]
    holder.clear()
    del cache, pool, q_rot
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "followup_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    report = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "timer": "HIP events (wall clock beside them)",
              "what": "follow-up = rewind(video_end) + layers x (append_pre_rope + native attention); rebuild = a fresh cache "
                      "for the same video, chunks x layers x (update_pre_rope + native attention) + flushes",
              "cases": [measure(name, args.chunks, args.rows, args.repeat, dev, torch.bfloat16)
                        for name in ("qwen448", "baseline")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()

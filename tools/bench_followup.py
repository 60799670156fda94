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

--fork measures PivotKVCache.fork instead (no bar: the feature is a capability): the same follow-up on a branch forked at
`video_end` against the follow-up after `rewind` on the parent, and the allocator bytes of N = 1, 2, 4 live conversations
as N branches of one cache against N fresh caches.  Output: profiles/fork_bench.json.
"""
import argparse
import gc
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


class Workload:
    """One geometry's inputs and the two things done with them: prefill a fresh cache, ask a question of a cache."""

    def __init__(self, geometry, n_chunks, rows, dev, td):
        B.set_geometry(geometry)
        self.geometry, self.n_chunks, self.rows, self.dev = geometry, n_chunks, rows, dev
        self.layers, self.L = B.LAYERS, B.FRAMES_PER_CHUNK * B.N_PATCH
        self.keep = max(1, int(B.RATIO * self.L))
        self.pool = [B.pool_set(i, dev, td, projection_layout=True) for i in range(4)]
        self.pos_base = [B.chunk_position_ids(c, dev) for c in range(n_chunks)]
        self.rotary = B.Rotary(dev)
        self.q_rot = torch.empty_like(self.pool[0][0])
        g = torch.Generator(device=dev).manual_seed(11)
        self.question = [tuple((1.7 * torch.randn((1, rows, h, B.D), generator=g, device=dev)).to(td).transpose(1, 2)
                               for h in (B.Hq, B.Hkv, B.Hkv)) for _ in range(4)]
        self.ids = None

    def build(self, attention=True):
        import retake.longvideo_cache as lc

        cfg = B.make_cache_config(self.layers)
        cfg.longvideo_kwargs["attention_kernel"] = "hip"
        cache = lc.build_kvcache(cfg, reserve_tokens=self.n_chunks * self.keep + self.L + 2048)
        call = 0
        for c in range(self.n_chunks):
            cache.kvcache_compression = True
            pos = self.pos_base[c].clone()
            for layer in range(self.layers):
                q, k, v = self.pool[call % len(self.pool)]
                call += 1
                out = cache.update_pre_rope(q, k, v, layer, pos, self.rotary, B.MROPE, query_out=self.q_rot)
                if out is None:
                    raise RuntimeError("update_pre_rope declined a video chunk of the benchmark geometry")
                if attention and cache.attention(*out, layer_idx=layer) is None:
                    raise RuntimeError("the native attention declined a chunk of the benchmark geometry")
            cache.after_forward()
        cache.kvcache_compression = False
        if self.ids is None:
            last = int(cache.position_cache[0][0, 0, -1].item())
            self.ids = (torch.arange(self.rows, device=self.dev) + last + 1).view(1, 1, self.rows).expand(3, 1, self.rows).contiguous()
        return cache

    def ask(self, cache):
        """The question's rows through every layer of `cache` (a parent at `video_end`, or a branch forked there)."""
        pos = self.ids.clone()
        for layer in range(self.layers):
            q, k, v = self.question[layer % len(self.question)]
            out = cache.append_pre_rope(q.clone(), k, v, layer, pos, self.rotary, B.MROPE)
            if out is None or cache.attention(*out, layer_idx=layer) is None:
                raise RuntimeError("the follow-up path declined the question's rows")

    def header(self):
        return {"geometry": self.geometry, "L": self.L, "chunks": self.n_chunks, "layers": self.layers,
                "question_rows": self.rows, "cache_rows_per_layer": self.n_chunks * self.keep}


def measure(geometry, n_chunks, rows, repeat, dev, td):
    w = Workload(geometry, n_chunks, rows, dev, td)
    holder = {}

    def rebuild(attention):
        holder.pop("cache", None)   # a rebuild starts from nothing, as a second `generate` does
        holder["cache"] = w.build(attention)

    rebuild(True)                   # warm-up: batch scratch, attention workspaces, the allocator
    res = w.header()
    for name, attention in (("rebuild_ms", True), ("rebuild_without_attention_ms", False)):
        ev, wall = timed(lambda: rebuild(attention))
        res[name], res[name.replace("_ms", "_wall_ms")] = ev, wall
    cache = holder["cache"]
    mark = cache.video_end
    assert mark is not None and cache.get_seq_length(0) == n_chunks * w.keep

    def followup():
        cache.rewind(mark)
        w.ask(cache)

    followup()
    pointers = [(st.k.data_ptr(), st.v.data_ptr(), st.pos.data_ptr()) for st in cache._layers]
    runs = [timed(followup) for _ in range(repeat)]
    assert pointers == [(st.k.data_ptr(), st.v.data_ptr(), st.pos.data_ptr()) for st in cache._layers]
    assert cache.get_seq_length(0) == n_chunks * w.keep + rows
    t0 = time.perf_counter()
    for _ in range(1000):
        cache.rewind(mark)
    res["rewind_host_us"] = (time.perf_counter() - t0) * 1e3
    res["followup_ms"] = statistics.median(r[0] for r in runs)
    res["followup_wall_ms"] = statistics.median(r[1] for r in runs)
    res["rebuild_over_followup"] = res["rebuild_ms"] / res["followup_ms"]
    holder.clear()
    del cache, w
    torch.cuda.empty_cache()
    return res


def measure_fork(geometry, n_chunks, rows, repeat, dev, td):
    """--fork: the same follow-up on a BRANCH (PivotKVCache.fork at video_end, rewound to its own fork point between
    questions) against the parent after `rewind`, in one process; and what N live conversations hold in the allocator as
    N branches of one cache against N fresh caches."""
    w = Workload(geometry, n_chunks, rows, dev, td)
    cache = w.build(True)
    mark = cache.video_end
    res = w.header()

    def on_parent():
        cache.rewind(mark)
        w.ask(cache)

    branch = cache.fork(mark, reserve_tokens=rows + 64)
    root = branch.video_end

    def on_branch():
        branch.rewind(root)
        w.ask(branch)

    on_parent(), on_branch()
    runs = [(timed(on_parent), timed(on_branch)) for _ in range(repeat)]   # interleaved: both see the same machine state
    cache.rewind(mark)
    assert branch.get_seq_length(0) == n_chunks * w.keep + rows and cache.get_seq_length(0) == n_chunks * w.keep
    res["followup_after_rewind_ms"] = statistics.median(r[0][0] for r in runs)
    res["followup_on_branch_ms"] = statistics.median(r[1][0] for r in runs)
    res["followup_after_rewind_wall_ms"] = statistics.median(r[0][1] for r in runs)
    res["followup_on_branch_wall_ms"] = statistics.median(r[1][1] for r in runs)
    res["branch_over_rewind"] = res["followup_on_branch_ms"] / res["followup_after_rewind_ms"]
    del branch, root

    def held():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    base = held()
    res["one_cache_bytes"] = sum(t.numel() * t.element_size() for st in cache._layers for t in (st.k, st.v, st.pos))
    res["live_conversations"] = []
    for n in (1, 2, 4):
        branches = [cache.fork(mark, reserve_tokens=rows + 64) for _ in range(n)]
        for b in branches:
            w.ask(b)
        forked = held() - base
        del branches, b
        before = held()
        fresh = [w.build(True) for _ in range(n)]
        for c in fresh:
            w.ask(c)
        rebuilt = held() - before
        del fresh, c
        res["live_conversations"].append({"n": n, "branches_bytes": forked, "fresh_caches_bytes": rebuilt})
    del cache, w
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--fork", action="store_true", help="measure PivotKVCache.fork (see the module docstring)")
    ap.add_argument("--out", default=None, help="default: profiles/followup_bench.json, or profiles/fork_bench.json with --fork")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fork_bench.json" if args.fork else "followup_bench.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.fork:
        what = ("follow-up = layers x (append_pre_rope + native attention) of the question's rows: on a branch forked at "
                "video_end (rewound to its fork point first) against the parent after rewind(video_end), interleaved; "
                "live_conversations = torch.cuda.memory_allocated of n branches of one cache against n fresh caches, each "
                "having answered the question")
    else:
        what = ("follow-up = rewind(video_end) + layers x (append_pre_rope + native attention); rebuild = a fresh cache "
                "for the same video, chunks x layers x (update_pre_rope + native attention) + flushes")
    report = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "timer": "HIP events (wall clock beside them)",
              "what": what,
              "cases": [(measure_fork if args.fork else measure)(name, args.chunks, args.rows, args.repeat, dev, torch.bfloat16)
                        for name in ("qwen448", "baseline")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()

"""bench.py --gpus N  (strong scaling: one video, chunks sharded over the ranks; retake/sharded.py is the library).

The one module of the package that imports the bench script at the repository's root (its synthetic inputs, geometry and
report format): the step `bench.py --gpus N` times, the in-process check that it assembles the cache one GPU builds, the
timed run and its entry point.  `retake.sharded` forwards these four names, so `sharded.bench_main` keeps working.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from typing import Optional

import torch
import torch.distributed as dist

from .sharded import (_P2P, PhaseTimer, ShardedPivotKV, _gather_stack, _mark, disable_p2p, dpselect_sharded, enable_p2p,
                      shard_chunks)


def _rank_inputs(c0: int, c1: int, dev, dtype):
    """What the rank that owns chunks [c0, c1) feeds a step -> (frames [1, T_loc (+ the halo frame in front), N, C], has_halo,
    the chunks' base ids).  The synthetic inputs are functions of the chunk / update index (bench.chunk_frames,
    bench.pool_set), so every rank regenerates its share and any world size compresses the very same video."""
    import bench as B

    halo = c0 > 0 and c1 > c0
    parts = ([B.chunk_frames(c0 - 1, dev, dtype)[-1:]] if halo else []) + [B.chunk_frames(c, dev, dtype) for c in range(c0, c1)]
    frames = torch.cat(parts)[None] if parts else torch.empty((1, 0, B.N_PATCH, B.C_EMB), dtype=dtype, device=dev)
    return frames, halo, [B.chunk_position_ids(c, dev) for c in range(c0, c1)]


def sharded_video_step(frames, has_halo: bool, T: int, c0: int, c1: int, layers: int, pool, pos_base, rotary, overlap: bool,
                       group=None, state: Optional[dict] = None, inputs=None, pre_rope: bool = False):
    """One rank's share of one video (what `bench.py --gpus N` times and tests/mp_sharded_gpu.py checks): DPSelect on
    the rank's frames with the distance rows all-gathered, PivotKV on chunks [c0, c1) at provisional temporal ids, then
    offsets + cache assembly.  `overlap`: the rows a chunk kept leave in one asynchronous all-gather right after its
    flush (needs equally many chunks on every rank).  `state`: a dict the caller keeps between videos (the p2p
    transport reuses its mapped landing buffers through it).  `inputs(c, layer, pos) -> (q, k, v)`: the layer's rotated
    q / k at the ids `pos` the update will see (what a model produces; tests/mp_sharded_gpu.py rotates fixed contents
    with it).  Without it the resident pool set is taken AS the rotated input, whatever the ids: right for timing, but
    a later block then scores different content than the single-GPU run (its scores, kept set and K differ; sizes agree).
    `pre_rope`: `inputs` returns the PRE-RoPE projections and every update is the attention prologue
    (PivotKVCache.update_pre_rope): the scores never see the ids, so the sharded and the sequential run keep the same
    tokens in every dtype, and with the single rotation of `finalize` the same key bits.
    Returns (retained tokens of this rank, (keys, values, ids))."""
    import bench as B

    L = B.FRAMES_PER_CHUNK * B.N_PATCH
    phases = (state or {}).get("phases")     # a PhaseTimer the caller wants filled (bench.py --gpus N)
    if phases is not None:
        phases.begin()
    out, mask, idx, dis = dpselect_sharded(frames, has_halo, T, 3, sync=False, group=group)
    _mark(phases, "dpselect")
    keep = max(1, int(B.RATIO * L))
    sh = ShardedPivotKV(B.make_cache_config(layers), group=group, expected_rows=(c1 - c0) * keep if overlap else None,
                        chunk_gather=(state or {}).get("chunk_gather"), reserve_tokens=(c1 - c0) * keep + L)
    cache = sh.cache
    q_rot = None
    for ci, c in enumerate(range(c0, c1)):
        cache.keypatches_mask_chunk = mask[c * L:(c + 1) * L]
        cache.kvcache_compression = True
        pos = pos_base[ci].clone()
        for layer in range(layers):
            if pre_rope:
                q0, k0, v = inputs(c, layer, pos)
                if q_rot is None or q_rot.shape != q0.shape or q_rot.dtype != q0.dtype:
                    q_rot = torch.empty_like(q0)   # where the rotated queries go: one scratch per video, not one per update
                if cache.update_pre_rope(q0, k0, v, layer, pos, rotary, B.MROPE, query_out=q_rot) is None:
                    raise RuntimeError("update_pre_rope declined a video chunk of the sharded step")
                continue
            cache.shift_temporal_ids_(pos, layer)       # block-local ids start at 0 (provisional)
            q, k, v = pool[(c * layers + layer) % len(pool)] if inputs is None else inputs(c, layer, pos)
            cache.update(k, v, layer, {"query_states": q, "position_ids": pos, "rotary_emb": rotary,
                                       "mrope_section": B.MROPE, "shift_next_position_ids": True})   # as the Qwen2-VL patch does
        cache.after_forward()
        if overlap:
            sh.gather_chunk()   # this chunk's kept rows leave now, beside the next chunk's scoring
    _mark(phases, "blocks")
    keys, values, pos = sh.finalize(rotary.inv_freq, B.MROPE, assemble=True, phases=phases)
    if state is not None:
        state["chunk_gather"] = sh.chunk_gather
    return (c1 - c0) * layers * keep, (keys, values, pos)


def _verify_case(dname: str, n_chunks: int, rank: int, world: int, dev, rotary, layers: int, group, state: dict, log) -> dict:
    """One (dtype, chunk count) case of `verify_sharded_equals_sequential`: the sequential cache of the whole video, this
    rank's block through `sharded_video_step`, the comparison.  -> the case's entry of the summary."""
    import bench as B
    from . import longvideo_cache as lc
    from . import visual_compression as vc

    L = B.FRAMES_PER_CHUNK * B.N_PATCH
    keep = max(1, int(B.RATIO * L))
    td = B.TORCH_DTYPE[dname]
    T = n_chunks * B.FRAMES_PER_CHUNK
    pool = [B.pool_set(i, dev, td, projection_layout=True) for i in range(n_chunks * layers)]

    def inputs(c, l, pos):   # what q_proj / k_proj / v_proj hand the attention patch
        return pool[(c * layers + l) % len(pool)]

    frames_all = torch.cat([B.chunk_frames(c, dev, td) for c in range(n_chunks)])[None]
    _, mask = vc.memory_bank_compress_keyframe(frames_all, T, 3, sync=False)
    q_rot = torch.empty_like(pool[0][0])   # where the rotated queries go (one scratch per build)
    seq = lc.build_kvcache(B.make_cache_config(layers))
    seq.prologue_operands = "pre_rope"    # what the blocks score (ShardedPivotKV): operands that never see an id
    for c in range(n_chunks):
        seq.keypatches_mask_chunk = mask[c * L:(c + 1) * L]
        seq.kvcache_compression = True
        pos = B.chunk_position_ids(c, dev)
        for l in range(layers):
            q0, k0, v = inputs(c, l, pos)
            if seq.update_pre_rope(q0, k0, v, l, pos, rotary, B.MROPE, query_out=q_rot) is None:
                raise AssertionError("update_pre_rope declined a chunk of the sequential reference run")
        seq.after_forward()
    blocks = shard_chunks(n_chunks, world)
    c0, c1 = blocks[rank]
    even = len({b - a for a, b in blocks}) == 1
    fr, halo, pos_base = _rank_inputs(c0, c1, dev, td)
    _, (keys, values, pos) = sharded_video_step(fr, halo, T, c0, c1, layers, pool, pos_base, rotary, even, group=group,
                                                state=state, inputs=inputs, pre_rope=True)
    p2p = _P2P.get(group)
    if p2p is not None:
        p2p.check()   # a bounded wait that ran out is reported as that, not as the mismatch it leaves behind
    for l in range(layers):
        assert keys[l].shape[2] == n_chunks * keep, (keys[l].shape, n_chunks * keep)
        if not torch.equal(pos[l], seq.position_cache[l]):
            bad = (pos[l] != seq.position_cache[l]).reshape(-1, pos[l].shape[-1]).any(0).reshape(-1, keep).sum(1)
            raise AssertionError(f"rank {rank} layer {l} {dname}: ids differ; wrong ids per kept chunk {bad.tolist()}; first "
                                 f"rows {pos[l].reshape(-1, pos[l].shape[-1])[0, ::keep].tolist()} vs "
                                 f"{seq.position_cache[l].reshape(-1, pos[l].shape[-1])[0, ::keep].tolist()}")
        if not torch.equal(values[l], seq.value_cache[l]):   # say where: differing rows per kept chunk of the assembled rows
            rows = (values[l] != seq.value_cache[l]).any(dim=3).any(dim=1)[0].reshape(-1, keep).sum(1)
            raise AssertionError(f"rank {rank} layer {l} {dname}: V differs; wrong rows per kept chunk {rows.tolist()}; "
                                 f"NaN entries {int(torch.isnan(values[l].float()).sum())}, all-zero rows "
                                 f"{int((values[l] == 0).all(dim=3).all(dim=1).sum())}")
        if not torch.equal(keys[l], seq.key_cache[l]):   # say where: per kept chunk of the assembled rows
            d = (keys[l].float() - seq.key_cache[l].float()).abs().amax(dim=(0, 1, 3)).reshape(-1, keep).amax(dim=1)
            raise AssertionError(f"rank {rank} layer {l} {dname}: K differs; max |diff| per kept chunk {d.tolist()}")
    a = B.cache_checksum(keys, values, pos)
    b = B.cache_checksum([seq.key_cache[l] for l in range(layers)], [seq.value_cache[l] for l in range(layers)],
                         seq.position_cache)
    assert a["ids_sum"] == b["ids_sum"] and a["v_bits_sum"] == b["v_bits_sum"] and a["tokens_per_layer"] == b["tokens_per_layer"]
    assert a["k_abs_sum"] == b["k_abs_sum"]
    torch.cuda.synchronize(dev)
    dist.barrier(group=group)
    if log is not None and rank == 0:
        log(f"{dname}: chunks {n_chunks} on {world} rank(s): blocks {blocks}, overlapped gathers {even}: assembled == "
            f"sequential, bit for bit")
    return {"dtype": dname, "chunks": n_chunks, "blocks": blocks, "overlapped_gathers": even}


def verify_sharded_equals_sequential(rank: int, world: int, dev, rotary, layers: int = 2, chunk_counts=None,
                                     group=None, state: Optional[dict] = None, log=None, dtypes=("fp32", "bf16")) -> dict:
    """Equality of the sharded and the sequential compression, over the transport `group` is configured for (RCCL
    collectives, or the p2p pushes after `enable_p2p`) and through the very function `bench.py --gpus N` times
    (`sharded_video_step`), in the parity dtype AND in the dtype the bench times.  For every dtype and every chunk count
    in `chunk_counts` (default: 2 * world - even blocks, per-chunk overlapped gathers - and 2 * world + 1 - ragged blocks,
    padded assembly at the end) every rank

      * builds the SEQUENTIAL cache of the whole small video on its own (`layers` layers, bench.py's deterministic
        tensors as the pre-RoPE projections, through PivotKVCache.update_pre_rope at the ids a single-GPU run sees), then
      * compresses its block through `sharded_video_step` (same projections, the block's PROVISIONAL ids) and compares
        the ASSEMBLED cache with the sequential one: position ids exact, V exact, K EXACT - bit patterns, in bf16 too:
        the scores are computed from the un-rotated operands (they never see an id) and `finalize` rotates every kept
        key once, at its final id, with the tables and roundings the sequential flush uses.

    Raises AssertionError on any mismatch (on the rank that sees it); returns a summary dict."""
    state = {} if state is None else state
    chunk_counts = tuple(chunk_counts) if chunk_counts is not None else (2 * world, 2 * world + 1)
    cases = [_verify_case(dname, n_chunks, rank, world, dev, rotary, layers, group, state, log)
             for dname in dtypes for n_chunks in chunk_counts]
    # every rank passed its own comparison (a failing rank raised and took the job down with it); make it explicit
    ok = torch.ones(1, dtype=torch.int64, device=dev if dist.get_backend(group) != "gloo" else "cpu")
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
    assert int(ok.item()) == 1
    return {"equal": True, "dtype": list(dtypes), "layers": layers, "cases": cases, "max_rel_k_diff": 0.0,
            "checked": "assembled cache == sequential cache on every rank, pre-RoPE operands, one rotation at the final ids: "
                       "ids, V and K bit patterns equal in every listed dtype"}


def measure_sharded(args, rank: int, world: int, dev, transport: str, share: bool, steps: int, warmup: int,
                    verify: bool = True) -> Optional[dict]:
    """The timed sharded run on an initialised process group: -> the report dict on rank 0, None elsewhere.
    Besides the whole-job rate the report says where a step's time goes on the ranks (`phase_ms`: [max, min] over the
    ranks of the mean ms per step of each PhaseTimer phase, of the host's wall time per step and of the idle time at the
    closing barrier) - what the first real multi-GPU run needs to explain a shortfall."""
    import bench as B
    from . import _native as nv

    red_dev = torch.device("cpu") if share else dev     # gloo reduces host tensors
    p2p = _P2P.get(None)
    tdtype = B.TORCH_DTYPE[args.dtype]
    T = args.frames
    n_chunks = T // B.FRAMES_PER_CHUNK
    L = B.FRAMES_PER_CHUNK * B.N_PATCH
    blocks = shard_chunks(n_chunks, world)
    c0, c1 = blocks[rank]
    even = len({b - a for a, b in blocks}) == 1     # else: padded assembly at the end instead of per-chunk gathers
    frames, halo, pos_base = _rank_inputs(c0, c1, dev, tdtype)
    pool = [B.pool_set(i, dev, tdtype) for i in range(min(args.pool, n_chunks * args.layers))]
    rotary = B.Rotary(dev)

    state = {}

    def step():
        return sharded_video_step(frames, halo, T, c0, c1, args.layers, pool, pos_base, rotary, even, state=state)

    # communicator set-up (RCCL builds its rings / the p2p scratch is mapped on the first exchange) is not part of a step:
    # run one tiny exchange before anything is timed, whatever --warmup says
    _gather_stack(torch.zeros(4, dtype=torch.int64, device=dev))
    # Before anything is timed: is the cache this transport assembles the cache one GPU builds?  (tests/mp_sharded_gpu.py's
    # check, in process, over the transport of the timed loop.)  A mismatch raises: no value is printed for a wrong path.
    verdict = None
    if verify:
        verdict = verify_sharded_equals_sequential(rank, world, dev, rotary, layers=2, state=state)
        torch.cuda.empty_cache()
    for _ in range(warmup):
        step()
    ids = nv.profile_kernel_ids()   # HIP events around the dominant kernels, on their launch stream, in the timed region
    nv.check(nv.lib.rtk_profile_reset(), "profile_reset")
    nv.check(nv.lib.rtk_profile_enable_mask((1 << ids["score_pass1"]) | (1 << ids["score_pass2"])), "profile_enable")
    phases = state["phases"] = PhaseTimer(dev)
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    retained = 0
    for _ in range(steps):
        r, (keys, values, pos) = step()
        retained += r
    torch.cuda.synchronize()
    t_done = time.perf_counter()
    dist.barrier()
    torch.cuda.synchronize()
    t_end = time.perf_counter()
    state.pop("phases")
    dt = torch.tensor([t_end - t0], dtype=torch.float64, device=red_dev)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    tot = torch.tensor([float(retained)], dtype=torch.float64, device=red_dev)
    dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    dt = float(dt.item())
    nv.check(nv.lib.rtk_profile_enable(0), "profile_enable")
    kern = {k: {"launches": n, "avg_us": ms / n * 1e3, "total_ms": ms} for k, (n, ms) in nv.profile_read().items()}
    # per-phase times of this rank (mean per step) -> [max, min] over the ranks
    pm = phases.per_step_ms()
    pm["finalize"] = pm["offsets"] + pm["rotate"] + pm["assembly"]
    pm["host_wall"] = (t_done - t0) / steps * 1e3
    pm["barrier_idle"] = (t_end - t_done) / steps * 1e3
    names = sorted(pm)
    hi = torch.tensor([pm[k] for k in names], dtype=torch.float64, device=red_dev)
    lo = hi.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    phase_ms = {k: [float(f"{a:.4g}"), float(f"{b:.4g}")] for k, a, b in zip(names, hi.tolist(), lo.tolist())}
    # untimed; the token count equals the N = 1 line's, the sums only at N = 1 (see sharded_video_step on `inputs`)
    checksum = B.cache_checksum(keys, values, pos) if rank == 0 else None
    if p2p is not None:
        p2p.check()   # a bounded wait that gave up would have left garbage: fail the run instead
    if rank != 0:
        return None
    return {
        "metric": "frames/sec through DPSelect+PivotKV @2048 frames; retained-KV-tokens/sec",
        "value": T * steps / dt, "unit": "frames/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": dt / steps * 1e3, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "retained_kv_tokens_per_s": float(tot.item()) / dt,
        "config": {"workload": f"BASELINE configs[3]: {T}-frame video sharded by frame chunk over {world} GPU(s), "
                               f"{n_chunks} chunks x {args.layers} layers, L={L}",
                   "workload_detail": f"Qwen2-VL-7B geometry: DPSelect (distance rows all-gathered) + PivotKV 4x; offsets + "
                                      f"whole-cache all-gather over "
                                      f"{('RCCL' if transport == 'rccl' else 'gloo, host-staged (tests)') if p2p is None else 'direct xGMI pushes (retake/p2p.py)'}",
                   "frames": T, "chunks": n_chunks, "layers": args.layers, "chunk_tokens": L,
                   "parallelism": f"chunk-sharded x{world}", "transport": transport,
                   "assembled_cache_tokens": int(keys[0].shape[2])},
        "cache_checksum": checksum,
        # untimed, before the timed region, over the same transport and through the same function the loop times
        "sharded_equals_sequential": bool(verdict and verdict["equal"]),
        "sharded_check": verdict,
        ("rccl_world_size" if transport == "rccl" else ("p2p_world_size" if p2p is not None else "host_staged_world_size")):
            dist.get_world_size(),
        "cpu_baseline": None,   # timed on rank 0 of the N = 1 run only (bench contract); see that line
        "kernels_timed_region_rank0": kern,
        "roofline": B.score_roofline(kern, args.dtype, L, T, (c1 - c0) * args.layers * steps),
        # [max, min] over the ranks, mean ms per step: PhaseTimer phases on the launch stream (dpselect: local distances +
        # all-gather + select; blocks: the rank's chunks x layers incl. starting the per-chunk gathers; offsets: the id scan;
        # rotate: kept keys at their final ids; assembly: waiting for / gathering the other ranks' rows; finalize = the
        # last three), the host's wall time per step and the idle time at the closing barrier
        "phase_ms": phase_ms,
        "phase_bytes_rank0": dict(phases.bytes),
    }


def bench_main(args, rank: int, world: int, local_rank: int):
    import bench as B

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")   # world size 1 without a launcher (RETAKE_FORCE_SHARDED=1)
    os.environ.setdefault("MASTER_PORT", "29544")
    transport = getattr(args, "transport", "rccl")
    # RETAKE_BENCH_SHARE_GPU=1 (tests only): every rank runs on GPU 0 over a gloo control plane, so that the multi-rank bench
    # path can run on a 1-GPU box (RCCL refuses two ranks on one device) - with the p2p transport as the data plane, or
    # (`--transport host`) with the collective-transport code path (ChunkGather, all_gather_caches) staged through the host
    share = os.environ.get("RETAKE_BENCH_SHARE_GPU") == "1" and transport in ("p2p", "host")
    if transport == "host" and not share:
        raise SystemExit("--transport host is the tests' form of the collective path (RETAKE_BENCH_SHARE_GPU=1); use rccl or p2p")
    dev = torch.device("cuda", 0 if share else local_rank)
    torch.cuda.set_device(dev)
    if not dist.is_initialized():
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    p2p = enable_p2p(device=dev) if transport == "p2p" else None
    out = measure_sharded(args, rank, world, dev, transport, share, args.steps, args.warmup,
                          verify=not getattr(args, "no_self_check", False))
    dist.barrier()
    if p2p is not None:
        disable_p2p()
    dist.destroy_process_group()
    if rank == 0:
        # RCCL writes its version banner to stdout through C stdio, which a pipe only sees at exit - after anything
        # Python printed.  Flush it out first so that the JSON line is the last line of rank 0's stdout.
        try:
            C.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        B.emit(out, getattr(args, "report", None))

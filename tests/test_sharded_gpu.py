"""The chunk-sharded prefill (retake/sharded.py and the modules behind it) on the GPU: the numerics of the block fix-up in
one process, the frame exchange of the sharded DPSelect, the ranks over every transport (p2p and host-staged collectives
with all ranks on GPU 0, RCCL on min(2, visible GPUs) ranks) and `bench.py --gpus N` end to end.  World size 8:
tests/test_00_world8_gpu.py; the host logic over gloo: tests/test_sharded_cpu.py.
"""
import numpy as np
import pytest
import torch

import proc_util
import synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------
# multi-GPU sharding, numerics of the block fix-up (single process, blocks run one after the other)
# ---------------------------------------------------------------------------------------------------
def test_sharded_blocks_reproduce_sequential_cache():
    """Two blocks compressed independently from provisional temporal id 0, then shifted by R(delta), must
    equal one cache that saw all chunks in order: same kept indices and ids, V identical, K within 1e-5."""
    import bench as B
    from retake import sharded

    _single_rank_group()
    layers, n_chunks, gh, gw, gpc = 2, 4, 8, 8, 4
    L = gpc * gh * gw
    inv_f = synth.inv_freq(B.D)
    rot = synth.RotaryStub(inv_f, B.A_SCALE, device=dev())
    cfg = B.make_cache_config(layers)
    cfg.longvideo_kwargs["kvcache_compression_kwargs"]["native_rope"] = False
    data = {}
    for c in range(n_chunks):
        for l in range(layers):
            q0, k0, v = synth.qkv_chunk(7000 + 10 * c + l, B.Hq, B.Hkv, L, B.D)
            data[c, l] = tuple(torch.from_numpy(a).to(dev()) for a in (q0, k0, v))
    masks = [torch.from_numpy(np.random.default_rng(c).uniform(size=L) < 0.3).to(dev()) for c in range(n_chunks)]

    def run(cache, chunks):
        for c in chunks:
            cache.keypatches_mask_chunk = masks[c]
            cache.kvcache_compression = True
            for l in range(layers):
                q0, k0, v = data[c, l]
                pos = torch.from_numpy(synth.mrope_position_ids(40 + gpc * c, gpc, gh, gw, hw0=3)).to(dev())
                prev = cache.get_prev_temporal_idx(l)
                pos[0, 0, :] += (prev + 1) - pos[0, 0, 0]
                q = synth.rope_forward(q0, pos, rot, B.MROPE)
                k = synth.rope_forward(k0, pos, rot, B.MROPE)
                cache.update(k, v, l, {"query_states": q, "position_ids": pos, "rotary_emb": rot,
                                       "mrope_section": B.MROPE})
            cache.after_forward()

    import retake.longvideo_cache as lc

    seq = lc.build_kvcache(cfg)
    run(seq, range(n_chunks))
    a = sharded.ShardedPivotKV(cfg, first_start=0)
    run(a.cache, [0, 1])
    ka, va, pa = a.finalize(torch.from_numpy(inv_f), B.MROPE, assemble=False)
    b = sharded.ShardedPivotKV(cfg, first_start=torch.stack([p[0, 0, -1] for p in pa]) + 1)
    run(b.cache, [2, 3])
    kb, vb, pb = b.finalize(torch.from_numpy(inv_f), B.MROPE, assemble=False)
    for l in range(layers):
        k_all = torch.cat([ka[l], kb[l]], dim=2)
        v_all = torch.cat([va[l], vb[l]], dim=2)
        p_all = torch.cat([pa[l], pb[l]], dim=-1)
        assert torch.equal(p_all, seq.position_cache[l])
        assert torch.equal(v_all, seq.value_cache[l])
        assert (k_all - seq.key_cache[l]).abs().max().item() <= 1e-5


def test_sharded_overlapped_assembly_equals_assembly_at_the_end():
    """ShardedPivotKV.gather_chunk (one asynchronous all-gather per chunk, segments rotated to their temporal
    position afterwards) must return the very cache finalize() assembles at the end - world size 1 through RCCL."""
    import bench as B
    from retake import sharded

    _single_rank_group()
    layers, n_chunks, gh, gw, gpc = 2, 3, 8, 8, 4
    L = gpc * gh * gw
    inv_f = synth.inv_freq(B.D)
    rot = synth.RotaryStub(inv_f, B.A_SCALE, device=dev())
    cfg = B.make_cache_config(layers)
    cfg.longvideo_kwargs["kvcache_compression_kwargs"]["native_rope"] = False
    data = {}
    for c in range(n_chunks):
        for l in range(layers):
            q0, k0, v = synth.qkv_chunk(9000 + 10 * c + l, B.Hq, B.Hkv, L, B.D)
            data[c, l] = tuple(torch.from_numpy(a).to(dev()).bfloat16() for a in (q0, k0, v))

    def run(overlap):
        sh = sharded.ShardedPivotKV(cfg, first_start=57)
        cache = sh.cache
        for c in range(n_chunks):
            cache.keypatches_mask_chunk = None
            cache.kvcache_compression = True
            pos = torch.from_numpy(synth.mrope_position_ids(0, gpc, gh, gw, hw0=3)).to(dev())
            for l in range(layers):
                q0, k0, v = data[c, l]
                cache.shift_temporal_ids_(pos, l)
                q = synth.rope_forward(q0.float(), pos, rot, B.MROPE).bfloat16()
                k = synth.rope_forward(k0.float(), pos, rot, B.MROPE).bfloat16()
                cache.update(k, v, l, {"query_states": q, "position_ids": pos, "rotary_emb": rot, "mrope_section": B.MROPE})
            cache.after_forward()
            if overlap:
                sh.gather_chunk()
        return sh.finalize(torch.from_numpy(inv_f), B.MROPE, assemble=True)

    ka, va, pa = run(False)
    kb, vb, pb = run(True)
    for l in range(layers):
        assert ka[l].shape == kb[l].shape and torch.equal(ka[l], kb[l])
        assert torch.equal(va[l], vb[l]) and torch.equal(pa[l], pb[l])
        assert int(pa[l][0, 0, 0]) >= 57


def _single_rank_group():
    import torch.distributed as dist

    if not dist.is_initialized():
        import os

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())


@pytest.mark.parametrize("route,dtype", [("pre_rope", torch.float32), ("pre_rope", torch.bfloat16), ("update", torch.float32)])
def test_sharded_blocks_reproduce_sequential_cache_plain_rope(route, dtype):
    """The LLaVA protocol (plain RoPE, ids [1, L], no mrope_section; tests/mp_sharded_gpu.py's plain_rope_* geometry: L 640,
    keep 63 at the non-dyadic ratio 0.0996, key-patch masks at a rate of 0.05): five chunks compressed as two blocks (2, 3)
    from provisional id 0 and finalized at first_start = 19 / block 0's last id + 1 must equal the video rows of one cache
    that saw a 19-token text segment and then all chunks in order.  Through the attention prologue on pre-RoPE projections
    (fp32, bf16): ids, V and K bit-equal - the contract verify_sharded_equals_sequential states for M-RoPE; through `update`
    on rotated fp32 tensors: ids and V exact, K within 1e-5 (the M-RoPE twin's bar).  The sequential ids are also compared
    with rope_ref's reforging formula on the kept indices, so the comparison is not purely self-referential."""
    import mp_sharded_gpu as mp
    import rope_ref as rr
    from retake import sharded

    _single_rank_group()
    d = dev()
    rot = mp.plain_rope_rotary(d)
    inv = torch.from_numpy(synth.inv_freq(mp.PLAIN_D))
    extra = {"native_rope": False} if route == "update" else {}
    L, keep, text, last_layer = mp.PLAIN_L, mp.PLAIN_KEEP, mp.PLAIN_TEXT, mp.PLAIN_LAYERS - 1
    kept = []     # the last layer's kept indices, per chunk
    seq = mp.plain_rope_sequential(5, dtype, d, rot, route,
                                   after_chunk=lambda cache, c: kept.append(cache.last_keep_indices.cpu().long()), **extra)
    assert seq.position_cache[0].shape == (1, text + 5 * keep)
    # independent: the last layer's ids are the reforged ids of the kept tokens of consecutive ids continuing the previous chunk
    start = text
    for c, idx in enumerate(kept):
        assert idx.numel() == keep and bool((idx[1:] > idx[:-1]).all())
        want = rr.reforge_ids(start + idx, keep, L)
        got = seq.position_cache[last_layer][0, text + c * keep:text + (c + 1) * keep].cpu()
        assert torch.equal(got, want), (c, got.tolist(), want.tolist())
        start = int(want[-1]) + 1
    a = sharded.ShardedPivotKV(mp.plain_rope_config(**extra), first_start=text)
    mp.plain_rope_feed(a.cache, [0, 1], dtype, d, rot, route)
    ka, va, pa = a.finalize(inv, None, assemble=False)
    b = sharded.ShardedPivotKV(mp.plain_rope_config(**extra), first_start=torch.stack([p[0, -1] for p in pa]) + 1)
    mp.plain_rope_feed(b.cache, [2, 3, 4], dtype, d, rot, route)
    kb, vb, pb = b.finalize(inv, None, assemble=False)
    for l in range(mp.PLAIN_LAYERS):
        k_all, v_all, p_all = torch.cat([ka[l], kb[l]], dim=2), torch.cat([va[l], vb[l]], dim=2), torch.cat([pa[l], pb[l]], dim=-1)
        assert p_all.shape == (1, 5 * keep) and torch.equal(p_all, seq.position_cache[l][:, text:])
        assert torch.equal(v_all, seq.value_cache[l][:, :, text:])
        if route == "pre_rope":
            assert torch.equal(k_all, seq.key_cache[l][:, :, text:])
        else:
            assert (k_all - seq.key_cache[l][:, :, text:]).abs().max().item() <= 1e-5


def test_sharded_overlapped_assembly_equals_assembly_at_the_end_plain_rope():
    """The plain-RoPE twin of test_sharded_overlapped_assembly_equals_assembly_at_the_end (3 chunks, bf16, first_start 57):
    gather_chunk + finalize(assemble=True) - ONE launch of rtk_rope_rotate_rows over the assembled cache with P = 1 - must
    return, bit for bit, the cache finalize() assembles at the end."""
    import mp_sharded_gpu as mp
    from retake import sharded

    _single_rank_group()
    d = dev()
    rot = mp.plain_rope_rotary(d)
    inv = torch.from_numpy(synth.inv_freq(mp.PLAIN_D))

    def run(overlap):
        sh = sharded.ShardedPivotKV(mp.plain_rope_config(), first_start=57)
        mp.plain_rope_feed(sh.cache, range(3), torch.bfloat16, d, rot, after_chunk=(lambda cache, c: sh.gather_chunk()) if overlap else None)
        if overlap:
            assert sh._gather is not None and sh._gather.rows() == 3 * mp.PLAIN_KEEP
        return sh.finalize(inv, None, assemble=True)

    ka, va, pa = run(False)
    kb, vb, pb = run(True)
    for l in range(mp.PLAIN_LAYERS):
        assert ka[l].shape == kb[l].shape == (1, mp.PLAIN_HKV, 3 * mp.PLAIN_KEEP, mp.PLAIN_D) and torch.equal(ka[l], kb[l])
        assert torch.equal(va[l], vb[l]) and torch.equal(pa[l], pb[l])
        # the first stored id is the block's start + the index of the first kept token (reforging keeps the minimum)
        assert pa[l].shape == (1, 3 * mp.PLAIN_KEEP) and 57 <= int(pa[l][0, 0]) < 57 + mp.PLAIN_L
        assert bool((pa[l][0, 1:] >= pa[l][0, :-1]).all())


def test_sharded_finalize_of_a_block_that_saw_no_chunk():
    """A rank whose block is empty (a video with fewer chunks than ranks) holds a cache that never saw an update: `finalize`
    must not raise on it - at world size 1 there is nobody to learn the geometry from and the result is an empty cache."""
    import mp_sharded_gpu as mp
    from retake import sharded

    _single_rank_group()
    inv = torch.from_numpy(synth.inv_freq(mp.PLAIN_D))
    for assemble in (False, True):
        sh = sharded.ShardedPivotKV(mp.plain_rope_config(), first_start=7)
        keys, values, pos = sh.finalize(inv, None, assemble=assemble)
        assert len(keys) == len(values) == len(pos)
        assert all(t.shape[-2] == 0 for t in list(keys) + list(values)) and all(p.shape[-1] == 0 for p in pos)


@pytest.mark.parametrize("sync", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dpselect_sharded_ratio_below_one_matches_single_gpu(sync, dtype):
    """World size 1 through the real collective path: select on the gathered distances, padded block,
    all-gather, placement gather - must equal the unsharded call bit for bit."""
    import retake.visual_compression as vc
    from retake import sharded

    _single_rank_group()
    T, N, C, t = 48, 6, 256, 17
    x = torch.from_numpy(synth.frames_video(321, T, N, C)).to(dev()).to(dtype)     # [1, T, N, C]
    ref_out, ref_mask = vc.memory_bank_compress_keyframe(x, t, 3, sync=sync)
    out, mask, idx, dis = sharded.dpselect_sharded(x, False, t, 3, sync=sync)
    assert out.shape == (1, t, N, C) and torch.equal(out, ref_out) and torch.equal(mask, ref_mask)
    # ratio 1.0 still returns the rank's own frames
    out1, mask1, idx1, _ = sharded.dpselect_sharded(x, False, T, 3, sync=sync)
    assert torch.equal(out1, x) and mask1.numel() == T * N


@pytest.mark.parametrize("sync", [True, False])
def test_dpselect_frame_exchange_emulated_ranks(sync):
    """Four ranks emulated on one device, every gather through rtk_gather_frames: local kept frames -> padded
    blocks (concatenated as the all-gather would) -> placement == the global gather of the unsharded call."""
    import retake._native as nv
    import retake.visual_compression as vc
    from retake import sharded

    T, N, C, t, world = 64, 5, 128, 23, 4
    xb = torch.from_numpy(synth.frames_video(99, T, N, C)).to(dev()).bfloat16()    # [1, T, N, C]
    ref_out, _, idx, _, _ = vc.dpselect_stages(xb, t, 3, sync)
    x = xb[0]
    T_own = T // world
    _, cmax, local, place = sharded.plan_frame_exchange(idx, T_own, world)
    st, dt = nv.stream(), nv.dtype_code(x)
    blocks = torch.empty((world * cmax, N, C), dtype=x.dtype, device=dev())
    for r in range(world):
        own = x[r * T_own:(r + 1) * T_own].contiguous()
        mine = local[r, :, 0].contiguous() if sync else local[r].contiguous()
        blk = blocks[r * cmax:(r + 1) * cmax]
        nv.check(nv.lib.rtk_gather_frames(nv.ptr(own), T_own, N, C, dt, nv.ptr(mine), cmax, int(sync), nv.ptr(blk), st),
                 "rtk_gather_frames")
    plc = place[:, 0].contiguous() if sync else place
    out = torch.empty((1, t, N, C), dtype=x.dtype, device=dev())
    nv.check(nv.lib.rtk_gather_frames(nv.ptr(blocks), world * cmax, N, C, dt, nv.ptr(plc), t, int(sync), nv.ptr(out), st),
             "rtk_gather_frames")
    assert torch.equal(out, ref_out)


def test_sharded_multi_rank_rccl():
    """The chunk-sharded path on min(2, visible GPUs) ranks over RCCL (tests/mp_sharded_gpu.py): assembled cache ==
    sequential cache (ids exact, V exact, K <= 1e-5) for an even and a ragged chunk split.  On a 1-GPU box this still
    drives the whole path through RCCL at world size 1; with >= 2 GPUs it is the first multi-rank run of the collectives."""
    r = proc_util.launch_ranks("mp_sharded_gpu.py", min(2, torch.cuda.device_count()))
    assert r.returncode == 0 and "MP_SHARDED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("world", [2, 3])
def test_p2p_allgather_processes(world):
    """retake/p2p.py over the C ABI (rtk_p2p_*): two / three processes map each other's landing buffers through hipIpc handles
    and push into them - all_gather of odd-sized / empty / growing payloads over 40 epochs, strided pushes into a final
    layout, and the bounded wait reporting a sender that never arrives.  All ranks share GPU 0 (same protocol and
    kernels as across GPUs; the stores just do not cross an xGMI link - test_p2p_across_gpus does that where it can)."""
    r = proc_util.launch_ranks("mp_p2p_gpu.py", world, env={"RETAKE_TEST_ONE_GPU": "1"})
    assert r.returncode == 0 and "MP_P2P_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ranks_over_p2p(world):
    """The chunk-sharded path at WORLD SIZE 2 and 3 with the p2p transport (tests/mp_sharded_gpu.py, RETAKE_TEST_TRANSPORT=p2p):
    distance rows, counts, temporal offsets, per-chunk pushes of the kept rows into their final position (landing buffers
    reused over four videos) and the ragged assembly at the end; assembled cache == sequential cache on every rank.
    Unlike RCCL, the p2p transport lets the ranks share one GPU, so this runs on the 1-GPU test box.  (World size 8:
    tests/test_00_world8_gpu.py.)"""
    r = proc_util.launch_ranks("mp_sharded_gpu.py", world, env={"RETAKE_TEST_TRANSPORT": "p2p", "RETAKE_TEST_ONE_GPU": "1"})
    assert r.returncode == 0 and "MP_SHARDED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_plain_rope_ranks_over_p2p(world):
    """The plain-RoPE (LLaVA protocol, ids [1, L]) sharded prefill at world size 2 and 3 over the p2p transport, all ranks on
    GPU 0 (tests/mp_sharded_gpu.py plain_rope_blocks): even blocks with per-chunk pushes, ragged blocks with the padded
    assembly, and world - 1 chunks - one rank's block is empty and takes part in every exchange with zero rows; assembled
    video rows == sequential cache on every rank, bit for bit, fp32 and bf16."""
    r = proc_util.launch_ranks("mp_sharded_gpu.py", world, env={"RETAKE_TEST_TRANSPORT": "p2p", "RETAKE_TEST_ONE_GPU": "1",
                                                       "RETAKE_TEST_ONLY_MORE_CASES": "1", "RETAKE_TEST_PLAIN_ROPE": "1"})
    assert r.returncode == 0 and "MP_SHARDED_PLAIN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("plain RoPE") == 6 and f"chunks {world - 1} on {world} rank(s)" in r.stdout


def test_sharded_plain_rope_two_ranks_collective_code_path_host_staged():
    """The same at world size 2 through the COLLECTIVE-transport code path (`ChunkGather`, `all_gather_caches`,
    `all_gather_ids` with [1, n] ids, `exchange_temporal_offsets` with a -1 row), every exchange staged through the host."""
    r = proc_util.launch_ranks("mp_sharded_gpu.py", 2, env={"RETAKE_TEST_TRANSPORT": "host", "RETAKE_TEST_ONE_GPU": "1",
                                                   "RETAKE_TEST_ONLY_MORE_CASES": "1", "RETAKE_TEST_PLAIN_ROPE": "1"})
    assert r.returncode == 0 and "MP_SHARDED_PLAIN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("plain RoPE") == 6 and "chunks 1 on 2 rank(s)" in r.stdout
    assert "overlapped gathers True" in r.stdout and "overlapped gathers False" in r.stdout


def test_sharded_plain_rope_multi_rank_rccl():
    """... and on min(2, visible GPUs) ranks over RCCL (world size 1 on a 1-GPU box: the path through the collectives)."""
    world = min(2, torch.cuda.device_count())
    r = proc_util.launch_ranks("mp_sharded_gpu.py", world, env={"RETAKE_TEST_ONLY_MORE_CASES": "1", "RETAKE_TEST_PLAIN_ROPE": "1"})
    assert r.returncode == 0 and "MP_SHARDED_PLAIN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("plain RoPE") == (6 if world >= 2 else 4)


def test_p2p_across_gpus():
    """The same two scripts with one rank per GPU (needs >= 2 visible GPUs): the pushes cross xGMI links."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one visible GPU: the p2p stores cannot cross a link here")
    world = min(n, 4)
    r = proc_util.launch_ranks("mp_p2p_gpu.py", world)
    assert r.returncode == 0 and "MP_P2P_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    r = proc_util.launch_ranks("mp_sharded_gpu.py", world, env={"RETAKE_TEST_TRANSPORT": "p2p"})
    assert r.returncode == 0 and "MP_SHARDED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_bench_two_ranks_share_one_gpu_p2p(tmp_path):
    """`bench.py --gpus 2 --transport p2p` end to end (rank start-up, halo frame, chunk blocks, timed loop, JSON line) with
    both ranks on GPU 0 (RETAKE_BENCH_SHARE_GPU=1: gloo control plane, p2p data plane), on a
    256-frame / 2-layer video.  The assembled cache must have the single-GPU run's size; its CONTENT is not comparable
    (the bench takes its resident tensors as the rotated inputs at whatever ids a block runs at, i.e. later blocks see
    different content - equality of sharded and sequential caches is tests/mp_sharded_gpu.py's job)."""
    common = ["--frames", "256", "--layers", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"]
    a, ra = proc_util.bench_line(common + ["--no-extras"], tmp_path, "one")
    b, rb = proc_util.bench_line(["--gpus", "2", "--transport", "p2p"] + common, tmp_path, "two", env={"RETAKE_BENCH_SHARE_GPU": "1"})
    assert b["n_gpus"] == 2 and b["scaling"] == "strong" and b["config"]["transport"] == "p2p"
    assert b["metric"] == a["metric"] and b["unit"] == a["unit"] and b["value"] > 0
    for key in ("tokens_per_layer", "layers"):
        assert rb["cache_checksum"][key] == ra["cache_checksum"][key], (key, ra["cache_checksum"], rb["cache_checksum"])
    assert b["config"]["assembled_cache_tokens"] == ra["cache_checksum"]["tokens_per_layer"]
    assert b["roofline"]["frac"] > 0 and b["cpu_baseline"] is None
    # the line carries its own proof: sharded == sequential was checked in process, over the same transport, before timing
    assert b["sharded_equals_sequential"] is True and b["p2p_world_size"] == 2
    assert [(c["dtype"], c["chunks"]) for c in rb["sharded_check"]["cases"]] == [("fp32", 4), ("fp32", 5), ("bf16", 4), ("bf16", 5)]
    # per-phase timing of the sharded step, max / min over the ranks (the first real multi-GPU run must say where time goes)
    for ph in ("dpselect", "blocks", "finalize", "step"):
        assert b["phase_ms"][ph][0] >= b["phase_ms"][ph][1] >= 0.0, b["phase_ms"]


def test_bench_two_ranks_collective_code_path_host_staged(tmp_path):
    """`bench.py --gpus 2 --transport host`: the COLLECTIVE-transport code path of the sharded step - `ChunkGather` (one
    all-gather per chunk beside the next chunk's scoring), `all_gather_caches`, the offsets scan, what an RCCL run executes -
    with two ranks on GPU 0, every exchange staged through the host over gloo (RCCL refuses two ranks on one device; the
    p2p tests never enter these functions).  Self-verified in process (even and ragged splits, fp32 and bf16) before timing."""
    common = ["--frames", "256", "--layers", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"]
    b, rb = proc_util.bench_line(["--gpus", "2", "--transport", "host"] + common, tmp_path, "host2", env={"RETAKE_BENCH_SHARE_GPU": "1"})
    assert b["n_gpus"] == 2 and b["config"]["transport"] == "host" and b["host_staged_world_size"] == 2 and b["value"] > 0
    assert b["sharded_equals_sequential"] is True
    assert [(c["dtype"], c["chunks"], c["overlapped_gathers"]) for c in rb["sharded_check"]["cases"]] == \
        [("fp32", 4, True), ("fp32", 5, False), ("bf16", 4, True), ("bf16", 5, False)]
    assert b["config"]["assembled_cache_tokens"] == 8 * 1568
    assert b["phase_ms"]["assembly"][0] > 0 and rb["phase_bytes_rank0"]["assembly_rows_received"] > 0


def test_sharded_prefill_two_ranks_collective_code_path_host_staged():
    """tests/mp_sharded_gpu.py with RETAKE_TEST_TRANSPORT=host at world size 2 on one GPU: assembled == sequential, bit for bit,
    through `ChunkGather` / `all_gather_caches` / `all_gather_ids` (the functions the RCCL transport runs)."""
    r = proc_util.launch_ranks("mp_sharded_gpu.py", 2, env={"RETAKE_TEST_TRANSPORT": "host", "RETAKE_TEST_ONE_GPU": "1", "RETAKE_TEST_DPSELECT": "1"})
    assert r.returncode == 0 and "MP_SHARDED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "overlapped gathers True" in r.stdout and "overlapped gathers False" in r.stdout


def test_bench_forced_sharded_world1_rccl_self_verifies(tmp_path):
    """`RETAKE_FORCE_SHARDED=1 python bench.py`: the sharded path at world size 1 over RCCL.  The line must carry
    `sharded_equals_sequential: true` (checked in process before the timed region) and - world size 1 being the one
    case where the bench's resident tensors mean the same thing in both paths - the plain run's cache fingerprint."""
    common = ["--frames", "256", "--layers", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"]
    a, ra = proc_util.bench_line(common + ["--no-extras"], tmp_path, "one")
    b, rb = proc_util.bench_line(common, tmp_path, "forced", env={"RETAKE_FORCE_SHARDED": "1", "MASTER_ADDR": "127.0.0.1",
                                                    "MASTER_PORT": str(proc_util.free_port())})
    assert b["sharded_equals_sequential"] is True and b["rccl_world_size"] == 1
    assert [(c["dtype"], c["chunks"]) for c in rb["sharded_check"]["cases"]] == [("fp32", 2), ("fp32", 3), ("bf16", 2), ("bf16", 3)]
    for key in ("tokens_per_layer", "layers", "ids_sum", "v_bits_sum"):
        assert rb["cache_checksum"][key] == ra["cache_checksum"][key], (key, ra["cache_checksum"], rb["cache_checksum"])
    assert abs(rb["cache_checksum"]["k_abs_sum"] - ra["cache_checksum"]["k_abs_sum"]) <= 1e-6 * ra["cache_checksum"]["k_abs_sum"]
    assert set(b["phase_ms"]) >= {"dpselect", "blocks", "offsets", "rotate", "assembly", "finalize", "step", "barrier_idle"}



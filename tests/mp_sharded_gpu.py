#!/usr/bin/env python3
"""Multi-rank GPU check of the chunk-sharded path, launched by tests/test_sharded_gpu.py::test_sharded_multi_rank_rccl as
    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P tests/mp_sharded_gpu.py
Every rank compresses its block of one small synthetic video (bench.py's deterministic tensors as the pre-RoPE
projections, through the attention prologue at the block's provisional ids) with retake.sharded_bench.sharded_video_step - RCCL
all-gathers of the distance rows, the temporal offsets and the compressed cache - and compares the assembled cache with
the cache the same rank builds sequentially on its own: ids, V and K bit patterns equal, in fp32 and in bf16.  Two shapes
per dtype: chunks divisible by the world size (per-chunk overlapped gathers) and one chunk more (ragged blocks, padded
assembly at the end).  Prints MP_SHARDED_OK on rank 0.

RETAKE_TEST_TRANSPORT=p2p runs the same check over the direct peer-to-peer pushes of retake/p2p.py with a gloo control
plane and rank r on GPU r % device_count - two ranks can then share the one GPU of a test box (RCCL refuses that) - and
repeats the even case so that the landing buffers of the per-chunk pushes are reused across videos.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import torch.distributed as dist


def dpselect_blocks(rank, world, dev):
    """DPSelect sharded by frame block over the live transport: every rank holds 12 frames (+ the halo frame in front of its
    block), the distance rows are all-gathered, the selection runs redundantly, and at ratio < 1 the kept frames are
    exchanged - output and key-patch mask must equal the unsharded call on the whole video, sync and per-patch, fp32 and
    bf16, ratio 1 and ~1/3."""
    import numpy as np

    import retake.visual_compression as vc
    import synth
    from retake import sharded

    per, N, C = 12, 6, 256
    T = per * world
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.from_numpy(synth.frames_video(500 + world, T, N, C)).to(dev).to(dtype)     # [1, T, N, C], same on every rank
        f0 = rank * per
        local = x[:, max(f0 - 1, 0):f0 + per].contiguous()
        for sync in (True, False):
            for t in (T, T // 3 + 1):
                ref_out, ref_mask = vc.memory_bank_compress_keyframe(x, t, 3, sync=sync)
                out, mask, idx, dis = sharded.dpselect_sharded(local, rank > 0, t, 3, sync=sync)
                assert torch.equal(mask, ref_mask), (str(dtype), sync, t, "mask")
                want = ref_out if t < T else x[:, f0:f0 + per]
                assert out.shape == want.shape and torch.equal(out, want), (str(dtype), sync, t, "frames")
    torch.cuda.synchronize(dev)
    dist.barrier()
    if rank == 0:
        print(f"sharded DPSelect over {world} ranks (halo frames, distance rows gathered, frame exchange at ratio < 1) == unsharded",
              flush=True)


# ---------------------------------------------------------------------------------------------------
# plain RoPE (the LLaVA protocol: ids [1, L], no mrope_section) - shared with the in-process tests of tests/test_hip_parity.py
# ---------------------------------------------------------------------------------------------------
PLAIN_HQ, PLAIN_HKV, PLAIN_D, PLAIN_L, PLAIN_LAYERS = 28, 4, 128, 640, 2     # L 640: the smallest family the prologue takes
PLAIN_RATIO, PLAIN_KEEP = 0.0996, 63                                          # non-dyadic: the id reforging truncates
PLAIN_TEXT = 19                                                               # text tokens in front of the video


def plain_rope_config(layers=PLAIN_LAYERS, **extra):
    import types

    kw = {"compression_ratio": PLAIN_RATIO, "compression_method": "pivotkv", "pos_embed_reforge": True}
    kw.update(extra)
    return types.SimpleNamespace(hidden_size=PLAIN_HQ * PLAIN_D, num_hidden_layers=layers, num_attention_heads=PLAIN_HQ,
                                 num_key_value_heads=PLAIN_HKV,
                                 longvideo_kwargs={"kvcache_compression": True, "kvcache_compression_kwargs": kw})


def plain_rope_rotary(dev):
    import synth

    return synth.RotaryStub(synth.inv_freq(PLAIN_D), synth.YARN_FACTOR4_ATTENTION_SCALING, device=dev)


def plain_rope_inputs(c, layer, dtype, dev):
    """Pre-RoPE q, k and v of (chunk, layer): a function of the two alone, so every rank regenerates them."""
    import synth

    return tuple(torch.from_numpy(a).to(dev).to(dtype) for a in synth.qkv_chunk(31000 + 10 * c + layer, PLAIN_HQ, PLAIN_HKV,
                                                                               PLAIN_L, PLAIN_D))


def plain_rope_mask(c, dev):
    """Key-patch mask of chunk c at a rate of 0.05: fewer masked tokens than `keep`, so the scores decide the rest."""
    import numpy as np

    m = np.random.default_rng(500 + c).uniform(size=PLAIN_L) < 0.05
    assert 0 < int(m.sum()) < PLAIN_KEEP, int(m.sum())
    return torch.from_numpy(m).to(dev)


def plain_rope_text(cache, dtype, dev):
    """A 19-token text segment in front of the video (compression off): the video's ids then start at 19."""
    cache.kvcache_compression = False
    pos = torch.arange(PLAIN_TEXT, device=dev)[None]
    g = torch.Generator().manual_seed(77)
    for layer in range(PLAIN_LAYERS):
        kt, vt = (torch.randn((1, PLAIN_HKV, PLAIN_TEXT, PLAIN_D), generator=g).to(dev).to(dtype) for _ in range(2))
        cache.update(kt, vt, layer, {"position_ids": pos})


def plain_rope_feed(cache, chunks, dtype, dev, rotary, route="pre_rope", after_chunk=None):
    """Video chunks `chunks` through `cache` (a PivotKVCache): route "pre_rope" = the attention prologue on the pre-RoPE
    projections, "update" = PivotKVCache.update on tensors rotated at the continuity-shifted ids."""
    import synth

    for c in chunks:
        cache.keypatches_mask_chunk = plain_rope_mask(c, dev)
        cache.kvcache_compression = True
        pos = (torch.arange(PLAIN_L, device=dev) + 40 + c * PLAIN_L)[None].contiguous()      # [1, L] token positions
        for layer in range(PLAIN_LAYERS):
            q0, k0, v = plain_rope_inputs(c, layer, dtype, dev)
            if route == "pre_rope":
                if cache.update_pre_rope(q0, k0, v, layer, pos, rotary, None) is None:
                    raise AssertionError("update_pre_rope declined a plain-RoPE video chunk")
            else:
                cache.shift_temporal_ids_(pos, layer)
                q, k = synth.rope_forward(q0, pos, rotary), synth.rope_forward(k0, pos, rotary)
                cache.update(k, v, layer, {"query_states": q, "position_ids": pos, "rotary_emb": rotary, "mrope_section": None})
        cache.after_forward()
        if after_chunk is not None:
            after_chunk(cache, c)


def plain_rope_sequential(n_chunks, dtype, dev, rotary, route="pre_rope", after_chunk=None, **cfg_extra):
    """The cache of one GPU that saw the text segment and then every chunk in order."""
    import retake.longvideo_cache as lc

    seq = lc.build_kvcache(plain_rope_config(**cfg_extra))
    if route == "pre_rope":
        seq.prologue_operands = "pre_rope"     # what the blocks score (ShardedPivotKV): operands that never see an id
    plain_rope_text(seq, dtype, dev)
    plain_rope_feed(seq, range(n_chunks), dtype, dev, rotary, route, after_chunk)
    return seq


def plain_rope_blocks(rank, world, dev):
    """The plain-RoPE sharded prefill over the live transport, driving ShardedPivotKV directly: `update_pre_rope` on this
    rank's chunks at provisional ids, `gather_chunk` on even splits, `finalize(assemble=True)` - and, on every rank, the
    sequential cache of the whole video (text prefix of 19 tokens): ids, V and K of the assembled video rows bit-equal, in
    fp32 and bf16.  Chunk counts: 2 * world (even blocks, per-chunk gathers), 2 * world + 1 (ragged blocks, padded
    assembly) and world - 1 (one rank's block is EMPTY: it takes part in every exchange with zero rows)."""
    import synth
    from retake import sharded

    rotary = plain_rope_rotary(dev)
    inv = torch.from_numpy(synth.inv_freq(PLAIN_D))
    state = None
    for dname, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for n_chunks in (2 * world, 2 * world + 1) + ((world - 1,) if world >= 2 else ()):
            seq = plain_rope_sequential(n_chunks, dtype, dev, rotary)
            blocks = sharded.shard_chunks(n_chunks, world)
            c0, c1 = blocks[rank]
            even = len({b - a for a, b in blocks}) == 1
            sh = sharded.ShardedPivotKV(plain_rope_config(), first_start=PLAIN_TEXT,
                                        expected_rows=(c1 - c0) * PLAIN_KEEP if even else None, chunk_gather=state)
            plain_rope_feed(sh.cache, range(c0, c1), dtype, dev, rotary,
                            after_chunk=(lambda cache, c: sh.gather_chunk()) if even else None)
            keys, values, pos = sh.finalize(inv, None, assemble=True, attention_scaling=rotary.attention_scaling)
            state = sh.chunk_gather
            p2p = sharded._P2P.get(None)
            if p2p is not None:
                p2p.check()   # a bounded wait that ran out is reported as that, not as the mismatch it leaves behind
            rows = n_chunks * PLAIN_KEEP
            for layer in range(PLAIN_LAYERS):
                what = f"rank {rank} {dname} chunks {n_chunks} layer {layer}"
                assert keys[layer].shape == (1, PLAIN_HKV, rows, PLAIN_D) and keys[layer].dtype == dtype, (what, keys[layer].shape)
                assert pos[layer].shape == (1, rows), (what, pos[layer].shape)
                assert torch.equal(pos[layer], seq.position_cache[layer][:, PLAIN_TEXT:]), what + ": ids differ"
                assert torch.equal(values[layer], seq.value_cache[layer][:, :, PLAIN_TEXT:]), what + ": V differs"
                assert torch.equal(keys[layer], seq.key_cache[layer][:, :, PLAIN_TEXT:]), what + ": K differs"
            torch.cuda.synchronize(dev)
            dist.barrier()
            if rank == 0:
                print(f"plain RoPE {dname}: chunks {n_chunks} on {world} rank(s): blocks {blocks}, overlapped gathers {even}: "
                      f"assembled == sequential, bit for bit", flush=True)
            del seq, sh, keys, values, pos
    if rank == 0:
        print("MP_SHARDED_PLAIN_OK", flush=True)


def main():
    import bench as B
    from retake import sharded
    from retake.sharded_bench import verify_sharded_equals_sequential

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if os.environ.get("RETAKE_TEST_POISON") == "1":
        # debugging aid: every torch.empty / empty_like of the process starts as NaN (floats) / a sentinel (ints), so a read
        # of memory nobody wrote shows up in the comparison instead of depending on what the allocator handed out
        real_empty, real_like = torch.empty, torch.empty_like

        def poison(t):
            if t.is_cuda and t.numel():
                if t.dtype.is_floating_point:
                    t.fill_(float("nan"))
                elif t.dtype in (torch.int64, torch.int32):
                    t.fill_(-77)
                elif t.dtype == torch.uint8:
                    t.fill_(0xA5)
            return t

        torch.empty = lambda *a, **k: poison(real_empty(*a, **k))
        torch.empty_like = lambda *a, **k: poison(real_like(*a, **k))
    p2p = os.environ.get("RETAKE_TEST_TRANSPORT") == "p2p"
    dev = torch.device("cuda", 0 if os.environ.get("RETAKE_TEST_ONE_GPU") == "1"
                       else int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if p2p:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        sharded.enable_p2p(device=dev)
    elif os.environ.get("RETAKE_TEST_TRANSPORT") == "host":
        # debugging aid: no device-side transport at all (no RCCL, no peer mapping) - every exchange staged through the host
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    # the comparison itself lives in the library (bench.py --gpus N runs it before its timed region as well)
    counts = (2 * world, 2 * world + 1) + ((2 * world, 2 * world, 2 * world) if p2p else ())
    if os.environ.get("RETAKE_TEST_ONLY_MORE_CASES") == "1":
        counts = ()
    state = {}
    res = verify_sharded_equals_sequential(rank, world, dev, B.Rotary(dev), layers=2, chunk_counts=counts,
                                           state=state, log=lambda m: print(m, flush=True))
    assert res["equal"] and len(res["cases"]) == 2 * len(counts) and (not counts or {c["dtype"] for c in res["cases"]} == {"fp32", "bf16"})
    # RETAKE_TEST_MORE_CASES="bf16:64,65": further chunk counts per dtype (world size 8: BASELINE's 64-chunk video in blocks
    # of 8 chunks, and the ragged 65-chunk split)
    for spec in filter(None, os.environ.get("RETAKE_TEST_MORE_CASES", "").split(";")):
        dname, cc = spec.split(":")
        cc = tuple(int(x) for x in cc.split(","))
        for one in cc:
            res = verify_sharded_equals_sequential(rank, world, dev, B.Rotary(dev), layers=2, chunk_counts=(one,), state=state,
                                                   log=lambda m: print(m, flush=True), dtypes=(dname,))
            assert res["equal"] and len(res["cases"]) == 1
    if os.environ.get("RETAKE_TEST_DPSELECT") == "1":
        dpselect_blocks(rank, world, dev)
    if os.environ.get("RETAKE_TEST_PLAIN_ROPE") == "1":
        plain_rope_blocks(rank, world, dev)
    if p2p:
        sharded.disable_p2p()
    dist.destroy_process_group()
    if rank == 0:
        print("MP_SHARDED_OK", flush=True)


if __name__ == "__main__":
    main()

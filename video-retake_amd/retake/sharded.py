"""One long video sharded over the GPUs of a node (BASELINE.json configs[3]).

One process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI; "gloo" in the CPU tests).
The video's frame chunks are split into contiguous blocks, one per rank:

  DPSelect   every rank computes the distance rows of its frames (one halo frame on the left), the
             [T, N] distance matrix is all-gathered (T*N*4 bytes, 1.6 MB at 2048x196), and the cheap
             stencil + top-k runs redundantly on every rank — deterministic, so all ranks hold the
             same indices and key-patch mask.  Frame gather: at ratio 1.0 (the shipped default) every
             frame stays in place; at ratio < 1 a rank gathers the kept frames it owns into a padded
             block, the blocks are all-gathered, and one more gather puts them in output order
             (`plan_frame_exchange`: kept indices ascend, so a rank's frames are one run per patch).
  PivotKV    (chunk, layer) scoring only reads the chunk's own q/k (longvideo_cache.py:264), so a rank
             runs `PivotKVCache.update` on its chunks with PROVISIONAL temporal ids starting at 0.
             Selection and the id rescale are translation invariant; the only coupling between blocks
             is the temporal offset of a block = last compressed temporal id of the previous block + 1
             (qwen2_vl.py:68-73).  `finalize` all-gathers one int64 per (rank, layer), takes the
             exclusive prefix, rotates each rank's kept keys by R(delta) (RoPE composes:
             R(p + delta) = R(delta) R(p)), shifts the stored ids, and (optionally) all-gathers the
             kept K / V / ids so every rank holds the full compressed cache.

No collective sits inside the scoring path; the exchanges are one small all-gather per video
(distances), one tiny all-gather per video (offsets) and, for the cache assembly, either two all-gathers per
video (K and V of every layer in one, the ids in the other) or - `gather_chunk` - one asynchronous all-gather per
chunk that overlaps the next chunk's scoring, plus the ids at the end.

Transport: `torch.distributed` collectives (RCCL) by default.  `enable_p2p(group)` switches every device-side exchange
of that group to the direct peer-to-peer pushes of retake/p2p.py (`rtk_p2p_*`: mapped peer buffers, one hop on every
xGMI link at once, no ring); with it `gather_chunk` pushes a chunk's kept rows straight into their final position of
every rank's assembled cache, so `finalize` has nothing left to copy.

Where the rest lives (the names are re-exported here):
    _shard_transport  the transport switch (_P2P, enable_p2p), `_gather_stack` - the one collective, the only place that
                      looks at the backend -, gather_counts, the all_gather_* assemblies, and the host-side index
                      arithmetic: shard_chunks, exchange_temporal_offsets, plan_frame_exchange
    _chunk_gather     ChunkGather, ChunkGatherP2P: a chunk's kept rows leave beside the next chunk's scoring
    sharded_bench     `bench.py --gpus N`: sharded_video_step, verify_sharded_equals_sequential, measure_sharded, bench_main -
                      the one module of the package that imports the bench script; reached from here on first use
"""
from __future__ import annotations

import ctypes as C
import time
from typing import List, Optional

import torch
import torch.distributed as dist

from ._chunk_gather import ChunkGather, ChunkGatherP2P
from ._shard_transport import (_P2P, _gather_stack, _p2p_for, all_gather_caches, all_gather_cat, all_gather_ids,  # noqa: F401
                               all_gather_rows, all_gather_rows_ragged, disable_p2p, enable_p2p, exchange_temporal_offsets,
                               gather_counts, plan_frame_exchange, shard_chunks)

_BENCH = ("sharded_video_step", "verify_sharded_equals_sequential", "measure_sharded", "bench_main")

__all__ = ["_P2P", "enable_p2p", "disable_p2p", "gather_counts", "all_gather_cat", "all_gather_rows", "all_gather_rows_ragged",
           "all_gather_caches", "all_gather_ids", "shard_chunks", "exchange_temporal_offsets", "plan_frame_exchange",
           "ChunkGather", "ChunkGatherP2P", "PhaseTimer", "ShardedPivotKV", "dpselect_sharded", *_BENCH]


def __getattr__(name):
    """bench.py calls `sharded.bench_main`: the bench driver's names are forwarded, its module imported on first use."""
    if name in _BENCH:
        from . import sharded_bench

        return getattr(sharded_bench, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class PhaseTimer:
    """Where a sharded step spends its time, per rank: marks on the CURRENT stream (HIP events on a GPU, the host clock
    under gloo), one list per step.  A phase is the span between two consecutive marks as the launch stream sees it, so
    it includes what that stream waited for (a collective, the side stream's pushes, a host round trip that left it
    idle).  `sharded_video_step` marks  dpselect | blocks | offsets | rotate | assembly;  read `per_step_ms()` after a
    device synchronisation."""

    ORDER = ("dpselect", "blocks", "offsets", "rotate", "assembly")

    def __init__(self, device):
        self.cuda = torch.device(device).type == "cuda"
        self.steps: List[list] = []
        self.bytes = {}

    def begin(self):
        self.steps.append([])
        self.mark("start")

    def mark(self, name: str):
        if not self.steps:
            return
        if self.cuda:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.steps[-1].append((name, e))
        else:
            self.steps[-1].append((name, time.perf_counter()))

    def note_bytes(self, name: str, n: int):
        self.bytes[name] = int(n)

    def per_step_ms(self) -> dict:
        """{phase: mean ms per step} over the recorded steps (+ "step": start -> last mark)."""
        tot = {k: 0.0 for k in self.ORDER}
        tot["step"] = 0.0
        n = 0
        for marks in self.steps:
            if len(marks) < 2:
                continue
            n += 1
            for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
                tot[name] = tot.get(name, 0.0) + (a.elapsed_time(b) if self.cuda else (b - a) * 1e3)
            a, b = marks[0][1], marks[-1][1]
            tot["step"] += a.elapsed_time(b) if self.cuda else (b - a) * 1e3
        return {k: v / max(1, n) for k, v in tot.items()}


def _mark(phases, name):
    if phases is not None:
        phases.mark(name)


# ---------------------------------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------------------------------
def dpselect_sharded(frames_local: torch.Tensor, has_halo: bool, tgt_mem_len: int, window_size: int = 3,
                     sync: bool = False, group=None):
    """frames_local [1, T_loc (+1 halo frame in front), N, C]; every rank holds the same number of own frames.
    Returns (compressed, mask_flat_global, idx_global, dis_global).  At ratio 1.0 (tgt_mem_len == total frames)
    `compressed` is the rank's own frames [1, T_loc, N, C]; at ratio < 1 it is the full compressed bank
    [1, tgt_mem_len, N, C], assembled on every rank from one all-gather of the kept frames."""
    from . import _native as nv

    nv.require_device(frames_local)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    x = frames_local[0].contiguous()
    Tl, N, Cc = x.shape
    dev = x.device
    dt = nv.dtype_code(x)
    with torch.cuda.device(dev):
        st = nv.stream()
        dis_l = torch.empty((Tl, N), dtype=torch.float32, device=dev)
        nv.check(nv.lib.rtk_dpselect_dis(nv.ptr(x), Tl, N, Cc, dt, nv.ptr(dis_l), st), "rtk_dpselect_dis")
        own = dis_l[1:] if has_halo else dis_l      # the halo frame only feeds the first own row
        counts = gather_counts(own.shape[0], dev, group)
        dis = all_gather_rows_ragged(own.contiguous(), group, counts)
        T = dis.shape[0]
        t = int(tgt_mem_len)
        if not 1 <= t <= T:
            raise ValueError(f"sharded DPSelect: tgt_mem_len {t} outside [1, {T}]")
        idx = torch.empty((t,) if sync else (t, N), dtype=torch.int64, device=dev)
        mask = torch.empty((t, N), dtype=torch.bool, device=dev)   # key-patch mask of the kept frames
        keys = torch.empty((2, T) if sync else (N, T), dtype=torch.float32, device=dev)
        nv.check(nv.lib.rtk_dpselect_select(nv.ptr(dis), T, N, t, int(window_size), int(bool(sync)), nv.ptr(idx),
                                            nv.ptr(mask), nv.ptr(keys), st), "rtk_dpselect_select")
        own_x = (x[1:] if has_halo else x).contiguous()
        T_own = own_x.shape[0]
        f0 = sum(counts[:rank])                      # first global frame of this rank
        if t == T:
            # ratio 1.0: every frame is kept at its own index -> the local output is a copy of the own frames
            idx_l = (idx[f0:f0 + T_own] - f0).contiguous()
            out = torch.empty((1, T_own, N, Cc), dtype=x.dtype, device=dev)
            nv.check(nv.lib.rtk_gather_frames(nv.ptr(own_x), T_own, N, Cc, dt, nv.ptr(idx_l), T_own,
                                              int(bool(sync)), nv.ptr(out), st), "rtk_gather_frames")
            return out, mask.flatten(), idx, dis
        # ratio < 1: own kept frames -> padded block -> all-gather -> output order
        if len(set(counts)) != 1:
            raise ValueError(f"sharded DPSelect at ratio < 1 needs equally many frames per rank, got {counts}")
        _, cmax, local, place = plan_frame_exchange(idx, T_own, world)
        mine = local[rank, :, 0].contiguous() if sync else local[rank].contiguous()
        block = torch.empty((cmax, N, Cc), dtype=x.dtype, device=dev)
        nv.check(nv.lib.rtk_gather_frames(nv.ptr(own_x), T_own, N, Cc, dt, nv.ptr(mine), cmax, int(bool(sync)),
                                          nv.ptr(block), st), "rtk_gather_frames")
        blocks = all_gather_rows(block, group)                       # [world * cmax, N, C] in rank order
        plc = place[:, 0].contiguous() if sync else place
        out = torch.empty((1, t, N, Cc), dtype=x.dtype, device=dev)
        nv.check(nv.lib.rtk_gather_frames(nv.ptr(blocks), world * cmax, N, Cc, dt, nv.ptr(plc), t, int(bool(sync)),
                                          nv.ptr(out), st), "rtk_gather_frames")
    return out, mask.flatten(), idx, dis


def _rotator(inv_freq: torch.Tensor, mrope_section: Optional[List[int]], attention_scaling: float, dev):
    """-> rotate(k, layer_stride, head_stride, n_layers, Hkv, rows, D, ids, ids_layer_stride, ids_row_stride, P): one
    `rtk_rope_rotate_rows` launch on `dev`'s current stream - the rows of `k` (elements from k's first one: layers, heads
    and rows at these strides), in place, at the ids `ids` [.., P, rows]."""
    from . import _native as nv

    sec = (C.c_int * len(mrope_section))(*mrope_section) if mrope_section else None
    nsec = len(mrope_section) if mrope_section else 0
    st = nv.stream()
    inv = inv_freq.to(device=dev, dtype=torch.float32).contiguous()

    def rotate(k, layer_stride, head_stride, n_layers, Hkv, rows, D, ids, ids_layer_stride, ids_row_stride, P):
        nv.check(nv.lib.rtk_rope_rotate_rows(nv.ptr(k), layer_stride, head_stride, n_layers, Hkv, rows, D, nv.dtype_code(k),
                                             nv.ptr(ids), ids_layer_stride, ids_row_stride, P, nv.ptr(inv), attention_scaling,
                                             sec, nsec, nv.round_mode(k.dtype), st), "rtk_rope_rotate_rows")

    return rotate


class ShardedPivotKV:
    """A rank's share of one video's PivotKV compression (see the module docstring)."""

    def __init__(self, config, group=None, first_start: int = 0, expected_rows: Optional[int] = None,
                 chunk_gather: Optional[ChunkGatherP2P] = None, reserve_tokens: Optional[int] = None):
        """expected_rows: rows this rank will keep per layer over the whole video (equal on all ranks); with the p2p
        transport it lets `gather_chunk` push rows to their final position (else the assembly happens at the end).
        chunk_gather: the ChunkGatherP2P of the previous video of the same shape, to reuse its mapped buffers."""
        from .longvideo_cache import PivotKVCache

        self.cache = PivotKVCache(config, reserve_tokens=reserve_tokens)   # capacity hint: kept rows + one chunk
        # the kept keys stay un-rotated (ids provisional) until `finalize` knows the block's temporal offset and rotates
        # them ONCE at their final ids - the same single rotation the sequential cache applies (reference :297-306)
        self.cache.defer_rerotation = bool(self.cache.pos_embed_reforge)
        # ... and the attention prologue scores the PRE-RoPE operands: the reference's own operands carry the rounding of a
        # rotation / un-rotation round trip at the chunk's FINAL ids (longvideo_cache.py:248-259), which a block does not
        # know before the offset scan - q0 / k0 never see an id, so every rank keeps what a single GPU with
        # prologue_operands="pre_rope" keeps, bit for bit, in every dtype
        self.cache.prologue_operands = "pre_rope"
        self.group = group
        self.first_start = first_start
        self.expected_rows = expected_rows
        self.chunk_gather = chunk_gather
        self._gather = None
        self._seen: List[int] = []

    def update(self, key_states, value_states, layer_idx, cache_kwargs):
        """PivotKVCache.update on this rank's block.  NOT attention-ready: while the re-rotation is deferred the
        returned keys are [un-rotated kept prefix | rotated current chunk] (the prefix takes its rotation in `finalize`,
        once its final ids are known), so only the current chunk's rows of the returned K may be attended to - which is
        all the sharded prefill does (scores are chunk-local, longvideo_cache.py:264)."""
        return self.cache.update(key_states, value_states, layer_idx, cache_kwargs)

    def update_pre_rope(self, *args, **kwargs):
        """PivotKVCache.update_pre_rope on this rank's block: with pre-RoPE operands the scores - and so the kept set -
        do not depend on the (provisional) ids at all, in any dtype."""
        return self.cache.update_pre_rope(*args, **kwargs)

    def gather_chunk(self):
        """Optional, after `after_forward()` of a chunk: start the all-gather of the rows that chunk kept (all
        layers, one collective) so that it overlaps the next chunk's scoring; `finalize(assemble=True)` then only
        waits, rotates every rank's segment to its true temporal position and exchanges the ids."""
        cache = self.cache
        cache.after_forward()
        kc, vc = cache.key_cache, cache.value_cache
        if self._gather is None:
            p2p = _p2p_for(kc[0], self.group)
            if p2p is None:
                self._gather = ChunkGather(self.group)
            elif self.expected_rows is None:
                return          # p2p pushes need their final position: assemble at the end instead
            else:
                _, Hkv, _, D = kc[0].shape
                cg = self.chunk_gather
                if cg is None or not cg.matches(self.expected_rows, len(kc), Hkv, D, kc[0].dtype):
                    need = ChunkGatherP2P._bytes(p2p.world, self.expected_rows, len(kc), Hkv, D, kc[0].dtype)
                    cg = ChunkGatherP2P(p2p, self.expected_rows, len(kc), Hkv, D, kc[0].dtype,
                                        capacity_bytes=0 if cg is None else need * 3 // 2)
                else:
                    cg.begin_video(self.expected_rows, len(kc), Hkv, D, kc[0].dtype)
                self._gather = self.chunk_gather = cg
            self._seen = [0] * len(kc)
        ks, vs = [], []
        for layer in range(len(kc)):
            ks.append(kc[layer][0, :, self._seen[layer]:])
            vs.append(vc[layer][0, :, self._seen[layer]:])
            self._seen[layer] = kc[layer].shape[2]
        self._gather.start(ks, vs)

    def finalize(self, inv_freq: torch.Tensor, mrope_section: Optional[List[int]], assemble: bool = True,
                 attention_scaling: Optional[float] = None, phases: Optional["PhaseTimer"] = None):
        """Exchange offsets, shift this rank's ids to their true temporal position, rotate the kept keys - un-rotated
        until now - ONCE at those final ids (what the sequential cache does per chunk, reference :297-306: same tables,
        same roundings, so a block's keys carry the bits they would have had in a single-GPU run), and optionally
        all-gather the full compressed cache.  Returns (keys, values, position_ids) lists per layer.
        attention_scaling: of the rotary module the keys belong to (default: the one the cache's updates were given).

        Collectives, in the order every rank enters them: the geometry (`_exchange_geometry`), the offsets (here), the
        row counts and the flags (`_agree_on_overlapped_gathers`), then the ids (`_finish_overlapped`) or the counts, K / V
        and the ids (`_rotate_own_and_assemble`, with `assemble`)."""
        self.cache.after_forward()
        p2p = _P2P.get(self.group)
        geo = self._exchange_geometry(p2p)
        if geo is None:    # nobody kept a row (the same answer on every rank): an empty cache, nothing to exchange
            self._gather = None
            return [], [], []
        dev, empty, keys, values, pos, last = geo
        delta = exchange_temporal_offsets(last, self.first_start, self.group)      # [layers]: one all-gather
        _mark(phases, "offsets")
        with torch.cuda.device(dev):
            rotate = _rotator(inv_freq, mrope_section, self._attention_scaling(attention_scaling), dev)
            self._shift_ids(pos, delta)
            counts, g = self._agree_on_overlapped_gathers(keys[0].shape[2], dev, assemble, p2p)
            if g is not None:
                return self._finish_overlapped(g, pos, counts, rotate, phases, p2p)
            return self._rotate_own_and_assemble(0 if empty else len(keys), keys, values, pos, counts, rotate, assemble, phases)

    def _exchange_geometry(self, p2p):
        """Step 1 -> (device, is this rank's block empty, its keys, values and ids per layer, its last provisional temporal id
        [layers]); None if no rank kept a row.  Enters ONE collective, the first of `finalize` on every rank: an all-gather
        of five int64.

        A rank whose block is empty (fewer chunks than ranks: `shard_chunks` hands out (c, c) blocks) holds a cache that
        never saw an update - no layers, no device, no dtype.  It still takes part in EVERY exchange of `finalize`, with
        zero rows: the ranks tell each other (layers, Hkv, D, dtype, id rank) here, and an empty rank adopts the geometry
        of the first rank that has rows."""
        from . import _native as nv

        cache = self.cache
        pcs = cache.position_cache
        if pcs:
            dev = pcs[0].device
            k0 = cache.key_cache[0]
            mine = [len(pcs), k0.shape[1], k0.shape[3], nv.dtype_code(k0), pcs[0].ndim]
        else:
            dev = p2p.device if p2p is not None else torch.device("cuda", torch.cuda.current_device())
            mine = [0, 0, 0, -1, 0]
        geo = _gather_stack(torch.tensor(mine, dtype=torch.int64, device=dev), self.group).tolist()
        have = [g_ for g_ in geo if g_[0] > 0]
        if not have:
            return None
        if any(g_ != have[0] for g_ in have):
            raise RuntimeError(f"sharded finalize: the ranks' caches disagree on (layers, Hkv, D, dtype, id rank): {geo}")
        n_layers, Hkv, D, dcode, id_ndim = have[0]
        if pcs:
            last = torch.stack([pc.reshape(-1, pc.shape[-1])[0, -1] for pc in pcs])               # [layers]
            return (dev, False, [cache.key_cache[layer] for layer in range(n_layers)],
                    [cache.value_cache[layer] for layer in range(n_layers)], pcs[:n_layers], last)
        dt = {nv.RTK_F32: torch.float32, nv.RTK_BF16: torch.bfloat16, nv.RTK_F16: torch.float16}[dcode]
        pcs = [torch.empty((3, 1, 0) if id_ndim == 3 else (1, 0), dtype=torch.int64, device=dev) for _ in range(n_layers)]
        kv0 = [torch.empty((1, Hkv, 0, D), dtype=dt, device=dev) for _ in range(n_layers)]
        last = torch.full((n_layers,), -1, dtype=torch.int64, device=dev)     # "-1 if the block kept nothing"
        return dev, True, kv0, list(kv0), pcs, last

    def _attention_scaling(self, attention_scaling: Optional[float]) -> float:
        if attention_scaling is not None:
            return attention_scaling
        b = self.cache._batch   # (a cache that never saw a compressed update has no batch: plain RoPE scaling)
        rot = b.rot if b is not None else None
        return rot.scaling if rot is not None else float(
            getattr(b.rotary_emb_fn if b is not None else None, "attention_scaling", 1.0))

    @staticmethod
    def _shift_ids(pos: List[torch.Tensor], delta: torch.Tensor):
        """Step 2: the stored ids of every layer, in place, from the provisional to the true temporal position.  No
        collective."""
        for layer, pc in enumerate(pos):
            if pc.ndim == 3:
                pc[0] += delta[layer]
            else:
                pc += delta[layer]

    def _agree_on_overlapped_gathers(self, rows: int, dev, assemble: bool, p2p):
        """Step 3 -> (row counts per rank, the started per-chunk gathers if ALL ranks finish from them, else None).
        Enters TWO collectives: the row counts (`gather_counts`), then an all-gather of two int64 (the flags).

        ONE decision for all ranks, taken before anybody waits on anything: the overlapped per-chunk gathers are used
        only if every rank started one for every chunk (its rows == the rows it kept) and every rank kept equally many
        rows; otherwise every rank that started any abandons them (ChunkGatherP2P.drop re-aligns the push epochs, so ranks
        that pushed different numbers of chunks neither stall nor latch a timeout) and the cache is assembled by the padded
        gather at the end."""
        g, self._gather = self._gather, None
        counts = gather_counts(rows, dev, self.group)
        mine_ok = g is not None and assemble and g.rows() == rows and len(set(counts)) == 1
        flags = _gather_stack(torch.tensor([int(mine_ok), g.pushes() if g is not None else -1], dtype=torch.int64,
                                           device=dev), self.group)
        if bool(flags[:, 0].min().item()):
            return counts, g
        pushes = [int(x) for x in flags[:, 1].tolist()]
        started = [x for x in pushes if x >= 0]
        if started:
            # `flags` is the same tensor on every rank, so every rank takes the same branch here - before anybody
            # enters another collective.  Two mismatches cannot be repaired after the fact and raise on ALL ranks:
            # a rank without per-chunk gathers among ranks that started some (its peers' pushes would wait for an
            # epoch it never publishes / its landing buffers keep another video's epoch), and unequal numbers of
            # all-gathers on the collective transport (the extra one has no partner).
            if len(started) != len(pushes):
                raise RuntimeError(f"per-chunk gathers were started on some ranks only (pushes per rank: {pushes}): "
                                   "every rank must call gather_chunk for every chunk, or none")
            if min(started) != max(started) and p2p is None:
                raise RuntimeError(f"ranks started between {min(started)} and {max(started)} per-chunk all-gathers: "
                                   "unmatched collectives")
            g.drop(min(started), max(started))
        return counts, None

    def _finish_overlapped(self, g, pos, counts, rotate, phases, p2p):
        """Step 4, from the overlapped gathers: wait for them, exchange the ids, rotate every row of every layer at its
        final id with ONE launch over the assembled cache.  Enters ONE collective (`all_gather_ids`); the waits of
        `g.finish()` are for collectives (pushes) started per chunk."""
        kv = g.finish()                                   # [2, layers, Hkv, world*n, D], keys still un-rotated
        pos = all_gather_ids(pos, self.group, counts)     # the final ids of every rank's rows
        _mark(phases, "assembly")                         # (the rows travelled beside the blocks: this is the wait)
        if phases is not None:
            phases.note_bytes("assembly_rows_received", kv.numel() * kv.element_size() * (len(counts) - 1) // len(counts))
        n_layers, rows = kv.shape[1], kv.shape[3]
        P = 3 if pos[0].ndim == 3 else 1
        ids_all = torch.stack([p_.reshape(P, rows) for p_ in pos]).contiguous()      # [layers, P, world*n]
        rotate(kv[0], kv.stride(1), kv.stride(2), n_layers, kv.shape[2], rows, kv.shape[4], ids_all, P * rows, rows, P)
        keys = [kv[0, layer][None] for layer in range(n_layers)]
        values = [kv[1, layer][None] for layer in range(n_layers)]
        _mark(phases, "rotate")
        if p2p is not None:
            p2p.check()   # synchronises; a wait that timed out left a partly filled landing buffer: raise
        return keys, values, pos

    def _rotate_own_and_assemble(self, own_layers, keys, values, pos, counts, rotate, assemble, phases):
        """Step 4, without the overlapped gathers: this rank's kept rows of every layer (`own_layers`: none on an empty
        rank) are rotated in place in the layers' cache buffers, at their final ids; then, with `assemble`, the THREE
        collectives of `all_gather_caches`: the row counts once more, K and V of every layer in one, the ids in one."""
        cache = self.cache
        cache._epoch += 1   # stored rows are rewritten: restore points taken before this are void (PivotKVCache.rewind)
        for layer in range(own_layers):
            st_l = cache._layers[layer]
            kbuf, k = st_l.k, keys[layer]
            rotate(kbuf, 0, kbuf.shape[2] * kbuf.shape[3], 1, k.shape[1], k.shape[2], k.shape[3], st_l.pos, 0,
                   st_l.pos.shape[1], 3 if pos[layer].ndim == 3 else 1)
        _mark(phases, "rotate")
        if assemble:
            own = sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in zip(keys, values))
            keys, values, pos = all_gather_caches(keys, values, pos, self.group)
            _mark(phases, "assembly")
            if phases is not None:
                phases.note_bytes("assembly_rows_received", own * (len(counts) - 1))
        return keys, values, pos

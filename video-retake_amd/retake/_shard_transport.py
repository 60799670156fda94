"""What moves bytes between the ranks of the sharded prefill (retake/sharded.py), and the index arithmetic around it.

Transport: `torch.distributed` collectives (RCCL) by default.  `enable_p2p(group)` switches every device-side exchange of
that group to the direct peer-to-peer pushes of retake/p2p.py (`rtk_p2p_*`: mapped peer buffers, one hop on every xGMI
link at once, no ring).  `_gather_stack` is the ONE place that looks at the backend; every exchange of the package is a
call of it.  The host logic below it is device independent and exercised over gloo by tests/test_sharded_cpu.py.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch
import torch.distributed as dist

_P2P = {}   # process group (None = the default group) -> retake.p2p.P2PGroup


def enable_p2p(group=None, device=None):
    """Route this group's device-side exchanges through mapped peer buffers (collective: every rank must call it)."""
    from .p2p import P2PGroup

    if group not in _P2P:
        _P2P[group] = P2PGroup(group, device)
    return _P2P[group]


def disable_p2p(group=None):
    g = _P2P.pop(group, None)
    if g is not None:
        g.close()


def _p2p_for(t: torch.Tensor, group):
    g = _P2P.get(group)
    return g if g is not None and t.is_cuda else None


class _Done:
    """The `work` of an exchange that was complete when it returned."""

    def wait(self):
        return True


def _gather_stack(t: torch.Tensor, group=None, *, copy: bool = True, async_op: bool = False):
    """t (same shape on every rank) -> [world, *t.shape] in rank order: THE collective of the sharded path.

    copy=False: with the p2p transport the result is the landing buffer itself, which is only valid until this rank's NEXT
    exchange on the group - for callers that copy out of it (permute + reshape / cat) before they return; at world size
    1, where those are views, it is cloned all the same.
    async_op=True: -> (work, result); `result` may be read after `work.wait()`, and `t` must live until then.  The p2p
    and the host-staged exchanges are complete when they return (`_Done`)."""
    t = t.contiguous()
    g = _p2p_for(t, group)
    if g is not None:
        recv = g.all_gather(t)
        if copy or g.world == 1:
            recv = recv.clone()
        return (_Done(), recv) if async_op else recv
    world = dist.get_world_size(group)
    if t.is_cuda and dist.get_backend(group) == "gloo":
        # device tensors over a gloo group (tests/mp_sharded_gpu.py with RETAKE_TEST_TRANSPORT=host, a debugging aid: the
        # sharded path with NO device-side transport at all - no RCCL, no peer mapping): staged through the host
        h = t.cpu()
        parts = [torch.empty_like(h) for _ in range(world)]
        dist.all_gather(parts, h, group=group)
        recv = torch.stack(parts).to(t.device)
        return (_Done(), recv) if async_op else recv
    recv = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    if t.is_cuda:
        work = dist.all_gather_into_tensor(recv, t, group=group, async_op=async_op)
    else:  # gloo has no all_gather_into_tensor on every build
        work = dist.all_gather(list(recv.unbind(0)), t, group=group, async_op=async_op)
    return (work, recv) if async_op else recv


def gather_counts(n: int, device, group=None) -> List[int]:
    """How many rows every rank is about to contribute (one tiny all-gather).  Equal-size collectives
    (`all_gather_into_tensor`) hang or corrupt memory when the ranks disagree, so every assembly asks first."""
    mine = torch.tensor([int(n)], dtype=torch.int64, device=device)
    counts = [int(c) for c in _gather_stack(mine, group).reshape(-1).tolist()]
    g = _p2p_for(mine, group)
    if g is not None:
        g.check()   # the .tolist() above synchronised: a bounded p2p wait that gave up (lost / late peer) raises HERE
    return counts


def _gather_ragged(shape, dim: int, counts: List[int], like: torch.Tensor, fill: Callable, group=None) -> torch.Tensor:
    """A block of `shape` with a different shape[dim] per rank (`counts`) -> the blocks of all ranks, rank-major along `dim`.

    The blocks are padded along `dim` to the longest one, exchanged with ONE equal-size all-gather and laid out with
    every rank's padding dropped.  `fill(own)` writes this rank's block straight into its rows of the send buffer.  Equal
    counts (every chunk keeps exactly `keep` tokens and the ranks hold equally many chunks) move exactly the rows: an
    uninitialised send buffer, and one permute copy of the result instead of a cat of per-rank slices."""
    n, nmax, equal = shape[dim], max(counts), len(set(counts)) == 1
    shape = list(shape)
    shape[dim] = nmax
    send = (torch.empty if equal else torch.zeros)(shape, dtype=like.dtype, device=like.device)
    fill(send if n == nmax else send.narrow(dim, 0, n))
    # along dim 0 the rank-major layout below is a VIEW of the result, which must then not be the p2p landing buffer
    recv = _gather_stack(send, group, copy=dim == 0)                   # [world, *shape]
    if equal:
        shape[dim] = len(counts) * n
        return recv.movedim(0, dim).reshape(shape)
    return torch.cat([recv[r].narrow(dim, 0, c) for r, c in enumerate(counts)], dim=dim)


# ---------------------------------------------------------------------------------------------------
# assemblies
# ---------------------------------------------------------------------------------------------------
def all_gather_cat(t: torch.Tensor, dim: int, group=None) -> torch.Tensor:
    """All-gather equally shaped tensors and concatenate along `dim` in rank order."""
    return torch.cat(list(_gather_stack(t, group).unbind(0)), dim=dim)


def all_gather_rows(local: torch.Tensor, group=None) -> torch.Tensor:
    """[rows_local, ...] -> [world*rows_local, ...] in rank order (distance rows)."""
    full = _gather_stack(local, group)
    return full.reshape((full.shape[0] * local.shape[0],) + tuple(local.shape[1:]))


def all_gather_rows_ragged(local: torch.Tensor, group=None, counts: Optional[List[int]] = None) -> torch.Tensor:
    """[rows_r, ...] with a different rows_r per rank -> [sum rows, ...] in rank order (a video whose chunk count is not a
    multiple of the world size gives the last ranks one chunk less)."""
    counts = counts if counts is not None else gather_counts(local.shape[0], local.device, group)
    if len(set(counts)) == 1:   # nothing to pad: the rows go out as they are
        return all_gather_rows(local, group)
    return _gather_ragged(local.shape, 0, counts, local, lambda own: own.copy_(local), group)


def all_gather_caches(keys: List[torch.Tensor], values: List[torch.Tensor], pos: List[torch.Tensor], group=None):
    """Cache assembly for ALL layers with two collectives instead of three per layer (xGMI is point to point: few
    large all-gathers use the links far better than 84 small ones, and each result needs one permute copy instead
    of a per-tensor scatter + cat).

    keys / values: per layer [1, Hkv, n, D]; pos: per layer [3, 1, n] or [1, n] int64.  The ranks first exchange their
    row counts (`_gather_ragged`).  Returns the per-layer lists [1, Hkv, sum n, D] / [..., sum n] in rank order."""
    n_layers = len(keys)
    _, Hkv, n, D = keys[0].shape
    counts = gather_counts(n, keys[0].device, group)

    def fill(own):   # stack straight into the send buffer
        torch.stack([k[0] for k in keys], out=own[0])
        torch.stack([v[0] for v in values], out=own[1])

    kv = _gather_ragged((2, n_layers, Hkv, n, D), 3, counts, keys[0], fill, group)   # rank-major inside a head
    return ([kv[0, l][None] for l in range(n_layers)], [kv[1, l][None] for l in range(n_layers)],
            all_gather_ids(pos, group, counts))


def all_gather_ids(pos: List[torch.Tensor], group=None, counts: Optional[List[int]] = None) -> List[torch.Tensor]:
    """Per-layer position ids [..., n_r] of every rank -> [..., sum n_r] in rank order, one collective."""
    n_layers, n = len(pos), pos[0].shape[-1]
    counts = counts if counts is not None else gather_counts(n, pos[0].device, group)
    pshape = tuple(pos[0].shape[:-1])
    rows = 1
    for d in pshape:
        rows *= d
    pall = _gather_ragged((n_layers, rows, n), 2, counts, pos[0],
                          lambda own: torch.stack([p.reshape(rows, n) for p in pos], out=own), group)
    return [pall[l].reshape(pshape + (sum(counts),)) for l in range(n_layers)]


# ---------------------------------------------------------------------------------------------------
# host logic (device independent; exercised by the gloo tests)
# ---------------------------------------------------------------------------------------------------
def shard_chunks(n_chunks: int, world: int) -> List[Tuple[int, int]]:
    """Contiguous, balanced chunk blocks [c0, c1) per rank (first `n_chunks % world` ranks get one more)."""
    base, extra = divmod(n_chunks, world)
    out, c = [], 0
    for r in range(world):
        n = base + (1 if r < extra else 0)
        out.append((c, c + n))
        c += n
    return out


def exchange_temporal_offsets(local_last: torch.Tensor, first_start: int = 0, group=None,
                              all_ranks: bool = False) -> torch.Tensor:
    """local_last [layers] int64 = last PROVISIONAL temporal id of this rank's block per layer (block ids
    start at 0; -1 if the block kept nothing).  Returns delta [layers] int64 for this rank: the true start
    of the block, i.e. first_start + sum over previous ranks of (last + 1); with all_ranks the whole
    [world, layers] table (every rank computes the same one)."""
    rank = dist.get_rank(group)
    spans = _gather_stack(local_last, group) + 1           # [world, layers]
    prefix = torch.cumsum(spans, dim=0) - spans            # exclusive
    table = (prefix + first_start).contiguous()
    return table if all_ranks else table[rank]


def plan_frame_exchange(idx: torch.Tensor, T_own: int, world: int):
    """Who sends which kept frame where (DPSelect at ratio < 1 on frames sharded `T_own` per rank).

    idx: the global selection, [t] (sync) or [t, N] (per patch position), ascending along dim 0
    (visual_compression.py:135,169).  Because it ascends, the kept frames of patch n that live on rank r are
    the run j in [start[r, n], start[r+1, n]).  Returns
      start  [world+1, N'] int64 (N' = 1 for sync),
      cmax   int, the longest run (the padded block length every rank sends),
      local  [world, cmax, N'] int64: rank r's local frame index for slot (jl, n); padding repeats a valid frame,
      place  [t, N'] int64: row of the rank-ordered concatenation of the padded blocks that holds output (j, n).
    Pure index arithmetic on idx's device; identical on every rank because idx is."""
    i2 = idx if idx.ndim == 2 else idx[:, None]
    t, n_pos = i2.shape
    dev = i2.device
    bounds = torch.arange(world + 1, device=dev, dtype=torch.int64) * T_own
    start = torch.searchsorted(i2.t().contiguous(), bounds[None, :].expand(n_pos, -1).contiguous()).t().contiguous()
    cmax = max(1, int((start[1:] - start[:-1]).max().item()))
    jl = torch.arange(cmax, device=dev, dtype=torch.int64)[None, :, None]          # [1, cmax, 1]
    j = start[:-1, None, :] + jl                                                     # [world, cmax, N']
    valid = j < start[1:, None, :]
    src = torch.gather(i2[None].expand(world, -1, -1), 1, j.clamp(max=t - 1))       # global frame per slot
    r0 = torch.arange(world, device=dev, dtype=torch.int64)[:, None, None] * T_own
    local = torch.where(valid, src - r0, torch.zeros_like(src)).clamp_(0, T_own - 1)
    owner = torch.div(i2, T_own, rounding_mode="floor")                              # [t, N']
    jj = torch.arange(t, device=dev, dtype=torch.int64)[:, None]
    place = owner * cmax + (jj - torch.gather(start, 0, owner))
    return start, cmax, local.contiguous(), place.contiguous()

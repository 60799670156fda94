"""Cache assembly overlapped with the compression of the following chunks (retake/sharded.py, `gather_chunk`): the rows a
chunk kept leave right after its flush - in one asynchronous all-gather (`ChunkGather`), or pushed straight to their final
position in every rank's assembled cache (`ChunkGatherP2P`)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ._shard_transport import _Done, _gather_stack  # noqa: F401  (`_Done`: what a finished exchange hands `ChunkGather`)


def _stage(k_new: List[torch.Tensor], v_new: List[torch.Tensor]) -> torch.Tensor:
    """k_new / v_new: per layer [Hkv, n, D] (any strides), the rows one chunk added -> send [2, layers, Hkv, n, D]."""
    Hkv, n, D = k_new[0].shape
    send = torch.empty((2, len(k_new), Hkv, n, D), dtype=k_new[0].dtype, device=k_new[0].device)
    torch.stack(list(k_new), out=send[0])
    torch.stack(list(v_new), out=send[1])
    return send


class ChunkGather:
    """Cache assembly overlapped with the compression of the following chunks: after each chunk's flush the rows it
    kept in every layer go out in ONE asynchronous all-gather (RCCL runs it on its own stream beside the score
    kernels of the next chunk); `finish` waits for the lot and lays the blocks out rank-major.  The rows travel at
    their PROVISIONAL temporal position - the caller applies R(delta_r) to rank r's segment afterwards."""

    def __init__(self, group=None):
        self.group = group
        self.items = []   # (work, recv [W, 2, layers, Hkv, n, D], send)

    def start(self, k_new: List[torch.Tensor], v_new: List[torch.Tensor]):
        """k_new / v_new: per layer [Hkv, n, D] (any strides), the rows one chunk added.  Every rank must call this
        equally often with equally many rows (callers whose ranks hold different chunk counts assemble at the end
        instead: `finalize` checks the totals before it trusts the overlapped gathers)."""
        send = _stage(k_new, v_new)
        self.items.append(_gather_stack(send, self.group, async_op=True) + (send,))

    def rows(self) -> int:
        return sum(it[2].shape[3] for it in self.items)

    def pushes(self) -> int:
        return len(self.items)

    def drop(self, lo: int = 0, hi: int = 0):
        """Abandon the started gathers.  They are collectives: every rank must have started equally many (`lo == hi`),
        which `sharded_video_step` guarantees by only overlapping even chunk splits - a mismatch cannot be repaired
        after the fact (the extra all-gather of one rank has no partner), so it raises instead of hanging in `wait`."""
        if lo != hi:
            raise RuntimeError(f"ranks started between {lo} and {hi} per-chunk all-gathers: unmatched collectives")
        for work, _, _ in self.items:
            work.wait()
        self.items = []

    def finish(self) -> torch.Tensor:
        """-> [2, layers, Hkv, world * rows, D]: rank-major, then chunk order, inside every head."""
        for work, _, _ in self.items:
            work.wait()
        world, _, n_layers, Hkv, _, D = self.items[0][1].shape
        total = self.rows()
        out = torch.empty((2, n_layers, Hkv, world, total, D), dtype=self.items[0][1].dtype,
                          device=self.items[0][1].device)
        at = 0
        for _, recv, _ in self.items:
            n = recv.shape[4]
            out[:, :, :, :, at:at + n] = recv.permute(1, 2, 3, 0, 4, 5)
            at += n
        self.items = []
        return out.view(2, n_layers, Hkv, world * total, D)


class ChunkGatherP2P:
    """`ChunkGather` over mapped peer buffers: the rows a chunk kept are pushed (side stream, beside the next chunk's
    scoring) straight to their FINAL position in every rank's assembled cache `[2, layers, Hkv, world * total, D]` -
    rank-major, then chunk order, inside every head - so `finish` only waits for the arrival flags; there is no receive
    buffer to permute.  Needs the rows per rank and video (`total`) up front.

    Lifetime: two landing buffers alternate between videos.  A peer starts pushing video n+2 into the buffer of video n
    as soon as ITS video n+1 is assembled, i.e. once this rank's last push of video n+1 has landed there - so the cache
    `finish` returned for video n is guaranteed intact only for reads this rank enqueued BEFORE its last `start` of video
    n+1.  Treat it as valid until this rank begins the next video; clone what must live longer.

    Memory: the two buffers are byte pools sized for the LARGEST video seen so far (`capacity` bytes each); a shorter
    or differently shaped video of at most that many bytes reuses them with its own strides, a larger one allocates a
    new pair 1.5x the need (mapped buffers are never freed before `P2PGroup.close()`, see SymmetricBuffer.close: the
    total mapped memory is bounded by ~3x the largest pair, not by the number of distinct shapes)."""

    def __init__(self, p2p, total: int, n_layers: int, Hkv: int, D: int, dtype, capacity_bytes: int = 0):
        self.p2p = p2p
        need = self._bytes(p2p.world, total, n_layers, Hkv, D, dtype)
        self.capacity = max(int(capacity_bytes), need)
        self.bufs = [p2p.symmetric(self.capacity), p2p.symmetric(self.capacity)]
        self.side = torch.cuda.Stream(device=p2p.device)
        self.gen, self.at = 1, 0
        self._sources: List[Tuple[torch.cuda.Event, torch.Tensor]] = []   # push sources whose copy kernel may still run
        self.begin_video(total, n_layers, Hkv, D, dtype)

    @staticmethod
    def _bytes(world, total, n_layers, Hkv, D, dtype) -> int:
        return 2 * n_layers * Hkv * world * int(total) * D * torch.empty((), dtype=dtype).element_size()

    def matches(self, total, n_layers, Hkv, D, dtype) -> bool:
        """Can a video of this shape land in the mapped buffers?"""
        return self._bytes(self.p2p.world, total, n_layers, Hkv, D, dtype) <= self.capacity

    def begin_video(self, total=None, n_layers=None, Hkv=None, D=None, dtype=None):
        if total is not None:
            if not self.matches(total, n_layers, Hkv, D, dtype):
                raise ValueError("p2p chunk gather: the video does not fit the mapped landing buffers")
            self.total, self.dtype = int(total), dtype
            self.shape = (2, n_layers, Hkv, self.p2p.world, self.total, D)
            self.es = torch.empty((), dtype=dtype).element_size()
        self.gen ^= 1
        self.at = 0
        self._release_sources()

    def start(self, k_new: List[torch.Tensor], v_new: List[torch.Tensor]):
        n_layers = len(k_new)
        Hkv, n, D = k_new[0].shape
        if self.at + n > self.total:
            raise ValueError(f"p2p chunk gather: {self.at + n} rows pushed, the landing buffer was sized for {self.total}")
        send = _stage(k_new, v_new)
        self.side.wait_stream(torch.cuda.current_stream(send.device))
        send.record_stream(self.side)
        row = D * self.es
        world, rank = self.p2p.world, self.p2p.rank
        self.bufs[self.gen].push(send, n * row, 2 * n_layers * Hkv, n * row, (rank * self.total + self.at) * row,
                                 world * self.total * row, stream=self.side)
        # the push kernel reads `send` on the side stream after this function has returned (record_stream above only
        # protects it under torch's caching allocator): the tensor is kept until an event behind its push has completed -
        # one or two chunks' rows at a time, not a second copy of everything the rank kept over the video
        ev = torch.cuda.Event()
        ev.record(self.side)
        self._release_sources()
        self._sources.append((ev, send))
        self.at += n

    def _release_sources(self):
        self._sources = [(e, t) for e, t in self._sources if not e.query()]

    def rows(self) -> int:
        return self.at

    def pushes(self) -> int:
        return self.bufs[self.gen].epoch

    def drop(self, lo: Optional[int] = None, hi: Optional[int] = None):
        """Abandon the per-chunk pushes of this video (`finalize` reaches that decision for all ranks at once and hands
        over the smallest / largest push count of the landing buffer over the ranks).  The ranks may have pushed
        DIFFERENT numbers of chunks (one skipped a `gather_chunk`, or `start` raised on one rank only): each waits for
        the smallest count - which every sender has reached, so nobody stalls into the timeout and no error is latched -
        and continues from the largest, so that the epochs agree again for the next video."""
        torch.cuda.current_stream(self.p2p.device).wait_stream(self.side)
        buf = self.bufs[self.gen]
        buf.resync(buf.epoch if lo is None else lo, buf.epoch if hi is None else hi)

    def finish(self) -> torch.Tensor:
        """-> [2, layers, Hkv, world * total, D], a view of the landing buffer (lifetime: class docstring)."""
        if self.at != self.total:
            raise ValueError(f"p2p chunk gather: {self.at} of {self.total} rows pushed")
        buf = self.bufs[self.gen]
        torch.cuda.current_stream(self.p2p.device).wait_stream(self.side)
        buf.wait()
        two, n_layers, Hkv, world, total, D = self.shape
        n = two * n_layers * Hkv * world * total * D * self.es
        return buf.local[:n].view(self.dtype).view(two, n_layers, Hkv, world * total, D)

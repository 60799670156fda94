"""DPSelect on a stream: keyframe selection for a video that does not end.

`memory_bank_compress_keyframe` needs the finished video.  `DPSelectStream` takes the frame embeddings as they arrive
(`push`), keeps them in a ring of 2 * segment_frames rows and emits one compressed `Segment` per `segment_frames` frames, in
fixed memory.  The rule is this project's own - the reference processes a finished video, so there is no reference run for
several segments, and what the rule does to answer quality has not been evaluated:

  * the distance of global frame g is the whole-video call's: 1.0 for g = 0, else `rtk_dpselect_dis` of the pair (g-1, g),
    bit for bit - also across the seam between two segments and between two pushes;
  * g is a peak by the whole-video rule, its window [g - w/2, g - w/2 + w - 1] laid on the GLOBAL frame line and clipped
    only at frame 0 and, at `finish()`, at the last frame; a peak's key is its distance + 2.0;
  * segment k = frames [k S, (k+1) S) keeps the top max(1, round(ratio * len)) (or min(keep, len)) keys of its own frames,
    ties to the lowest index, emitted in ascending order; the mask of a kept frame is whether it is a peak;
  * segment k leaves with the push that delivers frame (k+1) S - 1 + (w - 1 - w/2), the last frame its windows look at, or
    with `finish()`.

So a stream of one segment (S >= T) closed by `finish()` is the whole-video call; what is emitted depends on the frames and
the parameters only, not on how the pushes are cut; and a stream that ends after one frame emits that frame (a lone peak -
the reference raises for T == 1).

Three kernels per segment, nothing read back, no synchronisation, everything on the current stream:
    rtk_dpselect_ingest       new frames -> ring rows + their distance rows, one pass   (once per contiguous piece of a push)
    rtk_dpselect_select_ring  peaks + bonus + top-k of one segment, halo rows from the ring
    rtk_gather_frames         the kept frames, from the segment's rows
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import torch

from . import _native as nv

__all__ = ["DPSelectStream", "Segment", "plan_push", "plan_finish", "segment_geometry"]


class Segment(NamedTuple):
    frames: torch.Tensor           # [1, keep_k, N, C], a fresh tensor
    keypatches_mask: torch.Tensor  # [keep_k * N] bool: what cache.keypatches_mask_chunk takes
    idx: torch.Tensor              # GLOBAL frame indices, int64: [keep_k] (sync) / [keep_k, N] (async)
    first_frame: int               # k * S
    num_frames: int                # len_k
    dis: torch.Tensor              # [len_k, N] fp32: a copy of the segment's distance rows


def _halo(window: int) -> Tuple[int, int]:
    """(lookbehind, lookahead) of the peak window [g - w/2, g - w/2 + w - 1]."""
    return window // 2, window - 1 - window // 2


def plan_push(S: int, window: int, seen: int, t: int) -> list:
    """What a push of `t` frames does to a stream that has seen `seen`, as host integers:
    ("ingest", offset into the push, count, global index of the first frame) - one contiguous run of ring rows - and
    ("emit", k) - segment k is complete, its lookahead included.  A push is cut at the ring's wrap (multiples of 2 S) and
    behind every frame (k+1) S - 1 + la that completes a segment, so a piece never overwrites rows a pending segment needs."""
    la = _halo(window)[1]
    R = 2 * S
    ops, g, end = [], seen, seen + t
    while g < end:
        k = max(0, -((S + la - 1 - g) // S))          # the first segment whose last lookahead frame is at or behind g
        last = (k + 1) * S - 1 + la
        stop = min(end, (g // R + 1) * R, last + 1)
        ops.append(("ingest", g - seen, stop - g, g))
        if stop == last + 1:
            ops.append(("emit", k))
        g = stop
    return ops


def plan_finish(S: int, seen: int, emitted: int) -> list:
    """The segments `finish()` still owes: every segment that has a frame and has not left (at most two)."""
    return [("emit", k) for k in range(emitted, (seen + S - 1) // S)]


def segment_geometry(S: int, window: int, k: int, seen: int) -> Tuple[int, int, int, int]:
    """(first frame, len, left, right) of segment k when `seen` frames have arrived: the valid halo rows around it."""
    lb, la = _halo(window)
    first = k * S
    length = min(S, seen - first)
    return first, length, min(lb, first), min(la, seen - first - length)


class DPSelectStream:
    """Stateful DPSelect (module docstring).  `ratio` or an integer `keep` per segment; `window_size` and `sync` as
    `memory_bank_compress_keyframe` takes them.  The ring is allocated once, at the first push, which fixes N, C, dtype and
    device; all calls of one stream belong on one HIP stream (the kernels are ordered by it, nothing else)."""

    def __init__(self, segment_frames: int, *, ratio: Optional[float] = None, keep: Optional[int] = None,
                 window_size: int = 3, sync: bool = True):
        S, w = int(segment_frames), int(window_size)
        if w < 1:
            raise ValueError(f"DPSelectStream: window_size {window_size} < 1")
        if S < max(2, w):
            raise ValueError(f"DPSelectStream: segment_frames {segment_frames} < max(2, window_size = {w}): a segment's "
                             "halo must fit into the neighbouring segment")
        if (ratio is None) == (keep is None):
            raise ValueError("DPSelectStream: give exactly one of ratio and keep")
        if ratio is not None and not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f"DPSelectStream: ratio {ratio} outside (0, 1]")
        if keep is not None and not 1 <= int(keep) <= S:
            raise ValueError(f"DPSelectStream: keep {keep} outside [1, segment_frames = {S}]")
        self.segment_frames, self.window_size, self.sync = S, w, bool(sync)
        self.ratio = None if ratio is None else float(ratio)
        self.keep = None if keep is None else int(keep)
        self._frames = self._dis = self._keys = None
        self.reset()

    @classmethod
    def from_config(cls, config, segment_frames: int, window_size: int = 3) -> "DPSelectStream":
        """The stream for a model config: `longvideo_kwargs["visual_compression_kwargs"]`'s compression_ratio and
        patch_sync, as the whole-video path reads them."""
        ck = (getattr(config, "longvideo_kwargs", None) or {}).get("visual_compression_kwargs") or {}
        if ck.get("compression_method") != "Keyframe":
            raise ValueError(f"DPSelectStream.from_config: compression_method {ck.get('compression_method')!r} is not "
                             "'Keyframe' (DPSelect)")
        return cls(segment_frames, ratio=ck.get("compression_ratio"), window_size=window_size,
                   sync=bool(ck.get("patch_sync")))

    # ---- state ---------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Forget the stream, keep the ring."""
        self.frames_seen = 0
        self.segments_emitted = 0
        self._finished = False

    def memory_footprint(self) -> int:
        """Bytes of the ring (frames, distance rows, selection workspace): constant after the first push."""
        return sum(t.numel() * t.element_size() for t in (self._frames, self._dis, self._keys) if t is not None)

    def _keep_of(self, length: int) -> int:
        if self.keep is not None:
            return min(self.keep, length)
        return max(1, round(self.ratio * length))   # python's round, as the whole-video path (qwen2_vl.py:397)

    def _allocate(self, x: torch.Tensor) -> None:
        S, w = self.segment_frames, self.window_size
        _, N, Cc = x.shape
        nv.dtype_code(x)   # (raises for a dtype the kernels do not serve)
        self._frames = torch.empty((2 * S, N, Cc), dtype=x.dtype, device=x.device)
        self._dis = torch.empty((2 * S, N), dtype=torch.float32, device=x.device)
        self._keys = torch.empty((max(2 * S + w - 1, N * S),), dtype=torch.float32, device=x.device)

    # ---- the stream ----------------------------------------------------------------------------------------------------
    def push(self, frames: torch.Tensor) -> List[Segment]:
        """Feed `frames` ([t, N, C] or [1, t, N, C], t >= 0); returns the segments this push completed (often none)."""
        if self._finished:
            raise RuntimeError("DPSelectStream.push after finish(): call reset() to start a new stream")
        if frames.ndim == 4 and frames.shape[0] == 1:
            frames = frames[0]
        if frames.ndim != 3:
            raise ValueError(f"DPSelectStream.push: frames must be [t,N,C] or [1,t,N,C], got {tuple(frames.shape)}")
        if not self.sync and frames.shape[1] == 1:   # `.squeeze()` drops the patch axis (visual_compression.py:153-156)
            raise IndexError("DPSelectStream: sync=False with a single patch position (N == 1)")
        nv.require_device(frames)
        if self._frames is None:
            self._allocate(frames)
        ring = self._frames
        if frames.shape[1:] != ring.shape[1:] or frames.dtype != ring.dtype or frames.device != ring.device:
            raise ValueError(f"DPSelectStream.push: frames {tuple(frames.shape[1:])} {frames.dtype} on {frames.device} do not "
                             f"match the stream's {tuple(ring.shape[1:])} {ring.dtype} on {ring.device}")
        t = frames.shape[0]
        if t == 0:
            return []
        x = frames if frames.is_contiguous() else frames.contiguous()
        S, R = self.segment_frames, 2 * self.segment_frames
        _, N, Cc = ring.shape
        dt = nv.dtype_code(ring)
        out = []
        with torch.cuda.device(ring.device):
            st = nv.stream()
            for op in plan_push(S, self.window_size, self.frames_seen, t):
                if op[0] == "emit":
                    out.append(self._emit(op[1], st))
                    continue
                _, off, cnt, g = op
                prev = ring[(g - 1) % R] if g > 0 else None   # the frame before the piece is still in the ring
                nv.check(nv.lib.rtk_dpselect_ingest(nv.ptr(x[off]), nv.ptr(prev), cnt, N, Cc, dt, nv.ptr(ring[g % R]),
                                                    nv.ptr(self._dis[g % R]), st), "rtk_dpselect_ingest")
                self.frames_seen = g + cnt
        return out

    def finish(self) -> List[Segment]:
        """The stream ends: the remaining segments, their windows clipped at the last frame.  A later push raises until
        reset()."""
        if self._finished:
            return []
        self._finished = True
        out = []
        if self.frames_seen:
            with torch.cuda.device(self._frames.device):
                st = nv.stream()
                for _, k in plan_finish(self.segment_frames, self.frames_seen, self.segments_emitted):
                    out.append(self._emit(k, st))
        return out

    def _emit(self, k: int, st) -> Segment:
        S, R, sync = self.segment_frames, 2 * self.segment_frames, self.sync
        ring, dis = self._frames, self._dis
        _, N, Cc = ring.shape
        first, length, left, right = segment_geometry(S, self.window_size, k, self.frames_seen)
        keep, r0, dev = self._keep_of(length), first % R, ring.device
        idx = torch.empty((keep,) if sync else (keep, N), dtype=torch.int64, device=dev)
        mask = torch.empty((keep, N), dtype=torch.bool, device=dev)
        frames = torch.empty((1, keep, N, Cc), dtype=ring.dtype, device=dev)
        nv.check(nv.lib.rtk_dpselect_select_ring(nv.ptr(dis), R, N, r0, length, left, right, keep, self.window_size,
                                                 int(sync), nv.ptr(idx), nv.ptr(mask), nv.ptr(self._keys), st),
                 "rtk_dpselect_select_ring")
        # a segment is a contiguous run of ring rows (S divides R): the gather is the whole-video call's, idx local to it
        nv.check(nv.lib.rtk_gather_frames(nv.ptr(ring[r0]), length, N, Cc, nv.dtype_code(ring), nv.ptr(idx), keep,
                                          int(sync), nv.ptr(frames), st), "rtk_gather_frames")
        self.segments_emitted = k + 1
        return Segment(frames, mask.flatten(), idx + first, first, length, dis[r0:r0 + length].clone())

"""The position renumbering rule (video_position_gap on top of video_position_limit; csrc/pivotkv_rebase.hip) restated on the
host: numpy only, no call into the library.  The rule is this project's own - the reference has no counterpart, and what it
does to answer quality is not evaluated.  It generalises rebase_ref's one delta per layer to one per row.

  excess   in integers: e[first] = max(0, t[first] - prev - 1) with prev = t[first - 1] if first > 0 else -1 (the re-base's
           delta); e[i] = max(0, t[i] - t[i - 1] - gap) for first < i < end.  Gaps <= gap stay, 0 and negative ones too.
  deltas   d[i] = e[first] + ... + e[i]: non-negative, non-decreasing.
  decide   (d, total): total = d[end - 1] if the region is not empty, t[end - 1] >= limit and d[end - 1] > 0; else 0 - and
           then d is all zeros: nothing is applied.
  renumber one layer: t[i] -= d[i]; K row first + r (r < rows) <- rebase_ref.rotate(row, d[first + r]).

The rotation and its bar are rebase_ref's (rotate, bar, temporal_pairs): the kernel's arithmetic per row is the re-base's
with the row's own delta, so DESIGN.md §5's derivation holds row by row and no new constant appears."""
from __future__ import annotations

import numpy as np

import rebase_ref as rr


def excess(t, first: int, end: int, gap: int) -> np.ndarray:
    """e [end - first] in int64 (Python integers would do the same: no id here comes near 2^63)."""
    t = np.asarray(t, dtype=np.int64)
    if end <= first:
        return np.zeros(0, dtype=np.int64)
    prev = int(t[first - 1]) if first > 0 else -1
    e = np.empty(end - first, dtype=np.int64)
    e[0] = max(0, int(t[first]) - prev - 1)
    e[1:] = np.maximum(0, t[first + 1:end] - t[first:end - 1] - gap)
    return e


def deltas(t, first: int, end: int, gap: int) -> np.ndarray:
    return np.cumsum(excess(t, first, end, gap), dtype=np.int64)


def decide(t, first: int, end: int, limit: int, gap: int):
    """(d [end - first], total): what the layer applies - all zeros and 0 if it does not trigger."""
    d = deltas(t, first, end, gap)
    if len(d) == 0 or int(d[-1]) <= 0 or int(t[end - 1]) < limit:
        return np.zeros_like(d), 0
    return d, int(d[-1])


def renumber(ids, K, first: int, end: int, rows: int, limit: int, gap: int, inv_freq, sections=None):
    """One layer: ids int64 [P, cap], K [H, cap, D] -> (new ids, new K in float64, d [end - first], total).  K rows
    [first, first + rows) and ids [first, end) of row 0 change, and only where d > 0."""
    assert rows <= end - first
    ids = np.array(ids, dtype=np.int64, copy=True)
    out = np.array(K, dtype=np.float64, copy=True)
    d, total = decide(ids[0], first, end, limit, gap)
    if total:
        ids[0, first:end] -= d
        for v in np.unique(d[:rows]):      # one rotation per distinct delta
            if v:
                at = first + np.nonzero(d[:rows] == v)[0]
                out[:, at] = rr.rotate(out[:, at], int(v), inv_freq, ids.shape[0], sections)
    return ids, out, d, total

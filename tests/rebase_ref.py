"""The position re-base rule (video_position_limit; csrc/pivotkv_rebase.hip) restated on the host: numpy only, no call into
the library.  The rule is this project's own - the reference has no counterpart.

  decide   in integers: base = t[first - 1] + 1 if first > 0 else 0; delta = t[first] - base; the unit triggers iff the
           region is not empty, delta > 0 and t[end - 1] >= limit.  delta = 0 otherwise.
  rotate   in float64: theta64 = double(fl32(fl32(delta) * inv_freq[d])), o1 = x1 cos(theta64) + x2 sin(theta64),
           o2 = x2 cos(theta64) - x1 sin(theta64) on the temporal pairs (d, d + D/2) - all of them for P = 1, those the
           M-RoPE sections give to id row 0 for P = 3; every other channel is the input itself.
  rebase   both on one layer: ids [P, cap], K [H, cap, D].

The bar of the GPU tests, derived in DESIGN.md §5 (not measured): a rotated element is within
    half_ulp(dtype, |ref|) + C * (|x1| + |x2|),   C = 6 * 2^-24
of `rotate`'s value: the kernel's fp32 value o is within e = 2.5 * 2^-24 (|x1| + |x2|) of it (sin / cos correctly rounded:
2^-25 each; one product rounding and the fma's: 2^-24 each, of terms bounded by |x1| + |x2|), and rounding o to the storage
dtype adds at most half an ulp at |ref| if o lies in ref's binade or below, or at most |o - ref| if it lies above (the
power of two between them is representable) - so half_ulp(ref) + 2 e, and 2 * 2.5 rounds up to 6 with the second-order terms.
"""
from __future__ import annotations

import numpy as np

C = 6.0 * 2.0 ** -24
# (mantissa bits, exponent of the smallest normal) of the storage dtypes, by name
FORMATS = {"bfloat16": (7, -126), "float16": (10, -14), "float32": (23, -126)}


def temporal_pairs(D: int, P: int, sections=None) -> np.ndarray:
    """bool [D/2]: does the pair (d, d + D/2) follow id row 0?  (make_rowsel of csrc/common.cuh: two repetitions of the
    sections, section i of repetition rep follows row (rep * nsec + i) % 3.)"""
    h = D // 2
    if P == 1:
        return np.ones(h, dtype=bool)
    assert P == 3 and sections and 2 * sum(sections) == D
    nsec = len(sections)
    row = np.array([(rep * nsec + i) % 3 for rep in range(2) for i, s in enumerate(sections) for _ in range(s)])
    assert np.array_equal(row[:h] == 0, row[h:] == 0), "the sections split a rotation pair between id rows"
    return row[:h] == 0


def decide(t, first: int, end: int, limit: int) -> int:
    """The delta of one layer (0: not triggered), in Python integers."""
    if end <= first:
        return 0
    base = int(t[first - 1]) + 1 if first > 0 else 0
    delta = int(t[first]) - base
    return delta if delta > 0 and int(t[end - 1]) >= limit else 0


def angles(delta: int, inv_freq) -> np.ndarray:
    """theta64 [D/2] = double(fl32(fl32(delta) * inv_freq[d]))."""
    return (np.float32(delta) * np.asarray(inv_freq, dtype=np.float32)).astype(np.float32).astype(np.float64)


def rotate(x, delta: int, inv_freq, P: int = 1, sections=None, theta=None) -> np.ndarray:
    """x [..., D] (any float array) -> R(-delta) x in float64 on the temporal pairs.  theta: the angles to use instead of
    `angles(delta, inv_freq)` (the composition test passes exact float64 products)."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[-1]
    h = D // 2
    th = angles(delta, inv_freq) if theta is None else np.asarray(theta, dtype=np.float64)
    c, s = np.cos(th), np.sin(th)
    on = temporal_pairs(D, P, sections)
    x1, x2 = x[..., :h], x[..., h:]
    o1 = np.where(on, x1 * c + x2 * s, x1)
    o2 = np.where(on, x2 * c - x1 * s, x2)
    return np.concatenate([o1, o2], axis=-1)


def rebase(ids, K, first: int, end: int, length: int, limit: int, inv_freq, sections=None):
    """One layer: ids int64 [P, cap], K [H, cap, D] -> (new ids, new K in float64, delta).  Rows [first, length) of K and
    ids [first, end) of row 0 change, and only if the layer triggers."""
    ids = np.array(ids, dtype=np.int64, copy=True)
    out = np.array(K, dtype=np.float64, copy=True)
    delta = decide(ids[0], first, end, limit)
    if delta:
        ids[0, first:end] -= delta
        out[:, first:length] = rotate(out[:, first:length], delta, inv_freq, ids.shape[0], sections)
    return ids, out, delta


def half_ulp(dtype_name: str, x) -> np.ndarray:
    """Half the spacing of the storage dtype at |x| (at the smallest normal's for anything below it)."""
    m, emin = FORMATS[dtype_name]
    ax = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** emin)))
    return 0.5 * 2.0 ** (np.maximum(e, emin) - m)


def bar(dtype_name: str, ref, x) -> np.ndarray:
    """The bound on |kernel - ref| per element: x [..., D] the values before the rotation, ref = rotate(x, ...)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    h = x.shape[-1] // 2
    mag = x[..., :h] + x[..., h:]
    return half_ulp(dtype_name, ref) + C * np.concatenate([mag, mag], axis=-1)

"""The streaming DPSelect rule (retake/dpselect_stream.py) restated in numpy over a GIVEN distance matrix: the
specification for several segments, which the reference - it processes a finished video - cannot supply.

Input: dis [T, N] fp32, row g the distances of global frame g (row 0 = 1.0).  Output per segment k = frames
[k S, min((k+1) S, T)): the kept frames' GLOBAL indices (ascending) and whether each is a peak.

    row    sync: r[g] = mean_n dis[g, n], summed as dpselect_select_kernel sums it (lane partials n = l, l + 64, ... in
           order, then the xor-shuffle tree over 64 lanes, then / N, all fp32); async: r_n[g] = dis[g, n]
    peak   g is a peak iff for every j in [g - w/2, g - w/2 + w - 1] ∩ [0, T): r[g] > r[j] for j < g, r[g] >= r[j] for j > g
    key    r[g] + 2.0 (fp32) for a peak, else r[g]
    keep   max(1, round(ratio * len)) (python's round) or min(keep, len); the top keys of the segment, ties to the lowest
           index, emitted ascending; mask = peak
"""
import numpy as np


def patch_mean(dis: np.ndarray) -> np.ndarray:
    """dis.mean(1) in the kernel's summation order, fp32 throughout."""
    T, N = dis.shape
    part = np.zeros((T, 64), dtype=np.float32)
    for n in range(N):                       # lane l accumulates n = l, l + 64, ... in order
        part[:, n % 64] = part[:, n % 64] + dis[:, n]
    o = 32
    while o:                                 # v += shfl_xor(v, o): every lane ends with the same tree sum
        part = part + part[:, np.arange(64) ^ o]
        o >>= 1
    return part[:, 0] / np.float32(N)


def peaks(r: np.ndarray, window: int) -> np.ndarray:
    """r [T] -> bool [T], windows clipped at 0 and T - 1 only."""
    T = r.shape[0]
    out = np.zeros(T, dtype=bool)
    for g in range(T):
        a = max(g - window // 2, 0)
        b = min(g - window // 2 + window - 1, T - 1)
        out[g] = all((r[g] > r[j]) if j < g else (r[g] >= r[j]) for j in range(a, b + 1) if j != g)
    return out


def keep_count(length: int, ratio=None, keep=None) -> int:
    return min(keep, length) if keep is not None else max(1, round(ratio * length))


def _select_row(r: np.ndarray, S: int, window: int, ratio, keep):
    """One row over the whole stream -> per segment (global idx ascending, mask)."""
    T = r.shape[0]
    pk = peaks(r, window)
    key = np.where(pk, r + np.float32(2.0), r).astype(np.float32)
    out = []
    for first in range(0, T, S):
        length = min(S, T - first)
        k = keep_count(length, ratio, keep)
        order = np.argsort(-key[first:first + length], kind="stable")[:k]   # stable: ties to the lowest index
        idx = np.sort(order) + first
        out.append((idx.astype(np.int64), pk[idx]))
    return out


def select_stream(dis: np.ndarray, S: int, window: int, sync: bool, ratio=None, keep=None):
    """dis [T, N] -> list over segments of (idx, mask): sync idx [keep_k], async idx [keep_k, N]; mask [keep_k, N]."""
    dis = np.asarray(dis, dtype=np.float32)
    T, N = dis.shape
    if sync:
        return [(idx, np.repeat(m[:, None], N, axis=1)) for idx, m in _select_row(patch_mean(dis), S, window, ratio, keep)]
    cols = [_select_row(np.ascontiguousarray(dis[:, n]), S, window, ratio, keep) for n in range(N)]
    return [(np.stack([cols[n][s][0] for n in range(N)], axis=1), np.stack([cols[n][s][1] for n in range(N)], axis=1))
            for s in range(len(cols[0]))]

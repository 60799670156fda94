"""float64 torch restatement of prompt-guided PivotKV (kvcache_compression_kwargs["prompt_guided_scoring"]): no call into
the library.  A chunk of L rows is Lv = L - Lp video rows followed by the Lp rows of the appended prompt.

  score      score[j] = mean_g mean_{h in g} (1/Lp) sum_{i in [Lv, L)} softmax_{j' in [0, Lv)}(q~[h,i] . k~[g,j'] / sqrt(D))[j]
             for the video keys j < Lv: softmax over the video keys only, no causal mask, prompt keys never read.
  selection  keep = max(1, int(ratio * Lv)); the scores of masked video tokens (keypatches_mask_chunk[:Lv]) become 1.0 -
             every score is < 1, so they rank first; top-k over the Lv columns, ties lowest index first, ascending.
  ids        the kept columns of the chunk's ids; with reforge the temporal row becomes
             tmin + int64(float32(t - tmin) * float32(keep / Lv)), tmin = the smallest kept temporal id.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def operands(seed: int, Hq: int, Hkv: int, L: int, D: int, dtype, scale: float = 1.7):
    """q~ [Hq, L, D], k~ [Hkv, L, D] (CPU, `dtype`): scale * N(0, 1) like synth.qkv_chunk - peaked softmax rows."""
    rng = np.random.default_rng(seed)
    q = scale * rng.standard_normal((Hq, L, D), dtype=np.float32)
    k = scale * rng.standard_normal((Hkv, L, D), dtype=np.float32)
    return torch.from_numpy(q).to(dtype), torch.from_numpy(k).to(dtype)


def scores(q: torch.Tensor, k: torch.Tensor, Lp: int) -> torch.Tensor:
    """q [Hq, L, D], k [Hkv, L, D] (any float dtype, any device) -> float64 [Lv]: the exact score of these operands."""
    Hq, L, D = q.shape
    Hkv = k.shape[0]
    G, Lv = Hq // Hkv, L - Lp
    assert 0 < Lp < L and Hq == G * Hkv
    qp = q[:, Lv:].double().reshape(Hkv, G, Lp, D)
    kv = k[:, :Lv].double()
    logits = torch.einsum("ghid,gjd->ghij", qp, kv) / math.sqrt(D)
    p = torch.softmax(logits, dim=-1)               # over the video keys
    return (p.sum(2) / Lp).mean(1).mean(0)          # rows, heads of the group, groups


def keep_len(ratio: float, Lv: int) -> int:
    return max(1, int(ratio * Lv))


def select(score: torch.Tensor, keep: int, mask=None) -> torch.Tensor:
    """score [Lv] -> the kept video columns [keep] int64, ascending (mask: bool with at least Lv entries, or None)."""
    s = score.clone()
    if mask is not None:
        s[mask[:s.numel()].to(device=s.device, dtype=torch.bool)] = 1.0
    order = torch.sort(s, descending=True, stable=True).indices   # ties: lowest index first
    return torch.sort(order[:keep]).values


def threshold_band(score: torch.Tensor, keep: int, width: float, mask=None) -> torch.Tensor:
    """bool [Lv]: the unmasked tokens whose score lies within `width` of the threshold (the keep-th largest score after
    the mask override) - the only tokens an approximate score may rank differently."""
    s = score.clone()
    free = torch.ones_like(s, dtype=torch.bool)
    if mask is not None:
        m = mask[:s.numel()].to(device=s.device, dtype=torch.bool)
        s[m] = 1.0
        free = ~m
    thr = torch.sort(s, descending=True).values[keep - 1]
    return free & ((s - thr).abs() <= width)


def new_ids(ids: torch.Tensor, keep_idx: torch.Tensor, Lv: int, reforge: bool) -> torch.Tensor:
    """ids [P, L] int64 of the chunk -> [P, keep] ids of the kept video rows."""
    out = ids[:, keep_idx.to(ids.device)].clone()
    if reforge:
        keep = keep_idx.numel()
        t = out[0]
        tmin = t.min()
        ratio = torch.tensor(keep / Lv, dtype=torch.float32, device=ids.device)
        out[0] = tmin + ((t - tmin).to(torch.float32) * ratio).to(torch.int64)
    return out

"""The reference's small torch helpers (its longvideo_cache.py:16-116): repeat_kv, rotate_half and the two
apply_*rotary_pos_emb.  The attention patches use them on the current chunk; the cache's hot path does not."""
from __future__ import annotations

import torch


def repeat_kv(hidden_states: torch.Tensor, n_rep: int) -> torch.Tensor:
    """[B, Hkv, L, D] -> [B, Hkv*n_rep, L, D]  (longvideo_cache.py:16-25)."""
    b, h, s, d = hidden_states.shape
    if n_rep == 1:
        return hidden_states
    return hidden_states[:, :, None, :, :].expand(b, h, n_rep, s, d).reshape(b, h * n_rep, s, d)


def rotate_half(x):
    """cat(-x[D/2:], x[:D/2])  (longvideo_cache.py:28-32)."""
    half = x.shape[-1] // 2
    return torch.cat((-x[..., half:], x[..., :half]), dim=-1)


def _rotate(q, k, cos, sin, reverse, attention_scaling):
    if reverse:  # rotate towards the opposite direction (longvideo_cache.py:76-78)
        q_embed = ((q * cos) - (rotate_half(q) * sin)) / attention_scaling ** 2
        k_embed = ((k * cos) - (rotate_half(k) * sin)) / attention_scaling ** 2
    else:
        q_embed = (q * cos) + (rotate_half(q) * sin) if q is not None else None
        k_embed = (k * cos) + (rotate_half(k) * sin) if k is not None else None
    return q_embed, k_embed


def apply_multimodal_rotary_pos_emb(q, k, cos, sin, mrope_section, unsqueeze_dim=1, reverse=False,
                                    attention_scaling=1):
    """M-RoPE with the reference's extra `reverse` / `attention_scaling` arguments (longvideo_cache.py:35-83)."""
    sections = mrope_section * 2
    cos = torch.cat([m[i % 3] for i, m in enumerate(cos.split(sections, dim=-1))], dim=-1).unsqueeze(unsqueeze_dim)
    sin = torch.cat([m[i % 3] for i, m in enumerate(sin.split(sections, dim=-1))], dim=-1).unsqueeze(unsqueeze_dim)
    return _rotate(q, k, cos, sin, reverse, attention_scaling)


def apply_rotary_pos_emb(q, k, cos, sin, position_ids=None, unsqueeze_dim=1, reverse=False, attention_scaling=1):
    """1-D RoPE with `reverse` / `attention_scaling` (longvideo_cache.py:86-116)."""
    return _rotate(q, k, cos.unsqueeze(unsqueeze_dim), sin.unsqueeze(unsqueeze_dim), reverse, attention_scaling)

"""BranchGroup: the forks of one PivotKVCache (PivotKVCache.fork) decoding one token each, with ONE attention launch per
layer that reads the rows they share once (rtk_attention_decode_group) instead of once per branch.  Not in the reference,
which prefills the video again for every question.

A group is handed to a patched model as `past_key_values` with `input_ids [B, 1]` and per-branch position ids
(INTEGRATION.md §1); `group_attention_forward` is what the four attention patches call for it.  Everything else about a
member - its question's prefill, `mark` / `rewind` / `crop`, its validity against the parent - stays the member's own."""
from __future__ import annotations

from typing import Sequence

import torch

from . import _native as nv
from .native_attention import group_decode_attention


class BranchGroup:
    """branches: PivotKVCache forks of ONE parent at ONE mark (the same `forked_from` object, hence the same shared views
    and archive), in the order of the batch rows.  ValueError names the first member that is not; a fork whose parent has
    given up the shared rows raises what every call on it raises (PivotKVCache._branch_check)."""

    def __init__(self, branches: Sequence):
        self.members = list(branches)
        if not self.members:
            raise ValueError("BranchGroup needs at least one branch")
        mark = getattr(self.members[0], "forked_from", None)
        for i, br in enumerate(self.members):
            m = getattr(br, "forked_from", None)
            if m is None:
                raise ValueError(f"BranchGroup: member {i} is not a branch (PivotKVCache.fork)")
            if m is not mark:
                raise ValueError(f"BranchGroup: member {i} was forked from another parent or at another mark than member 0")
            if any(br is other for other in self.members[:i]):
                raise ValueError(f"BranchGroup: member {i} is in the group twice")
            br._branch_check("BranchGroup")
        self.group_attention_calls = 0      # `attention` calls so far
        self.group_attention_launches = 0   # ... and the group launches they made (more when a group had to be split)
        self._ws = {}

    def __len__(self):
        return len(self.members)

    def __getitem__(self, i):
        return self.members[i]

    def get_seq_length(self, layer_idx: int = 0) -> int:
        """The longest member's: HF reads it for the width of the mask only."""
        return max(br.get_seq_length(layer_idx) for br in self.members)

    def _own(self, br, layer_idx):
        st = br._layers[layer_idx]
        n = st.length
        return st.k.narrow(2, 0, n), st.v.narrow(2, 0, n)

    def attention(self, query_states, layer_idx, scaling=None):
        """query_states [B, Hq, 1, D], row b the rotated query of member b's newest own row -> [B, 1, Hq, D]: member b's
        attention over [archive | shared | its own rows] in one group launch.  A group the library declines for its size
        (5 branches at Hq / Hkv = 7) is served as the largest sub-groups that fit, in member order; a member's output
        bits do not depend on the split (include/retake_hip.h).  NotImplementedError for anything else it declines: no
        other route reads the shared rows."""
        B = len(self.members)
        if query_states.dim() != 4 or query_states.shape[0] != B or query_states.shape[2] != 1:
            raise ValueError(f"BranchGroup.attention takes [{B}, Hq, 1, D] queries, one row per member")
        for br in self.members:
            br._branch_check("BranchGroup.attention")
        first = self.members[0]
        shared, archive = first.shared(layer_idx), first.archive(layer_idx)
        owns = [self._own(br, layer_idx) for br in self.members]
        Hq, Hkv = query_states.shape[1], owns[0][0].shape[1]
        fit = max(1, min(nv.DECODE_GROUP_MAX, 32 // max(1, Hq // Hkv)))   # the library's envelope, restated
        outs = []
        for lo in range(0, B, fit):
            hi = min(B, lo + fit)
            out = group_decode_attention([query_states[b:b + 1] for b in range(lo, hi)], owns[lo:hi], shared, archive,
                                         scaling=scaling, workspace=self._ws)
            if out is None:
                raise NotImplementedError("BranchGroup.attention: the group kernel refuses this call "
                                          f"({nv.lib.rtk_last_error().decode(errors='replace')}) and no other route reads "
                                          "the rows the branches share")
            self.group_attention_launches += 1
            outs.append(out)
        self.group_attention_calls += 1
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def decode_step(self, query_states, key_states, value_states, layer_idx, position_ids, rotary_emb, mrope_section=None,
                    scaling=None, shift_ids_in_place=True):
        """One decode step of every member in a layer: query_states [B, Hq, 1, D], key_states / value_states
        [B, Hkv, 1, D] before RoPE, position_ids [3, B, 1] (M-RoPE) or [B, 1].  Member b's `append_pre_rope` on row b
        (the kernel, the cache rows and the ids a step of that member alone would leave), then one `attention`."""
        B = len(self.members)
        if query_states.dim() != 4 or query_states.shape[0] != B or query_states.shape[2] != 1:
            raise ValueError(f"BranchGroup.decode_step takes one new token per member: [{B}, H, 1, D] states")
        for b, br in enumerate(self.members):
            pos = position_ids[:, b:b + 1] if position_ids.dim() == 3 else position_ids[b:b + 1]
            out = br.append_pre_rope(query_states[b:b + 1], key_states[b:b + 1], value_states[b:b + 1], layer_idx, pos,
                                     rotary_emb, mrope_section, shift_ids_in_place=shift_ids_in_place)
            if out is None:
                raise NotImplementedError(f"BranchGroup.decode_step: member {b}'s append_pre_rope does not serve this call "
                                          "(it needs pos_embed_reforge, a native rotary module and GPU tensors), and no "
                                          "other route reads the rows the branches share")
        return self.attention(query_states, layer_idx, scaling=scaling)   # (rotated in place, row by row)


def group_attention_forward(module, hidden_states, position_ids, group, mrope_section=None, scaling=None,
                            shift_ids_in_place=True, output_attentions=False):
    """What the attention patches run when `past_key_value` is a BranchGroup, in place of prologue + native_attention:
    the projections, `group.decode_step`, o_proj.  [B, 1, hidden]."""
    bsz, q_len, _ = hidden_states.shape
    if q_len != 1 or bsz != len(group):
        raise ValueError(f"a BranchGroup of {len(group)} branches takes hidden states [{len(group)}, 1, hidden] - one new "
                         f"token per branch - got [{bsz}, {q_len}, ...]")
    if output_attentions or position_ids is None or (module.training and getattr(module, "attention_dropout", 0.0)):
        raise NotImplementedError("a BranchGroup is served by the group kernel alone: no attention weights, no dropout, and "
                                  "the per-branch position ids are needed")
    shape = (bsz, 1, -1, module.head_dim)
    q = module.q_proj(hidden_states).view(shape).transpose(1, 2)
    k = module.k_proj(hidden_states).view(shape).transpose(1, 2)
    v = module.v_proj(hidden_states).view(shape).transpose(1, 2)
    out = group.decode_step(q, k, v, module.layer_idx, position_ids, module.rotary_emb, mrope_section, scaling=scaling,
                            shift_ids_in_place=shift_ids_in_place)
    return module.o_proj(out.reshape(bsz, 1, -1))

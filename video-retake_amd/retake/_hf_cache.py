"""Which `DynamicCache` PivotKVCache subclasses, chosen once at import.  The reference subclasses transformers 4.48's
list-based class (public `key_cache` / `value_cache` lists; its longvideo_cache.py:119-144): HF's own while it still is
that one (`generate` checks isinstance against it), else - or without transformers - the stand-in `_ListDynamicCache`."""
from __future__ import annotations

from typing import List

import torch

try:  # the HF classes are third-party; they only matter for isinstance checks inside `generate`
    from transformers.cache_utils import DynamicCache as _HFDynamicCache
except Exception:  # noqa: BLE001
    _HFDynamicCache = None


def _hf_dynamic_cache_is_legacy() -> bool:
    if _HFDynamicCache is None:
        return False
    try:
        return hasattr(_HFDynamicCache(), "key_cache")
    except Exception:  # noqa: BLE001
        return False


class _ListDynamicCache:
    """Minimal stand-in used when the installed transformers no longer has the 4.48 list-based
    DynamicCache the reference subclasses (third-party API, restated from its documentation)."""

    def __init__(self, *args, **kwargs) -> None:
        self.key_cache: List[torch.Tensor] = []
        self.value_cache: List[torch.Tensor] = []
        self._seen_tokens = 0

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        if layer_idx == 0:
            self._seen_tokens += key_states.shape[-2]
        if len(self.key_cache) <= layer_idx:
            for _ in range(len(self.key_cache), layer_idx):
                self.key_cache.append([])
                self.value_cache.append([])
            self.key_cache.append(key_states)
            self.value_cache.append(value_states)
        elif len(self.key_cache[layer_idx]) == 0:
            self.key_cache[layer_idx] = key_states
            self.value_cache[layer_idx] = value_states
        else:
            self.key_cache[layer_idx] = torch.cat([self.key_cache[layer_idx], key_states], dim=-2)
            self.value_cache[layer_idx] = torch.cat([self.value_cache[layer_idx], value_states], dim=-2)
        return self.key_cache[layer_idx], self.value_cache[layer_idx]

    def get_seq_length(self, layer_idx: int = 0) -> int:
        if len(self.key_cache) <= layer_idx or len(self.key_cache[layer_idx]) == 0:
            return 0
        return self.key_cache[layer_idx].shape[-2]

    def get_max_cache_shape(self):
        return None

    def get_max_length(self):
        return None

    def __len__(self):
        return len(self.key_cache)

    def __getitem__(self, layer_idx):
        return self.key_cache[layer_idx], self.value_cache[layer_idx]

    def __iter__(self):
        for i in range(len(self)):
            yield self.key_cache[i], self.value_cache[i]


DynamicCache = _HFDynamicCache if _hf_dynamic_cache_is_legacy() else _ListDynamicCache

"""retake.longvideo_cache split by role: the module keeps exporting every name its callers use, each moved name is the
new module's own object, none of the new modules imports longvideo_cache (no import cycle), and the option validators
of build_kvcache keep their message texts."""
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOVED = {
    "_rope_torch": ("repeat_kv", "rotate_half", "_rotate", "apply_multimodal_rotary_pos_emb", "apply_rotary_pos_emb"),
    "_hf_cache": ("DynamicCache", "_ListDynamicCache", "_hf_dynamic_cache_is_legacy"),
    "_cache_state": ("_LayerStore", "_Side", "_Update", "_Rotary", "_version_of", "_on_device", "_inv_stamp", "_Batch",
                     "_CacheView", "_LayerMark", "CacheMark"),
    "native_attention": ("chunk_attention", "fp8_quantize_rows", "fp8_dequantize_rows", "native_attention",
                         "ATTENTION_KERNELS", "KV_CACHE_DTYPES"),
}
# what bench.py, tests/, tools/ and __graft_entry__.py read off retake.longvideo_cache
USED = ("build_kvcache", "PivotKVCache", "CacheMark", "DynamicCache", "chunk_attention", "native_attention",
        "fp8_quantize_rows", "fp8_dequantize_rows", "repeat_kv", "rotate_half", "apply_rotary_pos_emb",
        "apply_multimodal_rotary_pos_emb", "_version_of", "_inv_stamp", "torch", "__file__")


def test_longvideo_cache_exports_what_its_callers_use():
    import torch

    import retake.longvideo_cache as lc

    for name in USED:
        assert hasattr(lc, name), name
    assert lc.torch is torch
    assert lc.__all__ == ["repeat_kv", "rotate_half", "apply_multimodal_rotary_pos_emb", "apply_rotary_pos_emb",
                          "PivotKVCache", "CacheMark", "build_kvcache", "DynamicCache"]


def test_moved_names_are_the_new_modules_objects():
    import importlib

    import retake.longvideo_cache as lc

    home = {name: mod for mod, names in MOVED.items() for name in names}
    assert all(name in home or name in ("build_kvcache", "PivotKVCache", "torch", "__file__") for name in USED)
    for name, mod in home.items():
        assert getattr(lc, name) is getattr(importlib.import_module("retake." + mod), name), name
    assert issubclass(lc.PivotKVCache, lc.DynamicCache) and lc.PivotKVCache.__module__ == "retake.longvideo_cache"


def test_new_modules_import_alone_and_never_import_longvideo_cache():
    """A fresh interpreter imports each new module on its own - the package is dropped from sys.modules between two of
    them, so each import starts from nothing of `retake` - and none of them pulls in retake.longvideo_cache."""
    code = """
import importlib, sys
sys.path.insert(0, sys.argv[1])
for mod in sys.argv[2:]:
    for name in [n for n in sys.modules if n == "retake" or n.startswith("retake.")]:
        del sys.modules[name]
    importlib.import_module("retake." + mod)
    assert "retake." + mod in sys.modules
    assert "retake.longvideo_cache" not in sys.modules, mod + " imports retake.longvideo_cache"
print("alone:", *sys.argv[2:])
"""
    r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "video-retake_amd"), *MOVED],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "alone: " + " ".join(MOVED), r.stdout


@pytest.mark.parametrize("key, value, text", [
    ("attention_kernel", "triton", "attention_kernel must be None or 'hip', got 'triton'"),
    ("decode_attention", "split", "decode_attention must be None or 'packed', got 'split'"),
    ("kv_cache_dtype", "fp4", "kv_cache_dtype must be None or 'fp8_e4m3', got 'fp4'"),
])
def test_option_validator_messages(key, value, text):
    import retake.longvideo_cache as lc

    cfg = types.SimpleNamespace(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                                longvideo_kwargs={"kvcache_compression": True, key: value,
                                                  "kvcache_compression_kwargs": {"compression_ratio": 0.5,
                                                                                 "compression_method": "pivotkv"}})
    with pytest.raises(ValueError) as e:
        lc.build_kvcache(cfg)
    assert str(e.value) == text

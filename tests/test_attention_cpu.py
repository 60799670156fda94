"""CPU-side checks of the native chunk attention (include/retake_hip.h "Chunk attention"): host-side argument validation
of the two entry points, the opt-in switch, the no-CPU-fallback rule, and the precondition of the mask-free route."""
import glob
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000   # a 16-byte aligned non-NULL "pointer": every call below is rejected on the host, before any launch


def _fwd(nv, q=P, qsh=128, qsl=128, k=P, v=P, ksh=128 * 64, ksl=128, out=P, Hq=28, Hkv=4, Lq=8, Lk=64, off=None, D=128,
         dtype=None, scale=0.1, ws=None, ws_bytes=0):
    dtype = nv.RTK_BF16 if dtype is None else dtype
    off = Lk - Lq if off is None else off
    return nv.lib.rtk_attention_forward(q, qsh, qsl, k, v, ksh, ksl, out, Hq, Hkv, Lq, Lk, off, D, dtype, scale, ws, ws_bytes,
                                        None)


def test_forward_argument_validation_without_gpu():
    import retake._native as nv

    err = nv.lib.rtk_last_error
    assert _fwd(nv, q=None) == nv.RTK_EINVAL and b"NULL" in err()
    assert _fwd(nv, out=None) == nv.RTK_EINVAL and b"NULL" in err()
    assert _fwd(nv, Hq=28, Hkv=5) == nv.RTK_EINVAL and b"not a multiple of Hkv" in err()
    assert _fwd(nv, Lq=65, Lk=64) == nv.RTK_EINVAL and b"Lk 64 < Lq 65" in err()
    assert _fwd(nv, Lq=8, Lk=64, off=55) == nv.RTK_EINVAL and b"q_offset" in err()
    assert _fwd(nv, scale=0.0) == nv.RTK_EINVAL and b"scale" in err()
    assert _fwd(nv, D=80 + 4) == nv.RTK_EUNSUPPORTED and b"head_dim 84" in err()
    assert _fwd(nv, D=264) == nv.RTK_EUNSUPPORTED and b"head_dim 264" in err()
    assert _fwd(nv, dtype=nv.RTK_BF16_REFROUND) == nv.RTK_EUNSUPPORTED and b"dtype" in err()
    assert _fwd(nv, q=P + 2) == nv.RTK_EUNSUPPORTED and b"layout" in err()
    # one head of k / v spanning 2 GiB: Lk rows at a row stride of 2^20 elements
    assert _fwd(nv, Lk=1024, ksl=1 << 20) == nv.RTK_EUNSUPPORTED and b"2 GiB" in err()
    # decode over a long cache is key-split: the partials need the caller's workspace
    need = nv.lib.rtk_attention_workspace_bytes(28, 4, 1, 100352, 128, nv.RTK_BF16)
    assert need > 0 and need % 4 == 0
    assert _fwd(nv, Lq=1, Lk=100352, ksh=128 * 100352) == nv.RTK_EWORKSPACE and b"workspace too small" in err()
    assert _fwd(nv, Lq=1, Lk=100352, ksh=128 * 100352, ws=P, ws_bytes=need - 4) == nv.RTK_EWORKSPACE
    with pytest.raises(NotImplementedError):
        nv.check(_fwd(nv, D=84), "rtk_attention_forward")
    with pytest.raises(ValueError):
        nv.check(_fwd(nv, Lq=65, Lk=64), "rtk_attention_forward")


def test_workspace_query_validation_and_shape_only_split():
    import retake._native as nv

    wb = nv.lib.rtk_attention_workspace_bytes
    assert wb(28, 5, 1, 64, 128, nv.RTK_BF16) == 0 and b"not a multiple of Hkv" in nv.lib.rtk_last_error()
    assert wb(28, 4, 65, 64, 128, nv.RTK_BF16) == 0 and b"Lk 64 < Lq 65" in nv.lib.rtk_last_error()
    assert wb(28, 4, 1, 64, 84, nv.RTK_BF16) == 0 and b"head_dim" in nv.lib.rtk_last_error()
    # a chunk fills the chip by itself: no split, no workspace
    for Lq, Lk in ((2304, 2304), (2304, 2304 + 7488), (6272, 6272 + 98784)):
        assert wb(28, 4, Lq, Lk, 128, nv.RTK_BF16) == 0
        assert wb(28, 4, Lq, Lk, 128, nv.RTK_F16) == 0
    # few rows over many keys: split, sized [splits][Hq][Lq][D + 2] fp32, the same answer every time (shape only)
    a = wb(28, 4, 5, 100352, 128, nv.RTK_BF16)
    assert a > 0 and a % (28 * 5 * 130 * 4) == 0 and a == wb(28, 4, 5, 100352, 128, nv.RTK_BF16)
    assert wb(4, 2, 1, 73, 16, nv.RTK_F32) == 0     # the tiny-head fixtures: too few keys to split


def _cfg(**top):
    kw = {"kvcache_compression": True,
          "kvcache_compression_kwargs": {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    kw.update(top)
    return types.SimpleNamespace(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=kw)


def test_attention_kernel_switch():
    import retake.longvideo_cache as lc

    assert lc.build_kvcache(_cfg()).attention_kernel is None          # default: today's behaviour
    assert lc.build_kvcache(_cfg(attention_kernel=None)).attention_kernel is None
    cache = lc.build_kvcache(_cfg(attention_kernel="hip"))
    assert cache.attention_kernel == "hip" and callable(cache.attention) and cache.attention_calls == 0
    assert cache.memory_footprint()["attention_workspace"] == 0 and cache.memory_footprint()["total"] == 0
    with pytest.raises(ValueError, match="attention_kernel"):
        lc.build_kvcache(_cfg(attention_kernel="cuda"))


def test_chunk_attention_has_no_cpu_fallback():
    import retake.longvideo_cache as lc

    q, k = torch.randn(1, 4, 3, 16), torch.randn(1, 2, 8, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lc.chunk_attention(q, k, k.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lc.build_kvcache(_cfg(attention_kernel="hip")).attention(q, k, k.clone())


def test_native_route_is_not_taken_off_the_gpu_or_without_the_switch():
    """The patches' gate: with the switch off, or on CPU tensors, `native_attention` returns None (the existing route)
    without touching the cache's entry point."""
    import retake.longvideo_cache as lc

    mod = types.SimpleNamespace(training=False, attention_dropout=0.0, layer_idx=0,
                                config=types.SimpleNamespace(use_sliding_window=False, sliding_window=None, max_window_layers=0))
    q, k = torch.randn(1, 4, 3, 16), torch.randn(1, 2, 8, 16)
    mask = torch.zeros(1, 1, 3, 8)
    assert lc.native_attention(mod, lc.build_kvcache(_cfg()), q, k, k, mask) is None
    cache = lc.build_kvcache(_cfg(attention_kernel="hip"))
    assert lc.native_attention(mod, cache, q, k, k, mask) is None and cache.attention_calls == 0


def test_recorded_masks_are_causal_over_their_own_width():
    """Precondition of the mask-free route: every 4-D additive mask the reference's runs recorded is exactly 0 where
    j <= (T - Lq) + i and below -1e30 elsewhere, T being the mask's own width (HF builds it over the uncompressed
    positions) - so its width alone says what it masks."""
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "glue_attention_*.npz")))
    files = [f for f in files if not f.endswith("_fa2_sliding.npz")]
    assert len(files) == 7
    n = 0
    for f in files:
        g = np.load(f, allow_pickle=False)
        for name in sorted(x for x in g.files if x.endswith("_mask4")):
            m = g[name]
            assert m.ndim == 4 and m.shape[:2] == (1, 1)
            Lq, T = m.shape[2:]
            vis = np.arange(T)[None, :] <= (T - Lq) + np.arange(Lq)[:, None]
            assert (m[0, 0][vis] == 0).all(), (f, name)
            assert (m[0, 0][~vis] < -1e30).all(), (f, name)
            n += 1
    assert n == 35

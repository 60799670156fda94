"""CPU-side checks of the GQA-packed few-row attention (include/retake_hip.h rtk_attention_decode, rtk_attention_decode_fp8kv):
host-side argument validation of the entry points, the shape-only split plan, the opt-in switch and the no-CPU-fallback
rule.  Nothing here launches a kernel."""
import types

import pytest
import torch

P = 0x10000   # a 16-byte aligned non-NULL "pointer": every call below is rejected on the host, before any launch


def _dec(nv, q=P, qsh=128, qsl=128, k=P, v=P, ksh=128 * 64, ksl=128, out=P, Hq=28, Hkv=4, Lq=2, Lk=64, off=None, D=128,
         dtype=None, scale=0.1, ws=None, ws_bytes=0):
    dtype = nv.RTK_BF16 if dtype is None else dtype
    off = Lk - Lq if off is None else off
    return nv.lib.rtk_attention_decode(q, qsh, qsl, k, v, ksh, ksl, out, Hq, Hkv, Lq, Lk, off, D, dtype, scale, ws, ws_bytes, None)


def _dec8(nv, q=P, qsh=128, qsl=128, k=P, v=P, ksh=128 * 64, ksl=128, out=P, Hq=28, Hkv=4, Lq=2, Lk=64, off=None, D=128,
          dtype=None, scale=0.1, ws=None, ws_bytes=0, L8=128):
    """The same call through the two-segment entry point, over an archive of L8 rows."""
    dtype = nv.RTK_BF16 if dtype is None else dtype
    off = Lk - Lq if off is None else off
    return nv.lib.rtk_attention_decode_fp8kv(q, qsh, qsl, k, v, ksh, ksl, P, P, P, P, L8, 128 * L8, L8, out, Hq, Hkv, Lq, Lk, off,
                                             D, dtype, scale, ws, ws_bytes, None)


@pytest.mark.parametrize("fwd,query", [(_dec, "rtk_attention_decode_workspace_bytes"),
                                       (_dec8, "rtk_attention_decode_workspace_bytes_fp8kv")], ids=["16bit", "fp8kv"])
def test_decode_argument_validation_without_gpu(fwd, query):
    """The cases of test_forward_argument_validation_without_gpu (tests/test_attention_cpu.py) at Lq 2 - inside the packed
    envelope, so that each reaches the check it is about - and the envelope's own refusals."""
    import retake._native as nv

    err = nv.lib.rtk_last_error
    assert fwd(nv, q=None) == nv.RTK_EINVAL and b"NULL" in err()
    assert fwd(nv, out=None) == nv.RTK_EINVAL and b"NULL" in err()
    assert fwd(nv, Hq=28, Hkv=5) == nv.RTK_EINVAL and b"not a multiple of Hkv" in err()
    assert fwd(nv, Lq=65, Lk=64) == nv.RTK_EINVAL and b"Lk 64 < Lq 65" in err()
    assert fwd(nv, Lq=2, Lk=64, off=61) == nv.RTK_EINVAL and b"q_offset" in err()
    assert fwd(nv, scale=0.0) == nv.RTK_EINVAL and b"scale" in err()
    assert fwd(nv, D=80 + 4) == nv.RTK_EUNSUPPORTED and b"head_dim 84" in err()
    assert fwd(nv, D=264) == nv.RTK_EUNSUPPORTED and b"head_dim 264" in err()
    assert fwd(nv, dtype=nv.RTK_BF16_REFROUND) == nv.RTK_EUNSUPPORTED and b"dtype" in err()
    assert fwd(nv, q=P + 2) == nv.RTK_EUNSUPPORTED and b"layout" in err()
    assert fwd(nv, Lk=1024, ksl=1 << 20) == nv.RTK_EUNSUPPORTED and b"2 GiB" in err()
    # the partials always live in the caller's workspace
    if fwd is _dec:
        need = nv.lib.rtk_attention_decode_workspace_bytes(28, 4, 1, 100352, 128, nv.RTK_BF16)
    else:
        need = nv.lib.rtk_attention_decode_workspace_bytes_fp8kv(28, 4, 1, 100352, 128, 128, nv.RTK_BF16)
    assert need > 0 and need % 4 == 0
    assert fwd(nv, Lq=1, Lk=100352, ksh=128 * 100352) == nv.RTK_EWORKSPACE and b"workspace too small" in err()
    assert query.encode() in err()
    assert fwd(nv, Lq=1, Lk=100352, ksh=128 * 100352, ws=P, ws_bytes=need - 4) == nv.RTK_EWORKSPACE
    # outside the envelope: the caller makes the existing call
    assert fwd(nv, Hq=28, Hkv=4, Lq=3) == nv.RTK_EUNSUPPORTED and b"packed rows" in err()      # G * Lq = 21
    assert fwd(nv, dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and b"dtype" in err()
    assert fwd(nv, D=64) == nv.RTK_EUNSUPPORTED and b"head_dim" in err()
    with pytest.raises(NotImplementedError):
        nv.check(fwd(nv, Lq=3), "rtk_attention_decode")
    with pytest.raises(ValueError):
        nv.check(fwd(nv, Lq=65, Lk=64), "rtk_attention_decode")


def test_fp8kv_entry_point_own_checks():
    import retake._native as nv

    err = nv.lib.rtk_last_error
    assert _dec8(nv, L8=-1) == nv.RTK_EINVAL and b"L8" in err()
    rc = nv.lib.rtk_attention_decode_fp8kv(P, 128, 128, P, P, 128 * 64, 128, None, P, P, P, 64, 128 * 64, 64, P, 28, 4, 2, 64, 62,
                                           128, nv.RTK_BF16, 0.1, None, 0, None)
    assert rc == nv.RTK_EINVAL and b"NULL archive pointer" in err()
    # L8 == 0 is the 16-bit packed call: its workspace, its message
    assert nv.lib.rtk_attention_decode_workspace_bytes_fp8kv(28, 4, 1, 4000, 0, 128, nv.RTK_BF16) == \
        nv.lib.rtk_attention_decode_workspace_bytes(28, 4, 1, 4000, 128, nv.RTK_BF16)
    assert _dec8(nv, L8=0) == nv.RTK_EWORKSPACE and b"rtk_attention_decode:" in err()


def _plan(Hkv, K):
    """The rule of include/retake_hip.h (rtk_attention_decode), restated: (nsplit, keys per split)."""
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    n0 = max(1, min(ceil(512, Hkv), ceil(K, 128)))
    kps = 128 * ceil(ceil(K, n0), 128)
    return ceil(K, kps), kps


def test_workspace_query_and_the_shape_only_plan():
    import retake._native as nv

    wb, wb8 = nv.lib.rtk_attention_decode_workspace_bytes, nv.lib.rtk_attention_decode_workspace_bytes_fp8kv
    err = nv.lib.rtk_last_error
    assert wb(28, 5, 1, 64, 128, nv.RTK_BF16) == 0 and b"not a multiple of Hkv" in err()
    assert wb(28, 4, 65, 64, 128, nv.RTK_BF16) == 0 and b"Lk 64 < Lq 65" in err()
    assert wb(28, 4, 1, 64, 84, nv.RTK_BF16) == 0 and b"head_dim" in err()
    assert wb(28, 4, 3, 64, 128, nv.RTK_BF16) == 0 and b"packed rows" in err()
    assert wb(28, 4, 1, 64, 128, nv.RTK_F32) == 0 and b"dtype" in err()
    assert wb(28, 4, 1, 64, 64, nv.RTK_BF16) == 0 and b"head_dim" in err()
    assert wb8(28, 4, 3, 64, 128, 128, nv.RTK_BF16) == 0 and b"packed rows" in err()
    assert wb8(28, 4, 1, 64, -1, 128, nv.RTK_BF16) == 0 and b"L8" in err()
    row = 28 * 1 * 130 * 4
    a = wb(28, 4, 1, 100352, 128, nv.RTK_BF16)
    assert a > 0 and a % row == 0 and a == wb(28, 4, 1, 100352, 128, nv.RTK_BF16) == wb(28, 4, 1, 100352, 128, nv.RTK_F16)
    assert a // row == _plan(4, 100352)[0] == 112
    for Lk in list(range(1, 3001)) + [100352]:
        got = wb(28, 4, 1, Lk, 128, nv.RTK_BF16)
        assert got % row == 0
        ns, kps = _plan(4, Lk)
        assert got // row == ns, Lk
        # the splits [s kps, min(Lk, (s + 1) kps)) tile [0, Lk): none empty, none overlapping, every key covered
        assert kps % 128 == 0 and (ns - 1) * kps < Lk <= ns * kps, Lk
    # the archive counts padded to the key tile T = 32
    for L8, Lk in ((640, 70), (624, 1), (59, 70), (100288, 64), (1, 1)):
        ns, _ = _plan(4, Lk + -(-L8 // 32) * 32)
        assert wb8(28, 4, 1, Lk, L8, 128, nv.RTK_BF16) == ns * row


def _cfg(**top):
    kw = {"kvcache_compression": True,
          "kvcache_compression_kwargs": {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    kw.update(top)
    return types.SimpleNamespace(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=kw)


def test_decode_attention_switch():
    import retake.longvideo_cache as lc

    assert lc.build_kvcache(_cfg()).decode_attention is None
    assert lc.build_kvcache(_cfg(attention_kernel="hip")).decode_attention is None
    assert lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention=None)).decode_attention is None
    with pytest.raises(ValueError, match="decode_attention"):
        lc.build_kvcache(_cfg(decode_attention="packed"))                      # needs attention_kernel="hip"
    with pytest.raises(ValueError, match="decode_attention"):
        lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention="flash"))
    with pytest.raises(ValueError, match="decode_attention"):
        lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention=True))
    cache = lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention="packed"))
    assert cache.decode_attention == "packed" and cache.attention_kernel == "hip"
    assert cache.decode_attention_calls == 0 and cache.attention_calls == 0
    assert cache.memory_footprint()["attention_workspace"] == 0 and cache.memory_footprint()["total"] == 0


def test_no_cpu_fallback():
    import retake.longvideo_cache as lc

    q = torch.zeros((1, 28, 1, 128), dtype=torch.bfloat16)
    k = torch.zeros((1, 4, 64, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lc.chunk_attention(q, k, k, packed_gqa=True)
    cache = lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention="packed"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.attention(q, k, k)
    assert cache.decode_attention_calls == 0 and cache.attention_calls == 0

"""CPU-side checks of the wide packed attention (include/retake_hip.h rtk_attention_decode_wide, _wide_fp8kv, _wide_shared:
up to 64 packed rows): the exported symbols, host-side refusals of the entry points, the workspace queries under the
header's plan, and the opt-in switch multi_token_attention="packed".  Nothing here launches a kernel."""
import ctypes
import types

import pytest

P = 0x10000   # a 16-byte aligned non-NULL "pointer": every call below is rejected on the host, before any launch

SYMBOLS = ["rtk_attention_decode_wide", "rtk_attention_decode_wide_workspace_bytes",
           "rtk_attention_decode_wide_fp8kv", "rtk_attention_decode_wide_workspace_bytes_fp8kv",
           "rtk_attention_decode_wide_shared", "rtk_attention_decode_wide_workspace_bytes_shared"]


def _args(nv, q=P, qsh=128, qsl=128, k=P, v=P, ksh=128 * 64, ksl=128, out=P, Hq=28, Hkv=4, Lq=6, Lk=64, off=None, D=128,
          dtype=None, scale=0.1, ws=None, ws_bytes=0):
    dtype = nv.RTK_BF16 if dtype is None else dtype
    off = Lk - Lq if off is None else off
    return (q, qsh, qsl, k, v, ksh, ksl), (out, Hq, Hkv, Lq, Lk, off, D, dtype, scale, ws, ws_bytes, None)


def _wide(nv, name="rtk_attention_decode_wide", **kw):
    head, tail = _args(nv, **kw)
    return getattr(nv.lib, name)(*head, *tail)


def _wide8(nv, L8=128, name="rtk_attention_decode_wide_fp8kv", **kw):
    head, tail = _args(nv, **kw)
    return getattr(nv.lib, name)(*head, P, P, P, P, L8, 128 * L8, L8, *tail)


def _wide_sh(nv, L8=128, Ls=96, name="rtk_attention_decode_wide_shared", **kw):
    head, tail = _args(nv, **kw)
    return getattr(nv.lib, name)(*head, P, P, Ls, 128 * max(Ls, 1), 128, P, P, P, P, L8, 128 * L8, L8, *tail)


def _plan(Hkv, K):
    """The rule of include/retake_hip.h (rtk_attention_decode), restated: (nsplit, keys per split)."""
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    n0 = max(1, min(ceil(512, Hkv), ceil(K, 128)))
    kps = 128 * ceil(ceil(K, n0), 128)
    return ceil(K, kps), kps


def test_library_exports_the_wide_entry_points():
    import retake._native as nv

    raw = ctypes.CDLL(nv.lib._name)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(nv.lib, name).argtypes is not None, name
    assert nv.lib.rtk_version() == 18


@pytest.mark.parametrize("fwd,narrow", [(_wide, "rtk_attention_decode"), (_wide8, "rtk_attention_decode_fp8kv"),
                                        (_wide_sh, "rtk_attention_decode_shared")], ids=["16bit", "fp8kv", "shared"])
def test_wide_argument_validation_without_gpu(fwd, narrow):
    """The cases of test_decode_argument_validation_without_gpu at Lq 6 (42 packed rows: inside the wide envelope only, so
    that each reaches the check it is about): the codes the narrow call returns for them at Lq 2, and the envelope's own."""
    import retake._native as nv

    err = nv.lib.rtk_last_error
    who = (narrow.replace("decode", "decode_wide") + ":").encode()
    for kw, code, word in (({"q": None}, nv.RTK_EINVAL, b"NULL"), ({"out": None}, nv.RTK_EINVAL, b"NULL"),
                           ({"Hkv": 5}, nv.RTK_EINVAL, b"not a multiple of Hkv"),
                           ({"Lq": 65, "Lk": 64}, nv.RTK_EINVAL, b"Lk 64 < Lq 65"),
                           ({"off": 57}, nv.RTK_EINVAL, b"q_offset"), ({"scale": 0.0}, nv.RTK_EINVAL, b"scale"),
                           ({"scale": float("nan")}, nv.RTK_EINVAL, b"scale"),
                           ({"q": P + 2}, nv.RTK_EUNSUPPORTED, b"layout"),
                           ({"Lk": 1024, "ksl": 1 << 20}, nv.RTK_EUNSUPPORTED, b"2 GiB")):
        assert fwd(nv, **kw) == code and word in err() and err().startswith(who), (kw, err())
        # the narrow call, inside ITS envelope, returns the same code for the same mistake
        nkw = dict(kw)
        if "Lq" not in nkw:
            nkw["Lq"] = 2
            if "off" in nkw:
                nkw["off"] = 61
        assert fwd(nv, name=narrow, **nkw) == code and word in err(), (kw, err())
    # outside the envelope: the caller makes the forward call
    assert fwd(nv, Hq=28, Hkv=4, Lq=10) == nv.RTK_EUNSUPPORTED
    assert b"(Hq / Hkv) * Lq = 7 * 10 packed rows (at most 64)" in err() and err().startswith(who)
    assert fwd(nv, Hq=2, Hkv=2, Lq=65, Lk=65, ksh=128 * 65) == nv.RTK_EUNSUPPORTED
    assert b"(Hq / Hkv) * Lq = 1 * 65 packed rows (at most 64)" in err()
    assert fwd(nv, dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and b"dtype" in err() and err().startswith(who)
    assert fwd(nv, D=64) == nv.RTK_EUNSUPPORTED and b"head_dim 64" in err() and err().startswith(who)
    with pytest.raises(NotImplementedError):
        nv.check(fwd(nv, Lq=10), "rtk_attention_decode_wide")
    # the partials always live in the caller's workspace
    assert fwd(nv, Lq=6, Lk=4000, ksh=128 * 4000) == nv.RTK_EWORKSPACE and b"workspace too small" in err()
    assert narrow.replace("rtk_attention_decode", "rtk_attention_decode_wide_workspace_bytes").encode() in err()
    assert fwd(nv, name=narrow, Lq=2, Lk=4000, ksh=128 * 4000) == nv.RTK_EWORKSPACE
    need = 6 * 28 * 130 * 4 * _plan(4, 4000 + (128 if fwd is not _wide else 0) + (96 if fwd is _wide_sh else 0))[0]
    assert fwd(nv, Lq=6, Lk=4000, ksh=128 * 4000, ws=P, ws_bytes=need - 4) == nv.RTK_EWORKSPACE


def test_segment_entry_points_own_checks_and_fall_through():
    import retake._native as nv

    err = nv.lib.rtk_last_error
    assert _wide8(nv, L8=-1) == nv.RTK_EINVAL and b"L8" in err()
    assert _wide_sh(nv, Ls=-1) == nv.RTK_EINVAL and b"Ls" in err()
    head, tail = _args(nv)
    rc = nv.lib.rtk_attention_decode_wide_fp8kv(*head, None, P, P, P, 64, 128 * 64, 64, *tail)
    assert rc == nv.RTK_EINVAL and b"NULL archive pointer" in err()
    rc = nv.lib.rtk_attention_decode_wide_shared(*head, None, P, 96, 128 * 96, 128, P, P, P, P, 64, 128 * 64, 64, *tail)
    assert rc == nv.RTK_EINVAL and b"NULL" in err()
    # Ls == 0 is the _fp8kv call, L8 == 0 as well the plain one: their messages
    assert _wide_sh(nv, Ls=0) == nv.RTK_EWORKSPACE and b"rtk_attention_decode_wide_fp8kv:" in err()
    assert _wide_sh(nv, Ls=0, L8=0) == nv.RTK_EWORKSPACE and b"rtk_attention_decode_wide:" in err()
    assert _wide8(nv, L8=0) == nv.RTK_EWORKSPACE and b"rtk_attention_decode_wide:" in err()
    # at most 16 packed rows is the narrow call of the same segments: its message
    assert _wide(nv, Lq=2) == nv.RTK_EWORKSPACE and b"rtk_attention_decode:" in err()
    assert _wide8(nv, Lq=2) == nv.RTK_EWORKSPACE and b"rtk_attention_decode_fp8kv:" in err()
    assert _wide_sh(nv, Lq=2) == nv.RTK_EWORKSPACE and b"rtk_attention_decode_shared:" in err()


def test_workspace_queries_under_the_headers_plan():
    import retake._native as nv

    L = nv.lib
    wb, wb8, wbs = (L.rtk_attention_decode_wide_workspace_bytes, L.rtk_attention_decode_wide_workspace_bytes_fp8kv,
                    L.rtk_attention_decode_wide_workspace_bytes_shared)
    nb, nb8, nbs = (L.rtk_attention_decode_workspace_bytes, L.rtk_attention_decode_workspace_bytes_fp8kv,
                    L.rtk_attention_decode_workspace_bytes_shared)
    err = L.rtk_last_error
    bf = nv.RTK_BF16
    assert wb(28, 4, 10, 64, 128, bf) == 0 and b"packed rows (at most 64)" in err()
    assert wb(2, 2, 65, 65, 128, bf) == 0 and b"packed rows (at most 64)" in err()
    assert wb8(28, 4, 10, 64, 128, 128, bf) == 0 and b"packed rows (at most 64)" in err()
    assert wbs(28, 4, 10, 64, 128, 96, 128, bf) == 0 and b"packed rows (at most 64)" in err()
    assert wb(28, 4, 6, 64, 128, nv.RTK_F32) == 0 and b"dtype" in err()
    assert wb(28, 4, 6, 64, 64, bf) == 0 and b"head_dim" in err()
    assert wb(28, 5, 6, 64, 128, bf) == 0 and b"not a multiple of Hkv" in err()
    assert wb(28, 4, 65, 64, 128, bf) == 0 and b"Lk 64 < Lq 65" in err()
    assert wb8(28, 4, 6, 64, -1, 128, bf) == 0 and b"L8" in err()
    for Hq, Hkv, Lq in ((28, 4, 3), (28, 4, 6), (28, 4, 9), (32, 4, 8), (8, 8, 17), (2, 2, 64), (16, 1, 4)):
        row = Hq * Lq * 130 * 4
        for Lk in (Lq, 64, 127, 128, 129, 700, 4000, 100352):
            if Lk < Lq:
                continue
            assert wb(Hq, Hkv, Lq, Lk, 128, bf) == _plan(Hkv, Lk)[0] * row == wb(Hq, Hkv, Lq, Lk, 128, nv.RTK_F16), (Hq, Lq, Lk)
        for L8, Ls, Lk in ((640, 0, 70), (624, 96, 64), (59, 45, 70), (100288, 0, 64), (0, 100352, 64), (1, 1, Lq), (0, 0, 700)):
            K8, Ks = -(-L8 // 32) * 32, -(-Ls // 32) * 32
            assert wbs(Hq, Hkv, Lq, Lk, L8, Ls, 128, bf) == _plan(Hkv, Lk + K8 + Ks)[0] * row, (Hq, Lq, L8, Ls, Lk)
            assert wb8(Hq, Hkv, Lq, Lk, L8, 128, bf) == _plan(Hkv, Lk + K8)[0] * row, (Hq, Lq, L8, Lk)
    # at most 16 packed rows: the narrow queries
    for Hq, Hkv, Lq in ((28, 4, 1), (28, 4, 2), (32, 4, 2), (8, 8, 16), (16, 1, 1)):
        for Lk in (64, 700, 100352):
            assert wb(Hq, Hkv, Lq, Lk, 128, bf) == nb(Hq, Hkv, Lq, Lk, 128, bf) > 0
            assert wb8(Hq, Hkv, Lq, Lk, 624, 128, bf) == nb8(Hq, Hkv, Lq, Lk, 624, 128, bf) > 0
            assert wbs(Hq, Hkv, Lq, Lk, 624, 45, 128, bf) == nbs(Hq, Hkv, Lq, Lk, 624, 45, 128, bf) > 0


def _cfg(**top):
    kw = {"kvcache_compression": True,
          "kvcache_compression_kwargs": {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    kw.update(top)
    return types.SimpleNamespace(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=kw)


def test_multi_token_attention_switch():
    import retake.longvideo_cache as lc

    assert lc.build_kvcache(_cfg()).multi_token_attention is None
    assert lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention="packed")).multi_token_attention is None
    cache = lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention="packed", multi_token_attention="packed"))
    assert cache.multi_token_attention == "packed" and cache.decode_attention == "packed" and cache.attention_kernel == "hip"
    assert cache.wide_attention_calls == 0 and cache.decode_attention_calls == 0 and cache.attention_calls == 0
    # needs decode_attention="packed", and through it attention_kernel="hip": the message names both keys
    for top in ({}, {"attention_kernel": "hip"}):
        with pytest.raises(ValueError, match="multi_token_attention") as e:
            lc.build_kvcache(_cfg(multi_token_attention="packed", **top))
        assert "decode_attention" in str(e.value)
    with pytest.raises(ValueError, match="decode_attention"):   # (that key's own refusal comes first)
        lc.build_kvcache(_cfg(decode_attention="packed", multi_token_attention="packed"))
    for bad in ("wide", True, 1):
        with pytest.raises(ValueError) as e:
            lc.build_kvcache(_cfg(attention_kernel="hip", decode_attention="packed", multi_token_attention=bad))
        assert str(e.value) == f"multi_token_attention must be None or 'packed', got {bad!r}"


def test_the_dispatcher_keeps_to_the_geometries_that_measured_faster():
    """multi_token_attention="packed" sends a call to the wide kernel inside its envelope and at 4 <= Hq / Hkv <= 8 only
    (profiles/wide_decode_bench.json: at Hq / Hkv 1, 2 and at Hq 16 / Hkv 1 the chunk-kernel call is not slower)."""
    from retake.native_attention import wide_dispatch

    for Hq, Hkv, Lq, want in ((28, 4, 1, False), (28, 4, 2, False), (28, 4, 3, True), (28, 4, 6, True), (28, 4, 9, True),
                              (28, 4, 10, False), (32, 4, 2, False), (32, 4, 3, True), (32, 4, 8, True), (32, 4, 9, False),
                              (16, 4, 4, False), (16, 4, 5, True), (16, 4, 16, True), (16, 4, 17, False),
                              (8, 4, 9, False), (8, 4, 32, False), (8, 8, 17, False), (2, 2, 64, False), (16, 1, 4, False),
                              (40, 8, 4, True), (24, 4, 3, True)):
        assert wide_dispatch(Hq, Hkv, Lq) is want, (Hq, Hkv, Lq)

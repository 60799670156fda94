"""video_position_limit (the position re-base of a bounded video region; this project's own rule), the parts that need no
GPU: what build_kvcache accepts and refuses, the entry point's place in the ABI, the argument errors
rtk_pivotkv_rebase_batched raises on the host before any launch, and the rule's own restatement (tests/rebase_ref.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import rebase_ref as rr

KEY = "video_position_limit"


def _cfg(top=None, **kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top or {})
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


def test_the_key_is_off_by_default():
    import retake.longvideo_cache as lc

    for top in ({}, {KEY: None}, {"video_window_rows": 48}, {"video_window_rows": 48, KEY: None}):
        cache = lc.build_kvcache(_cfg(top))
        assert cache.video_position_limit is None and cache._position_offsets == {}
        off = cache.position_offset(0)
        assert off.dtype.is_floating_point is False and off.ndim == 0 and int(off) == 0
    for top in ({"video_window_rows": 48}, {"video_budget_rows": 48}):
        for P in (0, 1, 131072):
            cache = lc.build_kvcache(_cfg(dict(top, **{KEY: P})))
            assert cache.video_position_limit == P
            assert int(cache.position_offset(1)) == 0      # before any move: a zero


@pytest.mark.parametrize("top,kw,names", [
    ({KEY: 100}, {}, ("video_window_rows", "video_budget_rows")),
    ({KEY: 100, "video_window_rows": 48}, {"pos_embed_reforge": False}, ("pos_embed_reforge",)),
    ({KEY: 100, "video_budget_rows": 48}, {"pos_embed_reforge": False}, ("pos_embed_reforge",)),
    ({KEY: 100, "video_window_rows": 48, "kv_cache_dtype": "fp8_e4m3"}, {}, ("kv_cache_dtype",)),
    ({KEY: 100, "video_window_rows": 48}, {"native_rope": False}, ("native_rope",)),
    ({KEY: -1, "video_window_rows": 48}, {}, ()),
    ({KEY: 100.0, "video_window_rows": 48}, {}, ()),
    ({KEY: "100", "video_window_rows": 48}, {}, ()),
    ({KEY: True, "video_window_rows": 48}, {}, ()),
    ({KEY: False, "video_budget_rows": 48}, {}, ()),
], ids=["no_bound", "no_reforge_window", "no_reforge_budget", "fp8", "called_rope", "P-1", "Pfloat", "Pstr", "Ptrue", "Pfalse"])
def test_refusals_name_both_keys(top, kw, names):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top, **kw))
    msg = str(ei.value)
    assert KEY in msg
    for name in names:
        assert name in msg, (name, msg)


def test_a_rotary_module_that_has_to_be_called_is_refused_at_the_first_attempt():
    """No inv_freq, or a dynamic / longrope kind: ValueError from the check both policies run in front of their move - before
    anything is launched (no device here: a launch would fail differently)."""
    import retake._video_bound as vb
    import retake.longvideo_cache as lc

    cache = lc.build_kvcache(_cfg({KEY: 0, "video_window_rows": 48}))
    with pytest.raises(ValueError, match=KEY):
        vb._rebase_rotary(cache)                       # no chunk has bound a rotary module yet
    cache._batch = types.SimpleNamespace(rot=None)   # what a batch holds for a module `_rotary` declines
    with pytest.raises(ValueError, match="has to be called"):
        vb._rebase_rotary(cache)

    import torch

    class Dyn:
        inv_freq, attention_scaling, rope_type = torch.ones(4), 1.0, "dynamic"

    class NoInv:
        attention_scaling = 1.0

    assert cache._rotary(Dyn(), torch.device("cpu")) is None and cache._rotary(NoInv(), torch.device("cpu")) is None
    # with the key off the step does nothing at all, whatever the rotary module
    off = lc.build_kvcache(_cfg({"video_window_rows": 48}))
    assert vb.rebase_positions(off, {0: ["never looked at"]}) is None


def test_abi_symbol_struct_and_kernel_ids():
    import retake._native as nv

    assert "rtk_pivotkv_rebase_batched" in nv.EXPORTS and hasattr(nv.lib, "rtk_pivotkv_rebase_batched")
    assert nv.lib.rtk_version() == nv.ABI_VERSION      # an addition: no signature changed
    assert C.sizeof(nv.RebaseUnit) == 64
    assert [f[0] for f in nv.RebaseUnit._fields_] == ["k", "k_stride_h", "first", "rows", "ids", "ids_stride", "end", "H", "slot"]
    ids = nv.profile_kernel_ids()
    assert "rebase_decide" in ids and "rebase_apply" in ids


def test_the_unit_matches_the_header(tmp_path):
    import os
    import subprocess

    import retake._native as nv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rtk_rebase_unit));', '  printf("max %d\\n", RTK_REBASE_MAX_UNITS);']
    lines += [f'  printf("{n} %zu\\n", offsetof(rtk_rebase_unit, {n}));' for n, _ in nv.RebaseUnit._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(nv.RebaseUnit) and int(got["max"]) == nv.REBASE_MAX_UNITS
    for n, _ in nv.RebaseUnit._fields_:
        assert int(got[n]) == getattr(nv.RebaseUnit, n).offset, n


def test_argument_errors_without_a_device():
    """Every error is raised on the host before any launch: no device is touched (the pointers are never dereferenced)."""
    import retake._native as nv

    fake = 0x100000
    sec = (C.c_int * 3)(16, 24, 24)

    def rc(D=128, dtype=nv.RTK_BF16, P=1, inv=fake, nsec=0, limit=0, off=fake, delta=fake, n=1, **kw):
        u = nv.RebaseUnit(fake, 1024 * 128 * 2, 5, 100, fake, 1024, 105, 2, 0)
        for name, value in kw.items():
            setattr(u, name, value)
        return nv.lib.rtk_pivotkv_rebase_batched(C.byref(u), n, D, dtype, P, inv, sec if nsec else None, nsec, limit, off,
                                                 delta, None)

    for kw in ({"k": None}, {"ids": None}, {"inv": None}, {"off": None}, {"delta": None}, {"first": -1}, {"rows": -1},
               {"end": -1}, {"H": 0}, {"H": -2}, {"slot": -1}, {"k_stride_h": -16}, {"ids_stride": -1}, {"limit": -1},
               {"dtype": 2}, {"dtype": 9}, {"P": 2}, {"first": 106}, {"k_stride_h": 104 * 128 * 2},
               {"P": 3, "nsec": 3, "ids_stride": 100}, {"P": 3}, {"D": 0}):
        assert rc(**kw) == nv.RTK_EINVAL, kw
        assert nv.lib.rtk_last_error().startswith(b"rtk_pivotkv_rebase_batched"), kw
    for kw in ({"k": fake + 8}, {"k_stride_h": 1024 * 128 * 2 + 8}, {"D": 72}, {"D": 24}, {"D": 12, "dtype": nv.RTK_F32},
               {"D": 512}, {"ids": fake + 4}):
        assert rc(**kw) == nv.RTK_EUNSUPPORTED, kw
        assert nv.lib.rtk_last_error().startswith(b"rtk_pivotkv_rebase_batched"), kw
    # sections that do not add up to the head_dim
    assert rc(P=3, nsec=3, D=64) == nv.RTK_EINVAL and b"mrope_section" in nv.lib.rtk_last_error()
    # two units with one slot: the decision launch would race on it
    two = (nv.RebaseUnit * 2)(nv.RebaseUnit(fake, 1 << 20, 5, 100, fake, 1024, 105, 2, 3),
                              nv.RebaseUnit(fake, 1 << 20, 5, 100, fake, 1024, 105, 2, 3))
    assert nv.lib.rtk_pivotkv_rebase_batched(two, 2, 128, nv.RTK_BF16, 1, fake, None, 0, 0, fake, fake, None) == nv.RTK_EINVAL
    assert b"slot" in nv.lib.rtk_last_error()
    assert nv.lib.rtk_pivotkv_rebase_batched(None, 1, 128, nv.RTK_BF16, 1, fake, None, 0, 0, fake, fake, None) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_rebase_batched(None, -1, 128, nv.RTK_BF16, 1, fake, None, 0, 0, fake, fake, None) == nv.RTK_EINVAL
    with pytest.raises(NotImplementedError):
        nv.check(rc(D=72), "rtk_pivotkv_rebase_batched")
    # nothing to do: success, nothing launched
    assert nv.lib.rtk_pivotkv_rebase_batched(None, 0, 128, nv.RTK_BF16, 1, fake, None, 0, 0, fake, fake, None) == 0


# ---------------------------------------------------------------------------------------------------
# the rule's restatement
# ---------------------------------------------------------------------------------------------------
def test_the_decision_in_integers():
    t = np.array([0, 1, 2, 3, 4, 50, 51, 60, 61, 61, 99])
    assert rr.decide(t, 5, 11, 99) == 45                 # base = 5: the region follows the pinned rows
    assert rr.decide(t, 5, 11, 100) == 0                 # the last id has not reached the limit
    assert rr.decide(t, 5, 11, 0) == 45
    assert rr.decide(t, 0, 11, 0) == 0                   # nothing pinned and the first id is 0
    assert rr.decide(t + 7, 0, 11, 0) == 7               # ... nothing pinned: base = 0
    assert rr.decide(t, 1, 5, 0) == 0                    # already dense behind the pinned row
    assert rr.decide(t, 5, 5, 0) == 0                    # an empty region
    assert rr.decide(np.array([0, 1, 2, 2, 2, 9]), 3, 6, 0) == 0   # delta = 2 - 3 < 0 (M-RoPE: text ids may overlap): never up
    ids, K, d = rr.rebase(np.stack([t, t + 1000, t + 2000]), np.ones((2, 12, 16)), 5, 11, 11, 99, np.ones(8), [2, 3, 3])
    assert d == 45 and ids[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 15, 16, 16, 54]
    assert np.array_equal(ids[1:], np.stack([t + 1000, t + 2000]))
    assert np.array_equal(K[:, :5], np.ones((2, 5, 16))) and np.array_equal(K[:, 11:], np.ones((2, 1, 16)))
    on = np.concatenate([rr.temporal_pairs(16, 3, [2, 3, 3])] * 2)
    assert on.tolist() == [True, True] + [False] * 6 + [True, True] + [False] * 6
    assert np.array_equal(K[:, 5:11][..., ~on], np.ones((2, 6, 12))) and not np.any(K[:, 5:11][..., on] == 1.0)


@pytest.mark.parametrize("P,sections", [(1, None), (3, [16, 24, 24])])
def test_two_rebases_compose_into_one(P, sections):
    """R(-a) R(-b) = R(-(a + b)) in float64.  With exact angles the two sides agree to float64 roundoff; with the rule's
    fp32 angles each of the three angles is off by at most half an fp32 ulp, 2^-24 |theta| - the difference is bounded by
    that (derived, not measured)."""
    rng = np.random.default_rng(5)
    D = 128
    inv = (10000.0 ** (-np.arange(0, D, 2) / D)).astype(np.float32)
    x = rng.standard_normal((2, 37, D))
    h = D // 2
    mag = np.abs(x[..., :h]) + np.abs(x[..., h:])
    mag = np.concatenate([mag, mag], axis=-1)
    for d1, d2 in ((37, 1000), (1, 1), (624, 131072), (99999, 12345)):
        exact = lambda d: float(d) * inv.astype(np.float64)   # noqa: E731
        two = rr.rotate(rr.rotate(x, d1, inv, P, sections, theta=exact(d1)), d2, inv, P, sections, theta=exact(d2))
        one = rr.rotate(x, d1 + d2, inv, P, sections, theta=exact(d1 + d2))
        assert np.all(np.abs(two - one) <= 1e-9 * mag + 1e-300), (d1, d2)   # (angles of ~1e5 rad: 1e5 * 2^-52 and change)
        two = rr.rotate(rr.rotate(x, d1, inv, P, sections), d2, inv, P, sections)
        one = rr.rotate(x, d1 + d2, inv, P, sections)
        th = np.concatenate([3.0 * 2.0 ** -24 * 1.001 * float(d1 + d2) * inv.astype(np.float64)] * 2)
        assert np.all(np.abs(two - one) <= th * mag + 1e-12 * mag), (d1, d2)
        on = np.concatenate([rr.temporal_pairs(D, P, sections)] * 2)
        assert np.array_equal(one[..., ~on], x[..., ~on])
    assert np.array_equal(rr.rotate(x, 0, inv, P, sections), x)


def test_the_bar_is_the_derived_one():
    assert rr.C == 6.0 * 2.0 ** -24
    assert rr.half_ulp("bfloat16", 1.0) == 2.0 ** -8 and rr.half_ulp("bfloat16", 1.99) == 2.0 ** -8
    assert rr.half_ulp("float16", 0.75) == 2.0 ** -12 and rr.half_ulp("float32", -3.0) == 2.0 ** -23
    assert rr.half_ulp("float16", 1e-9) == 2.0 ** -25    # below the smallest normal: the subnormal spacing
    b = rr.bar("bfloat16", np.array([1.0, 1.0]), np.array([2.0, -3.0]))
    assert np.array_equal(b, np.full(2, 2.0 ** -8 + 6.0 * 2.0 ** -24 * 5.0))

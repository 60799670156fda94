"""Re-scoring and focus over fp8 archive rows (longvideo_kwargs["archive_rescore"]), the parts that need no GPU: what
build_kvcache accepts and refuses, that the key off leaves the two existing refusals as they were, the argument errors
rtk_pivotkv_rescore_fp8k_batched raises on the host before anything is launched, and the entry point's place in the ABI."""
import ctypes as C
import os
import subprocess
import types

import pytest

KEY, RESCORE, FP8 = "archive_rescore", "video_budget_rescore", "kv_cache_dtype"
ENTRY = "rtk_pivotkv_rescore_fp8k_batched"


def _cfg(top=None, **kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top or {})
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


# ---------------------------------------------------------------------------------------------------
# build_kvcache
# ---------------------------------------------------------------------------------------------------
def test_key_on_is_accepted_with_fp8_rows_and_the_budgets_rescoring():
    import retake.longvideo_cache as lc

    cache = lc.build_kvcache(_cfg({KEY: True, FP8: "fp8_e4m3", "video_budget_rows": 48, RESCORE: 0.5}))
    assert cache.archive_rescore is True and cache.video_budget_rescore == 0.5 and cache.kv_cache_dtype == "fp8_e4m3"
    assert cache.memory_footprint()["observe_queries"] == 0
    # without the budget too: `focus` is what the key serves then
    cache = lc.build_kvcache(_cfg({KEY: True, FP8: "fp8_e4m3"}))
    assert cache.archive_rescore is True and cache.video_budget_rescore is None
    # beside the options fp8 rows run beside
    for top, kw in (({"decode_attention": "packed"}, {}), ({}, {"pos_embed_reforge": False}), ({"video_budget_slack": 8}, {})):
        top = dict(top, **{KEY: True, FP8: "fp8_e4m3", "video_budget_rows": 48, RESCORE: 0.25})
        assert lc.build_kvcache(_cfg(top, **kw)).archive_rescore is True
    # a fork does not inherit the key (it needs no GPU to see: the branch is built from the same config)
    assert type(cache)(cache.config).archive_rescore is False


def test_key_off_is_off():
    import retake.longvideo_cache as lc

    for top in ({}, {KEY: None}, {KEY: False}, {KEY: False, FP8: "fp8_e4m3"}, {KEY: None, FP8: "fp8_e4m3"}):
        assert lc.build_kvcache(_cfg(top)).archive_rescore is False


@pytest.mark.parametrize("top,kw,names", [
    ({KEY: 1, FP8: "fp8_e4m3"}, {}, (KEY,)),
    ({KEY: 0, FP8: "fp8_e4m3"}, {}, (KEY,)),
    ({KEY: "yes", FP8: "fp8_e4m3"}, {}, (KEY,)),
    ({KEY: 1.0, FP8: "fp8_e4m3"}, {}, (KEY,)),
    ({KEY: True}, {}, (KEY, FP8)),
    ({KEY: True, "video_budget_rows": 48, RESCORE: 0.5}, {}, (KEY, FP8)),
    # what stays refused under fp8 rows stays refused
    ({KEY: True, FP8: "fp8_e4m3", "video_budget_rows": 48, "video_position_limit": 100}, {}, ("video_position_limit", FP8)),
    ({KEY: True, FP8: "fp8_e4m3"}, {"prompt_guided_scoring": True}, ("prompt_guided_scoring", FP8)),
    ({KEY: True, FP8: "fp8_e4m3"}, {"defer_rerotation": True}, ("defer_rerotation", FP8)),
], ids=["int1", "int0", "str", "float", "no_fp8", "no_fp8_rescore", "position_limit", "prompt_guided", "defer_rerotation"])
def test_refusals_name_their_keys(top, kw, names):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top, **kw))
    for name in names:
        assert name in str(ei.value), (name, str(ei.value))


@pytest.mark.parametrize("off", [{}, {KEY: None}, {KEY: False}], ids=["absent", "none", "false"])
def test_with_the_key_off_the_two_refusals_are_raised_as_before(off):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(dict(off, **{RESCORE: 0.5, "video_budget_rows": 48, FP8: "fp8_e4m3"})))
    assert RESCORE in str(ei.value) and FP8 in str(ei.value) and "e4m3 key rows are not scored again" in str(ei.value)
    # focus: the refusal comes before the cache is looked at (nothing is armed, nothing is on a device)
    cache = lc.build_kvcache(_cfg(dict(off, **{FP8: "fp8_e4m3"})))
    with pytest.raises(ValueError) as ei:
        cache.focus(8)
    assert "PivotKVCache.focus" in str(ei.value) and FP8 in str(ei.value) and "e4m3 key rows are not scored again" in str(ei.value)
    # ... and with the key on the next refusal is the one a 16-bit cache raises: not armed
    cache = lc.build_kvcache(_cfg({KEY: True, FP8: "fp8_e4m3"}))
    with pytest.raises(ValueError, match="not armed"):
        cache.focus(8)


# ---------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------
FAKE = 0x10000   # never dereferenced


def _call(n_units=1, Hq=28, Hkv=4, W=64, D=128, dt=None, alpha=0.5, qsh=64 * 128, qsl=128, scratch=FAKE, stride=1 << 22,
          **fields):
    import retake._native as nv

    u = nv.RescoreFp8kUnit(FAKE, FAKE, 2048 * 128, FAKE, 2048, FAKE, 1000)
    for name, value in fields.items():
        setattr(u, name, value)
    return nv.lib.rtk_pivotkv_rescore_fp8k_batched(C.byref(u), n_units, Hq, Hkv, W, D, nv.RTK_BF16 if dt is None else dt,
                                                   alpha, qsh, qsl, scratch, stride, None)


def test_argument_errors_without_a_device():
    import retake._native as nv

    name = ENTRY.encode()
    need = nv.lib.rtk_pivotkv_rescore_workspace_bytes(28, 4, 64, 1000, 128, nv.RTK_BF16)
    assert need > 0 and need % 256 == 0
    bad = [dict(q=None), dict(k8=None), dict(k_scale=None), dict(score=None), dict(scratch=None), dict(n=-1),
           dict(n=(1 << 24) + 1), dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=float("nan")), dict(W=0),
           dict(W=-3), dict(Hq=30), dict(Hq=0), dict(Hkv=0), dict(D=0),
           dict(qsl=127), dict(qsh=64), dict(k8_stride_h=999 * 128), dict(scale_stride_h=999),   # strides too small
           dict(qsl=132), dict(qsh=64 * 128 + 4), dict(k8_stride_h=2048 * 128 + 8), dict(q=FAKE + 8), dict(k8=FAKE + 8),
           dict(k_scale=FAKE + 2), dict(score=FAKE + 2),                   # 16-byte alignment; scales and scores: 4
           dict(scratch=FAKE + 128), dict(stride=need + 8), dict(stride=need - 256)]   # scratch misaligned / short
    for kw in bad:
        assert _call(**kw) == nv.RTK_EINVAL, kw
        assert nv.lib.rtk_last_error().startswith(name), kw
    assert _call(stride=need, n=1000 + nv.RESCORE_KEYS, k8_stride_h=4096 * 128, scale_stride_h=4096) == nv.RTK_EINVAL
    # no archive exists for fp32 payloads or other head dims, nor for a mode-carrying dtype code
    for kw in (dict(dt=nv.RTK_F32), dict(D=64, qsl=64, qsh=64 * 64), dict(D=256, qsl=256, qsh=64 * 256), dict(dt=nv.RTK_BF16_FAST)):
        assert _call(**kw) == nv.RTK_EUNSUPPORTED, kw
        assert nv.lib.rtk_last_error().startswith(name), kw
    f =nv.lib.rtk_pivotkv_rescore_fp8k_batched
    assert f(None, 1, 28, 4, 64, 128, nv.RTK_BF16, 0.5, 8192, 128, FAKE, need, None) == nv.RTK_EINVAL
    assert f(None, -1, 28, 4, 64, 128, nv.RTK_BF16, 0.5, 8192, 128, FAKE, need, None) == nv.RTK_EINVAL
    # nothing to do: success, nothing launched (the stream is NULL and every pointer fake)
    assert f(None, 0, 28, 4, 64, 128, nv.RTK_BF16, 0.5, 8192, 128, None, 0, None) == 0
    assert _call(n=0) == 0 and _call(n=0, q=None, k8=None, k_scale=None, score=None, stride=0) == 0
    assert _call(n=0, dt=nv.RTK_F16) == 0
    with pytest.raises(ValueError, match=ENTRY):
        nv.check(_call(alpha=2.0), ENTRY)


def test_abi_header_exports_and_library_agree(tmp_path):
    import retake._native as nv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "retake_hip.h")).read()
    assert ENTRY in nv.EXPORTS and hasattr(nv.lib, ENTRY) and f" {ENTRY}(" in header
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18              # an addition: no signature changed
    assert f"Contents ({len(nv.EXPORTS)} entry points" in header
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rtk_rescore_fp8k_unit));']
    lines += [f'  printf("{n} %zu\\n", offsetof(rtk_rescore_fp8k_unit, {n}));' for n, _ in nv.RescoreFp8kUnit._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(nv.RescoreFp8kUnit) == 56
    for n, _ in nv.RescoreFp8kUnit._fields_:
        assert int(got[n]) == getattr(nv.RescoreFp8kUnit, n).offset, n

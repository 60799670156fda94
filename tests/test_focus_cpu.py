"""PivotKVCache.watch_question / focus: the argument checks that need no device, the entry point's host-side refusals
(every one returns before any launch: the pointers are never dereferenced) and the ctypes mirror of rtk_focus_unit."""
import ctypes as C
import os
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cache(**top):
    import retake.longvideo_cache as lc

    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    cfg = types.SimpleNamespace(hidden_size=4 * 128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                longvideo_kwargs=dict({"kvcache_compression": True, "kvcache_compression_kwargs": kw}, **top))
    return lc.build_kvcache(cfg)


@pytest.mark.parametrize("rows", [0, -1, 1.5, "8", None, True, False])
def test_watch_question_refuses_bad_rows(rows):
    cache = _cache()
    with pytest.raises(ValueError, match="rows must be an int >= 1"):
        cache.watch_question(rows)
    assert cache._watch is None


def test_watch_question_needs_video_end():
    cache = _cache()
    assert cache.video_end is None
    for rows in (1, 64):
        with pytest.raises(ValueError, match="video_end"):
            cache.watch_question(rows)
    with pytest.raises(ValueError, match="video_end"):
        cache.watch_question()                       # the default is 64 rows
    assert cache._watch is None and "focus_queries" not in cache.memory_footprint()
    with pytest.raises(ValueError, match="watch_question"):
        cache.watched_queries(0)
    cache.unwatch_question()                         # disarming an unarmed cache is fine


@pytest.mark.parametrize("keep_rows", [0, -3, 2.0, "96", None, True, False])
def test_focus_refuses_bad_keep_rows(keep_rows):
    with pytest.raises(ValueError, match="keep_rows must be an int >= 1"):
        _cache().focus(keep_rows)


def test_focus_refusals_that_need_no_device():
    with pytest.raises(ValueError, match="not armed"):
        _cache().focus(96)
    with pytest.raises(ValueError, match="reserve_tokens"):
        _cache().focus(96, reserve_tokens=True)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        _cache(attention_kernel="hip", kv_cache_dtype="fp8_e4m3").focus(96)
    cache = _cache()
    cache.defer_rerotation = True
    with pytest.raises(NotImplementedError, match="defer_rerotation"):
        cache.focus(96)
    for name in ("focus_scores", "focus_kept"):      # only a focused cache has them
        with pytest.raises(ValueError, match="not a focused cache"):
            getattr(_cache(), name)(0)


def test_entry_point_validates_on_the_host():
    import retake._native as nv

    lib, who = nv.lib, b"rtk_pivotkv_focus_gather_batched"
    assert "rtk_pivotkv_focus_gather_batched" in nv.EXPORTS and lib.rtk_version() == nv.ABI_VERSION   # appended: no bump
    assert lib.rtk_pivotkv_focus_gather_batched(None, 0, None) == 0
    assert lib.rtk_pivotkv_focus_gather_batched(None, 1, None) == nv.RTK_EINVAL and who in lib.rtk_last_error()
    SRC, DST, IDX = 1 << 32, 1 << 33, 1 << 34       # addresses nobody reads

    def call(**change):
        u = nv.FocusUnit(SRC, DST, 4096 * 256, 1024 * 256, 4, 256, 5, 5, 700, 96, 705, 12, IDX)
        for k, v in change.items():
            setattr(u, k, v)
        rc = lib.rtk_pivotkv_focus_gather_batched(C.byref(u), 1, None)
        return rc, lib.rtk_last_error()

    for change, word in ((dict(src=None), b"NULL"), (dict(dst=None), b"NULL"), (dict(idx=None), b"NULL idx"),
                         (dict(head=-1), b"negative"), (dict(tail=-1), b"negative"), (dict(keep=701), b"exceeds"),
                         (dict(streams=0), b"streams"), (dict(row_bytes=0), b"row_bytes"), (dict(row_bytes=10), b"row_bytes"),
                         (dict(src=SRC + 2), b"aligned"), (dict(dst_stride=1024 * 256 + 2), b"aligned"),
                         (dict(src_stride=-4096), b"negative"), (dict(dst_stride=112 * 256), b"dst_stride"),
                         (dict(n=1 << 40), b"int32"), (dict(dst=SRC + 4096), b"overlap"),
                         (dict(src=DST + 1024, src_stride=0), b"overlap")):
        rc, msg = call(**change)
        assert rc == nv.RTK_EINVAL and msg.startswith(who) and word in msg, (change, rc, msg)


def test_the_unit_matches_the_header(tmp_path):
    import retake._native as nv

    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rtk_focus_unit));', '  printf("max %d\\n", RTK_FOCUS_MAX_UNITS);']
    lines += [f'  printf("{f} %zu\\n", offsetof(rtk_focus_unit, {f}));' for f, _ in nv.FocusUnit._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(nv.FocusUnit) and int(got["max"]) == nv.FOCUS_MAX_UNITS
    for f, _ in nv.FocusUnit._fields_:
        assert int(got[f]) == getattr(nv.FocusUnit, f).offset, f

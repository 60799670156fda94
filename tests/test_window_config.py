"""The sliding video window (video_window_rows / video_window_slack), the parts that need no GPU: what build_kvcache
accepts and refuses, the entry point's place in the ABI, and the argument errors rtk_pivotkv_slide_batched raises on the host
before anything is launched."""
import ctypes as C
import types

import pytest


def _cfg(top=None, **kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top or {})
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


def test_defaults_are_off():
    import retake.longvideo_cache as lc

    cache = lc.build_kvcache(_cfg())
    assert cache.video_window_rows is None and cache.video_window_slack == 0 and cache.window_dropped == []
    cache = lc.build_kvcache(_cfg({"video_window_rows": None, "video_window_slack": 0}))
    assert cache.video_window_rows is None
    cache = lc.build_kvcache(_cfg({"video_window_rows": 100352, "video_window_slack": 1568}))
    assert (cache.video_window_rows, cache.video_window_slack) == (100352, 1568)
    assert lc.build_kvcache(_cfg({"video_window_rows": 48})).video_window_slack == 0
    # every other option keeps working beside it
    for top, kw in (({"kv_cache_dtype": "fp8_e4m3"}, {}), ({"decode_attention": "packed"}, {}), ({}, {"score_rounding": "fast"}),
                    ({}, {"overlap_streams": 2}), ({}, {"flush_every_layers": 1}), ({}, {"pos_embed_reforge": False})):
        top = dict(top, video_window_rows=48, video_window_slack=32)
        assert lc.build_kvcache(_cfg(top, **kw)).video_window_rows == 48


@pytest.mark.parametrize("top,kw", [
    ({"video_window_rows": 48}, {"defer_rerotation": True}),
    ({"video_window_rows": 48}, {"prompt_guided_scoring": True}),
    ({"video_window_rows": 0}, {}),
    ({"video_window_rows": -5}, {}),
    ({"video_window_rows": 48.0}, {}),
    ({"video_window_rows": "48"}, {}),
    ({"video_window_rows": True}, {}),
    ({"video_window_rows": 48, "video_window_slack": -1}, {}),
    ({"video_window_rows": 48, "video_window_slack": 1.5}, {}),
    ({"video_window_slack": -1}, {}),
], ids=["defer_rerotation", "prompt_guided_scoring", "W0", "W-5", "Wfloat", "Wstr", "Wbool", "S-1", "Sfloat", "S-1_alone"])
def test_refusals_name_both_keys(top, kw):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top, **kw))
    msg = str(ei.value)
    assert "video_window_rows" in msg and "video_window_slack" in msg
    for name in kw:
        assert name in msg


def test_abi_symbol_struct_and_kernel_id():
    import retake._native as nv

    assert "rtk_pivotkv_slide_batched" in nv.EXPORTS and hasattr(nv.lib, "rtk_pivotkv_slide_batched")
    # rtk_version still answers what the binding expects: this entry point is an addition, no signature changed, and
    # the number itself is pinned by earlier tests
    assert nv.lib.rtk_version() == nv.ABI_VERSION
    assert C.sizeof(nv.SlideUnit) == 48
    assert [f[0] for f in nv.SlideUnit._fields_] == ["base", "stream_stride", "streams", "row_bytes", "first", "drop", "rows"]
    assert nv.SlideUnit.first.offset == 24 and nv.SlideUnit.row_bytes.offset == 20
    assert "slide_units" in nv.profile_kernel_ids()


def test_argument_errors_without_a_device():
    """Every error is raised on the host before any launch, and so are the cases that launch nothing: no device is touched."""
    import retake._native as nv

    fake = 0x10000   # never dereferenced

    def rc(n=1, **kw):
        u = nv.SlideUnit(fake, 4096, 2, 256, 5, 7, 100)
        for name, value in kw.items():
            setattr(u, name, value)
        return nv.lib.rtk_pivotkv_slide_batched(C.byref(u), n, None)

    for kw in ({"base": None}, {"first": -1}, {"drop": -1}, {"rows": -1}, {"streams": 0}, {"streams": -2}, {"row_bytes": 0},
               {"row_bytes": -4}, {"row_bytes": 6}, {"base": fake + 2}, {"stream_stride": 4098}):
        assert rc(**kw) == nv.RTK_EINVAL, kw
        assert nv.lib.rtk_last_error().startswith(b"rtk_pivotkv_slide_batched"), kw
    assert nv.lib.rtk_pivotkv_slide_batched(None, 1, None) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_slide_batched(None, -1, None) == nv.RTK_EINVAL
    with pytest.raises(ValueError):
        nv.check(rc(first=-1), "rtk_pivotkv_slide_batched")
    # nothing to move: success, nothing launched
    assert nv.lib.rtk_pivotkv_slide_batched(None, 0, None) == 0
    assert rc(drop=0) == 0 and rc(rows=0) == 0

"""The video budget (video_budget_rows / video_budget_slack), the parts that need no GPU: what build_kvcache accepts and
refuses, the three entry points' place in the ABI, the argument errors they raise on the host before anything is launched,
and the rule's CPU restatement (tests/budget_ref.py) against hand-worked cases."""
import ctypes as C
import os
import types

import pytest
import torch

import budget_ref as br

ENTRY_POINTS = ("rtk_pivotkv_keep_scores_batched", "rtk_pivotkv_budget_select_batched", "rtk_pivotkv_squeeze_batched")


def _cfg(top=None, **kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top or {})
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


def test_defaults_are_off():
    import retake.longvideo_cache as lc

    for top in ({}, {"video_budget_rows": None, "video_budget_slack": 0}):
        cache = lc.build_kvcache(_cfg(top))
        assert cache.video_budget_rows is None and cache.video_budget_slack == 0 and cache.budget_dropped == []
        assert cache.score_when_keeping_all is False
        assert "row_scores" not in cache.memory_footprint()          # no new footprint key
        cache._store(0)
        assert cache._layers[0].sc is None and cache._layers[0].sc_len == 0   # no score buffer
        with pytest.raises(ValueError, match="video_budget_rows"):
            cache.row_scores(0)
    cache = lc.build_kvcache(_cfg({"video_budget_rows": 100352, "video_budget_slack": 1568}))
    assert (cache.video_budget_rows, cache.video_budget_slack) == (100352, 1568)
    assert cache.score_when_keeping_all is True                      # a chunk that keeps all of its rows is still scored
    assert cache.memory_footprint()["row_scores"] == 0 and cache.memory_footprint()["total"] == 0
    assert cache.row_scores(0).numel() == 0
    assert lc.build_kvcache(_cfg({"video_budget_rows": 48})).video_budget_slack == 0
    # every other option the window runs beside keeps working beside it
    for top, kw in (({"kv_cache_dtype": "fp8_e4m3"}, {}), ({"decode_attention": "packed"}, {}), ({}, {"score_rounding": "fast"}),
                    ({}, {"score_rounding": "reference"}), ({}, {"overlap_streams": 2}), ({}, {"flush_every_layers": 1}),
                    ({}, {"pos_embed_reforge": False})):
        top = dict(top, video_budget_rows=48, video_budget_slack=32)
        assert lc.build_kvcache(_cfg(top, **kw)).video_budget_rows == 48


@pytest.mark.parametrize("top,kw,also", [
    ({"video_budget_rows": 48, "video_window_rows": 48}, {}, "video_window_rows"),
    ({"video_budget_rows": 48}, {"defer_rerotation": True}, "defer_rerotation"),
    ({"video_budget_rows": 48}, {"prompt_guided_scoring": True}, "prompt_guided_scoring"),
    ({"video_budget_rows": 0}, {}, None),
    ({"video_budget_rows": -5}, {}, None),
    ({"video_budget_rows": 48.0}, {}, None),
    ({"video_budget_rows": "48"}, {}, None),
    ({"video_budget_rows": True}, {}, None),
    ({"video_budget_rows": 48, "video_budget_slack": -1}, {}, None),
    ({"video_budget_rows": 48, "video_budget_slack": 1.5}, {}, None),
    ({"video_budget_rows": 48, "video_budget_slack": False}, {}, None),
    ({"video_budget_slack": -1}, {}, None),
], ids=["window", "defer_rerotation", "prompt_guided_scoring", "B0", "B-5", "Bfloat", "Bstr", "Bbool", "S-1", "Sfloat", "Sbool",
        "S-1_alone"])
def test_refusals_name_both_keys(top, kw, also):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top, **kw))
    msg = str(ei.value)
    assert "video_budget_rows" in msg and "video_budget_slack" in msg
    if also:
        assert also in msg


def test_abi_symbols_structs_and_kernel_ids():
    import retake._native as nv

    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "retake_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in nv.EXPORTS and hasattr(nv.lib, name)
        assert f"int {name}(" in header
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18              # additions only: no signature changed
    assert [f[0] for f in nv.SqueezeUnit._fields_] == ["base", "stream_stride", "streams", "row_bytes", "first", "rows_out",
                                                       "rows_in", "idx"]
    assert C.sizeof(nv.SqueezeUnit) == 56 and nv.SqueezeUnit.first.offset == 24 and nv.SqueezeUnit.idx.offset == 48
    assert C.sizeof(nv.BudgetSelectUnit) == 24 and C.sizeof(nv.KeepScoresUnit) == 32
    assert f"#define RTK_SQUEEZE_MAX_UNITS {nv.SQUEEZE_MAX_UNITS}" in header
    assert {"keep_scores", "budget_select", "squeeze_units"} <= set(nv.profile_kernel_ids())


def _errors(fn_name, make, bad, noop=()):
    """Every `bad` field setting makes the call return RTK_EINVAL with the entry point's name in rtk_last_error - on a NULL
    stream and fake pointers, so nothing can have been launched."""
    import retake._native as nv

    fn = getattr(nv.lib, fn_name)

    def rc(**kw):
        u = make()
        for name, value in kw.items():
            setattr(u, name, value)
        return fn(C.byref(u), 1, None)

    for kw in bad:
        assert rc(**kw) == nv.RTK_EINVAL, (fn_name, kw)
        assert nv.lib.rtk_last_error().startswith(fn_name.encode()), (fn_name, kw)
    assert fn(None, 1, None) == nv.RTK_EINVAL and nv.lib.rtk_last_error().startswith(fn_name.encode())
    assert fn(None, -1, None) == nv.RTK_EINVAL and nv.lib.rtk_last_error().startswith(fn_name.encode())
    assert fn(None, 0, None) == 0                                    # n_units == 0: success, nothing launched
    for kw in noop:
        assert rc(**kw) == 0, (fn_name, kw)
    with pytest.raises(ValueError, match=fn_name):
        nv.check(rc(**bad[0]), fn_name)


def test_argument_errors_without_a_device():
    import retake._native as nv

    fake = 0x10000   # never dereferenced
    _errors("rtk_pivotkv_squeeze_batched", lambda: nv.SqueezeUnit(fake, 4096, 2, 256, 5, 7, 9, fake),
            [{"base": None}, {"idx": None}, {"first": -1}, {"rows_out": -1}, {"rows_in": -1}, {"rows_out": 10},
             {"rows_in": 1 << 31, "rows_out": 0}, {"streams": 0}, {"streams": -2}, {"row_bytes": 0}, {"row_bytes": -4},
             {"row_bytes": 6}, {"base": fake + 2}, {"stream_stride": 4098}],
            noop=[{"rows_out": 0}, {"rows_out": 0, "idx": None}])
    _errors("rtk_pivotkv_budget_select_batched", lambda: nv.BudgetSelectUnit(fake, fake, 10, 4),
            [{"score": None}, {"idx": None}, {"n": 0}, {"n": -3}, {"keep": 0}, {"keep": -1}, {"keep": 11}])
    _errors("rtk_pivotkv_keep_scores_batched", lambda: nv.KeepScoresUnit(fake, fake, fake, 8),
            [{"score": None}, {"dst": None}, {"keep": -1}], noop=[{"keep": 0}, {"keep": 0, "score": None, "dst": None}])


def test_rule_against_hand_worked_cases():
    t = torch.tensor
    # distinct scores: the newest row (score 0.1, the minimum) survives, then the two best of the rest, in sequence order
    assert br.survivors(t([0.5, 0.9, 0.2, 0.7, 0.1]), 3).tolist() == [1, 3, 4]
    # ties go to the lowest index: of the three rows at 1.0 the first two survive with the newest
    assert br.survivors(t([1.0, 0.3, 1.0, 1.0, 0.2]), 3).tolist() == [0, 2, 4]
    # a tie at the threshold below a clear winner
    assert br.survivors(t([0.4, 2.0, 0.4, 0.4, 9.0]), 3).tolist() == [0, 1, 4]
    # the newest row does not compete: a top score there does not cost the others a place
    assert br.survivors(t([0.1, 0.2, 0.3, 5.0]), 3).tolist() == [1, 2, 3]
    assert br.survivors(t([0.7, 0.7, 0.7, 0.7]), 1).tolist() == [3]
    assert br.survivors(t([0.7, 0.1, 0.9]), 3).tolist() == [0, 1, 2]
    assert br.survivors(t([3.0]), 1).tolist() == [0]
    # slack: nothing happens up to B + S rows, and an eviction goes all the way down to B
    s = t([0.5, 0.9, 0.2, 0.7, 0.1])
    assert br.evict(s, 3, 2) is None and br.evict(s, 5, 0) is None
    assert br.evict(s, 3, 1).tolist() == [1, 3, 4] and br.evict(s, 4, 0).tolist() == [0, 1, 3, 4]
    # three chunks of two rows, B = 3: S = 0 evicts after chunks 2 and 3, S = 2 only after chunk 3
    chunks = [t([0.5, 0.9]), t([0.2, 0.7]), t([0.8, 0.1])]
    out = br.simulate(chunks, 3, 0)
    assert [(a.tolist(), d, e) for a, d, e in out] == [([0, 1], 0, 0), ([0, 1, 3], 1, 1), ([1, 4, 5], 3, 2)]
    out = br.simulate(chunks, 3, 2)
    assert [(a.tolist(), d, e) for a, d, e in out] == [([0, 1], 0, 0), ([0, 1, 2, 3], 0, 0), ([1, 4, 5], 3, 1)]

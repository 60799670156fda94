"""The host-side refusals around the bounded video region (include/retake_hip.h "Sliding window", "Video budget"): one call per
row of ROWS to rtk_pivotkv_slide_batched, rtk_pivotkv_keep_scores_batched, rtk_pivotkv_budget_select_batched or
rtk_pivotkv_squeeze_batched, its return code and the whole rtk_last_error() text, and one build_kvcache call per row of
CONFIGS, its whole ValueError text, compared with tests/golden/region_refusals.json.  The file pins the order of the checks,
the codes and the wording - what a caller's logs and `nv.check` show - across rewrites of the code around the kernels.
Nothing here launches a kernel: every row is refused before any launch or holds only units with nothing to do (checked
here, before the call), on a NULL stream with pointers that are never dereferenced.

    python tests/test_region_refusals_cpu.py --record     rewrites the golden file from the package as built
"""
import ctypes as C
import json
import os
import sys
import types

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region_refusals.json")
P = 0x10000   # a 16-byte aligned non-NULL "pointer"
SLIDE, KEEP, SELECT, SQUEEZE = ("rtk_pivotkv_slide_batched", "rtk_pivotkv_keep_scores_batched",
                                "rtk_pivotkv_budget_select_batched", "rtk_pivotkv_squeeze_batched")
# every row starts from this error text (no row's own), so a call that sets none - the no-ops - is recorded as such
SENTINEL = "rtk_attention_workspace_bytes: unsupported head_dim 4 (a multiple of 8 up to 256)"
BIG = 1 << 54   # rows whose byte offset at 256 bytes a row overflows int64 / 4


def _reset(nv):
    assert nv.lib.rtk_attention_workspace_bytes(1, 1, 1, 1, 4, nv.RTK_F32) == 0 and nv.lib.rtk_last_error().decode() == SENTINEL


def _unit_types(nv):
    """entry point -> (unit type, a unit that passes every check, the test that a unit launches nothing)"""
    return {SLIDE: (nv.SlideUnit, (P, 4096, 2, 256, 5, 7, 100), lambda u: u.drop == 0 or u.rows == 0),
            KEEP: (nv.KeepScoresUnit, (P, P, P, 8), lambda u: u.keep == 0),
            SELECT: (nv.BudgetSelectUnit, (P, P, 10, 4), lambda u: False),
            SQUEEZE: (nv.SqueezeUnit, (P, 4096, 2, 256, 5, 7, 9, P), lambda u: u.rows_out == 0)}


def _call(nv, fn, spec):
    """spec: `units` - one dict of field overrides per unit (default: one unit, no override); `n` - n_units if not their count;
    `null` - pass NULL for the array; `noop` - the call is expected to succeed, so every unit must be one that launches nothing"""
    unknown = set(spec) - {"units", "n", "null", "noop"}
    assert not unknown, (fn, unknown)
    cls, ok, idle = _unit_types(nv)[fn]
    overs = spec.get("units", [{}])
    arr = (cls * max(1, len(overs)))()
    for u, over in zip(arr, overs):
        cls.__init__(u, *ok)
        for name, value in over.items():
            assert name in [f[0] for f in cls._fields_], (fn, name)
            setattr(u, name, value)
    n = spec.get("n", len(overs))
    if spec.get("noop"):   # nothing may get as far as a launch
        assert n <= 0 or (not spec.get("null") and n <= len(overs) and all(idle(u) for u in arr[:n])), (fn, spec)
    return getattr(nv.lib, fn)(None if spec.get("null") else arr, n, None)


def _one(**over):
    return dict(units=[over])


def _rows():
    rows = []
    prologue = [("n_units_negative", dict(n=-1)), ("n_units_negative_before_null", dict(n=-1, null=True)),
                ("null_units", dict(null=True)), ("null_units_two", dict(null=True, n=2)),
                ("no_units_null", dict(null=True, n=0, noop=True)), ("no_units", dict(n=0, noop=True))]
    # the fields rtk_slide_unit and rtk_squeeze_unit share
    streams = [("null_base", _one(base=None)), ("first_negative", _one(first=-1)), ("streams_zero", _one(streams=0)),
               ("streams_negative", _one(streams=-2)), ("row_bytes_zero", _one(row_bytes=0)), ("row_bytes_negative", _one(row_bytes=-4)),
               ("row_bytes_odd", _one(row_bytes=6)), ("base_misaligned", _one(base=P + 2)), ("stride_misaligned", _one(stream_stride=4098)),
               ("base_and_stride_misaligned", _one(base=P + 1, stream_stride=-4098)),
               ("null_base_before_streams", _one(base=None, streams=0)), ("first_negative_before_row_bytes", _one(first=-1, row_bytes=6)),
               ("streams_before_row_bytes", _one(streams=0, row_bytes=0)), ("row_bytes_before_alignment", _one(row_bytes=6, base=P + 2)),
               ("alignment_before_overflow", _one(stream_stride=4098, first=BIG)), ("first_overflows", _one(first=BIG)),
               ("first_at_the_bound_row_bytes_4", _one(row_bytes=4, first=(1 << 59) + 1)),
               ("second_unit", dict(units=[{}, dict(streams=0)])), ("third_unit_first_fault_wins", dict(units=[{}, {}, dict(row_bytes=6), dict(base=None)])),
               ("first_unit_before_second", dict(units=[dict(base=P + 2), dict(base=None)]))]
    r = prologue + streams + [
        ("drop_negative", _one(drop=-1)), ("rows_negative", _one(rows=-1)), ("negative_before_streams", _one(drop=-1, streams=0)),
        ("drop_overflows", _one(drop=BIG)), ("rows_overflows", _one(rows=BIG)), ("overflow_before_workgroups", _one(first=BIG, drop=1 << 33, rows=1 << 33)),
        ("too_many_workgroups", _one(drop=1 << 33, rows=1 << 33)), ("too_many_workgroups_streams", _one(streams=0x40000000)),
        ("idle_unit_is_checked", _one(drop=0, streams=0)), ("idle_unit_is_checked_overflow", _one(rows=0, drop=BIG)),
        ("drop_zero", dict(units=[dict(drop=0)], noop=True)), ("rows_zero", dict(units=[dict(rows=0)], noop=True)),
        ("all_idle", dict(units=[dict(drop=0), dict(rows=0), dict(drop=0, rows=0)], noop=True)),
        ("idle_then_fault", dict(units=[dict(drop=0), dict(rows=-1)]))]
    rows += [(f"{SLIDE}/{name}", SLIDE, spec) for name, spec in r]
    r = prologue + streams + [
        ("null_idx", _one(idx=None)), ("rows_out_negative", _one(rows_out=-1)), ("rows_in_negative", _one(rows_in=-1)),
        ("rows_out_exceeds_rows_in", _one(rows_out=10)), ("rows_out_exceeds_before_int32", _one(rows_out=1 << 32, rows_in=1 << 31)),
        ("rows_in_int32", _one(rows_in=1 << 31, rows_out=0)), ("rows_in_int32_bound", _one(rows_in=0x7fff0001)),
        ("rows_in_int32_before_idx", _one(rows_in=0x7fff0001, idx=None)), ("negative_before_null_idx", _one(rows_in=-1, idx=None)),
        ("null_base_before_null_idx", _one(base=None, idx=None)), ("null_idx_before_streams", _one(idx=None, streams=0)),
        ("too_many_workgroups", _one(row_bytes=0x7ffffffc, streams=128)), ("overflow_before_workgroups", _one(row_bytes=0x7ffffffc, streams=128, first=1 << 31)),
        ("idle_unit_is_checked", _one(rows_out=0, streams=0)),
        ("rows_out_zero", dict(units=[dict(rows_out=0)], noop=True)), ("rows_out_zero_null_idx", dict(units=[dict(rows_out=0, idx=None)], noop=True)),
        ("rows_in_at_the_bound", dict(units=[dict(rows_out=0, rows_in=0x7fff0000)], noop=True)),
        ("all_idle", dict(units=[dict(rows_out=0), dict(rows_out=0, rows_in=0)], noop=True)),
        ("idle_then_fault", dict(units=[dict(rows_out=0), dict(rows_out=10)]))]
    rows += [(f"{SQUEEZE}/{name}", SQUEEZE, spec) for name, spec in r]
    r = prologue + [
        ("null_score", _one(score=None)), ("null_idx", _one(idx=None)), ("n_zero", _one(n=0)), ("n_negative", _one(n=-3)),
        ("keep_zero", _one(keep=0)), ("keep_negative", _one(keep=-1)), ("keep_exceeds_n", _one(keep=11)),
        ("null_before_n", _one(score=None, n=0)), ("n_before_keep", _one(n=0, keep=0)),
        ("second_unit", dict(units=[{}, dict(keep=11)])), ("first_unit_before_second", dict(units=[dict(n=0), dict(idx=None)]))]
    rows += [(f"{SELECT}/{name}", SELECT, spec) for name, spec in r]
    r = prologue + [
        ("null_score", _one(score=None)), ("null_dst", _one(dst=None)), ("keep_negative", _one(keep=-1)),
        ("keep_before_null", _one(keep=-1, score=None)), ("second_unit", dict(units=[{}, dict(dst=None)])),
        ("idle_then_fault", dict(units=[dict(keep=0), dict(keep=-1)])),
        ("keep_zero", dict(units=[dict(keep=0)], noop=True)),
        ("keep_zero_null_pointers", dict(units=[dict(keep=0, score=None, dst=None, keep_idx=None)], noop=True)),
        ("all_idle", dict(units=[dict(keep=0), dict(keep=0, score=None)], noop=True))]
    rows += [(f"{KEEP}/{name}", KEEP, spec) for name, spec in r]
    return rows


def _configs():
    """(id, top-level keys, kvcache_compression_kwargs): every refusing config of tests/test_window_config.py and
    tests/test_budget_config.py, and configs with two faults for the order"""
    out = []
    for word, key, slack in (("window", "video_window_rows", "video_window_slack"), ("budget", "video_budget_rows", "video_budget_slack")):
        c = [("defer_rerotation", {key: 48}, {"defer_rerotation": True}), ("prompt_guided_scoring", {key: 48}, {"prompt_guided_scoring": True}),
             ("rows_0", {key: 0}, {}), ("rows_-5", {key: -5}, {}), ("rows_float", {key: 48.0}, {}), ("rows_str", {key: "48"}, {}),
             ("rows_bool", {key: True}, {}), ("slack_-1", {key: 48, slack: -1}, {}), ("slack_float", {key: 48, slack: 1.5}, {}),
             ("slack_bool", {key: 48, slack: False}, {}), ("slack_none", {key: 48, slack: None}, {}), ("slack_-1_alone", {slack: -1}, {}),
             ("rows_and_slack", {key: 0, slack: "x"}, {}),
             ("values_before_defer_rerotation", {key: 0}, {"defer_rerotation": True}),
             ("defer_rerotation_before_prompt_guided_scoring", {key: 48}, {"defer_rerotation": True, "prompt_guided_scoring": True}),
             ("fp8_defer_rerotation_first", {key: 48, "kv_cache_dtype": "fp8_e4m3"}, {"defer_rerotation": True})]
        out += [(f"build_kvcache/{word}/{name}", top, kw) for name, top, kw in c]
    both = [("budget_with_window", {"video_budget_rows": 48, "video_window_rows": 48}, {}),
            ("window_values_before_budget_values", {"video_budget_rows": 0, "video_window_rows": 0}, {}),
            ("window_defer_rerotation_before_budget", {"video_budget_rows": 48, "video_window_rows": 48}, {"defer_rerotation": True}),
            ("budget_values_before_window_with_budget", {"video_budget_rows": -1, "video_window_rows": 48}, {}),
            ("budget_with_window_before_defer_rerotation", {"video_budget_rows": 48, "video_window_rows": 48, "video_window_slack": 3},
             {"prompt_guided_scoring": False}),
            ("off_window_does_not_refuse_the_budget", {"video_budget_rows": 48, "video_window_rows": None}, {"prompt_guided_scoring": True})]
    return out + [(f"build_kvcache/both/{name}", top, kw) for name, top, kw in both]


ROWS, CONFIGS = _rows(), _configs()


def _cfg(top, kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top)
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


def _refusals(nv, lc):
    got = {}
    for rid, fn, spec in ROWS:
        _reset(nv)
        rc = _call(nv, fn, spec)
        got[rid] = [rc, nv.lib.rtk_last_error().decode()]
    for rid, top, kw in CONFIGS:
        try:
            lc.build_kvcache(_cfg(top, kw))
            got[rid] = [0, ""]
        except ValueError as e:
            got[rid] = [nv.RTK_EINVAL, str(e)]
    return got


def _check_kinds(nv, got):
    """a refusal: RTK_EINVAL and a text of its own, never RTK_EHIP - nothing reached the device; a no-op: 0 and no text"""
    for rid, fn, spec in ROWS:
        rc, text = got[rid]
        if spec.get("noop"):
            assert (rc, text) == (0, SENTINEL), rid
        else:
            assert rc == nv.RTK_EINVAL and text.startswith(fn + ": "), (rid, rc, text)
    for rid, _, _ in CONFIGS:
        assert got[rid][0] == nv.RTK_EINVAL and got[rid][1], rid


def test_every_refusal_returns_the_recorded_code_and_text():
    import retake._native as nv
    import retake.longvideo_cache as lc

    ids = [r[0] for r in ROWS + CONFIGS]
    assert len(set(ids)) == len(ids) and {fn for _, fn, _ in ROWS} == {SLIDE, KEEP, SELECT, SQUEEZE}
    want = json.load(open(GOLDEN))
    got = _refusals(nv, lc)
    assert sorted(got) == sorted(want)
    for rid in ids:
        assert got[rid] == want[rid], rid
    _check_kinds(nv, got)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-retake_amd"))
    import retake._native as nv_
    import retake.longvideo_cache as lc_

    got_ = _refusals(nv_, lc_)
    _check_kinds(nv_, got_)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(rid)}: {json.dumps(v)}" for rid, v in sorted(got_.items())) + "\n}\n")
    print("recorded", len(got_), "refusals in", GOLDEN)

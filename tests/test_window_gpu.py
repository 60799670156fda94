"""The sliding video window of PivotKVCache (video_window_rows / video_window_slack) on the GPU.  Every case is a TWIN
comparison, bit for bit: the same inputs go to a cache with the window and to one without, and after every after_forward
the windowed cache's rows must be the unbounded twin's pinned rows followed by its LAST n rows (n = the windowed region):
scoring, selection and the reforged ids depend only on the chunk and on the last stored temporal id, and a slide changes
neither.  The counters are checked against the rule itself, restated here in a few lines (`_rule`).

Shapes: 2 layers, Hq 4, Hkv 2, D 128 (the driver and helpers of tests/test_rewind_gpu.py), 5 text rows, then 5 chunks of
L = 64 (selection inside update) or L = 512 (the batched flush), compression ratio 0.5, W = 1.5 x keep - a slide cuts
inside a chunk - with slack 0 and slack = keep."""
import pytest
import torch

import attention_ref as ar
import synth
from test_rewind_gpu import SEC, A, D, LAYERS, TEXT, _cfg, _Driver, _qkv, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

RATIO, CHUNKS, QUESTION = 0.5, 5, 7


class _WindowDriver(_Driver):
    """test_rewind_gpu's driver (its calls, its ids, its log) at ratio 0.5 around ONE cache, built here from one config that
    carries the two window keys - top-level keys of longvideo_kwargs, which that driver's own constructor cannot pass."""

    def __init__(self, protocol, ids, dtype, L, W=None, S=0, reserve=None, reforge=True, fp8=False, **extra):
        import retake.longvideo_cache as lc

        cfg = _cfg(reforge, fp8, compression_ratio=RATIO, **extra)
        if W is not None:   # ("off": the keys spelled out with their defaults)
            cfg.longvideo_kwargs.update(video_window_rows=None if W == "off" else W, video_window_slack=S)
        self.cache = lc.build_kvcache(cfg, **({"reserve_tokens": reserve} if reserve else {}))
        self.protocol, self.mrope, self.dtype, self.L, self.prompt = protocol, ids == "mrope", dtype, L, 0
        self.sec = SEC if self.mrope else None
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.t_next = 0
        self.log = []


_driver = _WindowDriver


def _rule(chunks, keep, W, S):
    """The window rule on one layer: (region, rows dropped so far, slides so far) after each chunk."""
    region = dropped = slides = 0
    out = []
    for _ in range(chunks):
        region += keep
        if region > W + S:
            dropped += region - W
            slides += 1
            region = W
        out.append((region, dropped, slides))
    return out


def _windowed(t, n, dim=2):
    """[pinned rows | last n rows] of the unbounded twin's tensor."""
    return torch.cat([t.narrow(dim, 0, TEXT), t.narrow(dim, t.shape[dim] - n, n)], dim=dim)


def _check_twin(w, u, n, what):
    """The windowed cache against the unbounded one, every layer: K, V, ids."""
    pw, pu = w.cache.position_cache, u.cache.position_cache
    assert len(pw) == len(pu), what                      # (no reforging: no ids are kept, by either)
    for l in range(LAYERS):
        assert w.cache.get_seq_length(l) == TEXT + n, (what, l)
        _same(w.cache.key_cache[l], _windowed(u.cache.key_cache[l], n), (what, "K", l))
        _same(w.cache.value_cache[l], _windowed(u.cache.value_cache[l], n), (what, "V", l))
        if l < len(pu) and isinstance(pu[l], torch.Tensor):
            _same(pw[l], _windowed(pu[l], n, pu[l].ndim - 1), (what, "ids", l))
        assert int(w.cache.get_prev_temporal_idx(l)) == int(u.cache.get_prev_temporal_idx(l)), (what, l)


def _check_counters(cache, c, L, keep, region, dropped, what):
    assert cache.num_evicted_tokens == [(c + 1) * (L - keep) + dropped] * LAYERS, what
    assert (cache.window_dropped or [0] * LAYERS) == [dropped] * LAYERS, what
    assert [cache.get_seq_length(l) for l in range(LAYERS)] == [TEXT + region] * LAYERS, what


def _run_twins(protocol, ids, dtype, L, S, chunks=CHUNKS, **kw):
    keep = int(RATIO * L)
    W = keep + keep // 2
    w = _driver(protocol, ids, dtype, L, W=W, S=S, **kw)
    u = _driver(protocol, ids, dtype, L, **kw)
    for d in (w, u):
        d.step(1, TEXT)
    epoch = w.cache._epoch
    for c, (region, dropped, slides) in enumerate(_rule(chunks, keep, W, S)):
        for d in (w, u):
            d.step(2 + c, L, video=True)
        what = (protocol, ids, dtype, L, S, "chunk", c)
        assert region <= W + S
        _check_twin(w, u, region, what)
        _check_counters(w.cache, c, L, keep, region, dropped, what)
        assert w.cache._epoch == epoch + slides, what           # a slide, and nothing else here, moves the epoch
        assert w.cache.video_end is not None and w.cache.video_end.epoch == w.cache._epoch
    assert slides >= 1 and u.cache.get_seq_length(0) == TEXT + chunks * keep
    return w, u, keep, W


def _attention_within_bars(log, dtype):
    """The chunk's attention outputs the driver logged (cache.attention on the views update returned) against float64 on
    those views - the windowed cache's dense rows - with the bar of tests/test_attention_gpu.py: max(2 E, half an ulp of the
    output dtype at the output's magnitude), E the reference's eager expression's error on the same inputs."""
    assert len(log) == LAYERS
    for l, (q, k, v, out) in enumerate(log):
        ref = ar.attention_fp64(q, k, v)
        err = (out.double() - ref).abs().max().item()
        e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(dtype, ref.abs().max().item()))
        print(f"window attention[layer {l} Lq {q.shape[2]} Lk {k.shape[2]}]: native {err:.3e}  eager E {e:.3e}  bar {bar:.3e}")
        assert err <= bar, (l, err, bar)


# ---------------------------------------------------------------------------------------------------
# 1. the twin run
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ["S0", "Skeep"])
@pytest.mark.parametrize("L", [64, 512])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("protocol", ["update", "pre_rope"])
def test_twin_run(protocol, ids, dtype, L, S):
    keep = int(RATIO * L)
    S = keep if S == "Skeep" else 0
    w, u, keep, W = _run_twins(protocol, ids, dtype, L, S)
    assert [st.pinned for st in w.cache._layers] == [TEXT] * LAYERS
    # the next chunk's attention reads the windowed rows: [pinned | window | chunk]
    at = len(w.log)
    w.step(2 + CHUNKS, L, video=True)
    assert w.log[at][1].shape[2] == TEXT + _rule(CHUNKS, keep, W, S)[-1][0] + L
    _attention_within_bars(w.log[at:], dtype)


def test_twin_run_without_reforge():
    _run_twins("update", "mrope", torch.bfloat16, 512, 0, reforge=False)


@pytest.mark.parametrize("kw", [{"score_rounding": "fast"}, {"overlap_streams": 2}, {"flush_every_layers": 1},
                                {"in_place_compaction": False}],
                         ids=["score_fast", "overlap_streams", "flush_every_layers", "staged_eviction"])
def test_twin_run_beside_other_options(kw):
    _run_twins("update", "mrope", torch.bfloat16, 512, 0, chunks=3, **kw)


# ---------------------------------------------------------------------------------------------------
# 2. fp8 rows: the archive is the video region
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ["S0", "Skeep"])
@pytest.mark.parametrize("L", [64, 512])
def test_twin_run_fp8(L, S):
    keep = int(RATIO * L)
    W, S = keep + keep // 2, (keep if S == "Skeep" else 0)
    w = _driver("pre_rope", "mrope", torch.bfloat16, L, W=W, S=S, fp8=True)
    u = _driver("pre_rope", "mrope", torch.bfloat16, L, fp8=True)
    for d in (w, u):
        d.step(1, TEXT)
    for c, (region, dropped, slides) in enumerate(_rule(CHUNKS, keep, W, S)):
        for d in (w, u):
            d.step(2 + c, L, video=True)
        what = ("fp8", L, S, "chunk", c)
        pw, pu = w.cache.position_cache, u.cache.position_cache
        for l in range(LAYERS):
            assert w.cache.archive_len(l) == region and u.cache.archive_len(l) == (c + 1) * keep, what
            for name, a, b in zip(("k8", "v8", "ks8", "vs8"), w.cache.archive(l), u.cache.archive(l)):
                _same(a, b.narrow(2, b.shape[2] - region, region), (what, name, l))
            _same(pw[l], _windowed(pu[l], region, 2), (what, "ids", l))
            sw, su = w.cache._layers[l], u.cache._layers[l]          # the 16-bit rows: the text, untouched
            assert sw.length == su.length == TEXT and sw.archive_at == TEXT
            _same(sw.k[:, :, :TEXT], su.k[:, :, :TEXT], (what, "K16", l))
            _same(sw.v[:, :, :TEXT], su.v[:, :, :TEXT], (what, "V16", l))
            assert int(w.cache.get_prev_temporal_idx(l)) == int(u.cache.get_prev_temporal_idx(l))
        _check_counters(w.cache, c, L, keep, region, dropped, what)
    assert slides >= 1
    # the next chunk's attention over [archive window | text | chunk]: the log holds dense views only for the 16-bit rows,
    # so the truth is taken over the dequantised dense rows the cache hands out
    at = len(w.log)
    w.step(2 + CHUNKS, L, video=True, after_forward=False)
    import retake.longvideo_cache as lc

    for l, (q, k16, v16, out) in enumerate(w.log[at:]):
        a = w.cache.archive(l)
        k = torch.cat([lc.fp8_dequantize_rows(a[0], a[2], torch.bfloat16), k16], dim=2)
        v = torch.cat([lc.fp8_dequantize_rows(a[1], a[3], torch.bfloat16), v16], dim=2)
        # every archive row is visible to every query row; the text rows and the chunk are causal by index.  With the
        # text in front of the chunk in both orders the visible set of each row is the same
        ref = ar.attention_fp64(q, k, v)
        err = (out.double() - ref).abs().max().item()
        e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(torch.bfloat16, ref.abs().max().item()))
        print(f"window attention fp8[layer {l}]: native {err:.3e}  eager E {e:.3e}  bar {bar:.3e}")
        assert err <= bar, (l, err, bar)
    w.cache.after_forward()


# ---------------------------------------------------------------------------------------------------
# 3. marks, rewind, fork
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,protocol", [(64, "update"), (512, "pre_rope")])
def test_marks_across_a_slide(L, protocol):
    keep = int(RATIO * L)
    W = keep + keep // 2
    a = _driver(protocol, "mrope", torch.bfloat16, L, W=W)
    u = _driver(protocol, "mrope", torch.bfloat16, L)
    for d in (a, u):
        d.step(1, TEXT)
        d.step(2, L, video=True)
    early = a.cache.mark()                      # before the first slide (chunk 2 brings the region to 2 keep > W)
    old_end = a.cache.video_end
    for d in (a, u):
        d.step(3, L, video=True)
    assert a.cache.window_dropped == [2 * keep - W] * LAYERS
    before = _state(a.cache)
    for m in (early, old_end):
        with pytest.raises(ValueError, match="rewritten wholesale"):
            a.cache.rewind(m)
    _same_state(a.cache, before, "a mark from before the slide")
    assert a.cache.window_dropped == [2 * keep - W] * LAYERS
    # video_end, taken right after the slide, is good: a question, then back
    ve = a.cache.video_end
    assert ve is not None and ve.epoch == a.cache._epoch and ve.layers[0].length == TEXT + W
    t = a.t_next
    a.step(10, QUESTION)
    assert a.cache.get_seq_length(0) == TEXT + W + QUESTION
    a.cache.rewind(ve)
    a.t_next = t
    _same_state(a.cache, before, "after the question and the rewind")
    b = _driver(protocol, "mrope", torch.bfloat16, L, W=W)       # a cache that was never asked
    b.step(1, TEXT)
    for c in range(2):
        b.step(2 + c, L, video=True)
    _same_state(a.cache, b.cache, "against a cache that was never asked")
    assert a.cache.window_dropped == b.cache.window_dropped
    # more video after that rewind still equals the twin
    for c, (region, dropped, _) in list(enumerate(_rule(CHUNKS, keep, W, 0)))[2:]:
        for d in (a, u):
            d.step(2 + c, L, video=True)
        _check_twin(a, u, region, ("after the rewind, chunk", c))
        _check_counters(a.cache, c, L, keep, region, dropped, ("after the rewind, chunk", c))


def test_a_branch_forked_before_a_slide_is_dead():
    L = 64
    keep = int(RATIO * L)
    a = _driver("update", "mrope", torch.bfloat16, L, W=keep + keep // 2)
    a.step(1, TEXT)
    a.step(2, L, video=True)
    br = a.cache.fork()
    br.mark()                                   # alive
    a.step(3, L, video=True)                    # the parent slides
    assert a.cache.window_dropped[0] > 0
    with pytest.raises(ValueError, match="parent cache"):
        br.mark()
    q, k, v = _qkv(9000, 1, torch.bfloat16)
    with pytest.raises(ValueError, match="parent cache"):
        br.update(k, v, 0, {})
    live = a.cache.fork()                       # a branch forked after the slide is fine
    live.mark()


# ---------------------------------------------------------------------------------------------------
# 4. the plateau
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_capacity_stops_growing(fp8):
    L, S = 64, 0
    keep = int(RATIO * L)
    W = keep + keep // 2
    a = _driver("pre_rope" if fp8 else "update", "mrope", torch.bfloat16, L, W=W, S=S, reserve=TEXT + W + S + L + QUESTION, fp8=fp8)
    a.step(1, TEXT)

    def pointers():
        out = []
        for st in a.cache._layers:
            out.append(tuple((t.data_ptr(), tuple(t.shape)) for t in (st.k, st.v, st.pos, st.k8, st.v8, st.ks8, st.vs8)
                             if t is not None))
        return out

    seen = {}
    for c in range(12):
        a.step(2 + c, L, video=True)
        a.log.clear()
        if c + 1 in (4, 12):
            seen[c + 1] = (pointers(), a.cache.memory_footprint())
    assert seen[4][0] == seen[12][0]
    assert seen[4][1] == seen[12][1]
    assert a.cache.get_seq_length(0) == TEXT + W and a.cache.window_dropped == [12 * keep - W] * LAYERS
    assert all(st.k.shape[2] >= TEXT + (0 if fp8 else W + S) + L + QUESTION for st in a.cache._layers)


def test_growth_is_sized_for_the_window():
    """A layer that outgrows its first buffer before the window is full grows ONCE, to pinned + W + S + one chunk."""
    L, W, S = 512, 2000, 100
    a = _driver("update", "mrope", torch.bfloat16, L, W=W, S=S)
    a.step(1, TEXT)
    assert a.cache._layers[0].k.shape[2] == 1024
    for c in range(CHUNKS):
        a.step(2 + c, L, video=True)
        a.log.clear()
    assert a.cache.window_dropped == [] and a.cache.get_seq_length(0) == TEXT + CHUNKS * int(RATIO * L)
    assert all(st.k.shape[2] == st.v.shape[2] == TEXT + W + S + L for st in a.cache._layers)


# ---------------------------------------------------------------------------------------------------
# 5. window off, and the launch count
# ---------------------------------------------------------------------------------------------------
def _slide_launches(fn):
    import retake._native as nv

    kid = nv.profile_kernel_ids()["slide_units"]
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable_mask(1 << kid)
    try:
        fn()
        return nv.profile_read().get("slide_units", (0, 0.0))[0]
    finally:
        nv.lib.rtk_profile_enable(0)
        nv.lib.rtk_profile_reset()


def _five_chunks(d, L):
    d.step(1, TEXT)
    for c in range(CHUNKS):
        d.step(2 + c, L, video=True)


@pytest.mark.parametrize("L", [64, 512])
def test_window_off_changes_nothing_and_launches_nothing(L):
    keep = int(RATIO * L)
    off = _driver("update", "mrope", torch.bfloat16, L, W="off")
    assert "video_window_rows" in off.cache.config.longvideo_kwargs and off.cache.video_window_rows is None
    twin = _Driver("update", "mrope", torch.bfloat16, L, compression_ratio=RATIO)     # a config that never heard of the keys
    assert _slide_launches(lambda: _five_chunks(off, L)) == 0
    _five_chunks(twin, L)
    _same_state(off.cache, twin.cache, "window off")
    assert off.cache.window_dropped == [] and off.cache._epoch == twin.cache._epoch
    assert off.cache.num_evicted_tokens == [CHUNKS * (L - keep)] * LAYERS
    # with the window on: ONE launch per slide, all layers and tensors in it
    on = _driver("update", "mrope", torch.bfloat16, L, W=keep + keep // 2)
    assert _slide_launches(lambda: _five_chunks(on, L)) == _rule(CHUNKS, keep, keep + keep // 2, 0)[-1][2]


def test_no_after_forward_no_window():
    """Slides happen in after_forward only: a caller that never calls it keeps every row."""
    L = 64
    keep = int(RATIO * L)
    a = _driver("update", "mrope", torch.bfloat16, L, W=keep + keep // 2)
    a.step(1, TEXT)
    for c in range(3):
        a.step(2 + c, L, video=True, after_forward=False)
    assert a.cache.get_seq_length(0) == TEXT + 3 * keep and a.cache.window_dropped == []

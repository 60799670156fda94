"""The video budget of PivotKVCache (video_budget_rows / video_budget_slack) on the GPU.  Every case is a TWIN comparison,
bit for bit: the same inputs go to a cache with the budget and to one whose budget is so large that it never evicts - which
therefore stores the score of every kept row.  After every after_forward the rule (tests/budget_ref.py) is simulated on the
twin's `row_scores`, layer by layer, which gives the indices of the rows that are still alive; the budget cache's K, V, ids
and row_scores must be the twin's pinned rows followed by its region rows at those indices: scoring, selection and the
reforged ids depend only on the chunk and on the last stored temporal id, and the newest row always survives.

Shapes: test_window_gpu's - 2 layers, Hq 4, Hkv 2, D 128 (the driver and helpers of tests/test_rewind_gpu.py), 5 text rows,
then 6 chunks of L = 64 (selection inside update) or L = 512 (the batched flush), compression ratio 0.5, B = 1.5 x keep - an
eviction cuts inside chunks - with slack 0 and slack = keep.  Every chunk carries a key-patch mask (30 % of its tokens), so
exact ties at 1.0 occur in every region."""
import numpy as np
import pytest
import torch

import budget_ref as br
import synth
from test_rewind_gpu import SEC, A, D, LAYERS, TEXT, _cfg, _Driver, _qkv, _same, _same_state, _state, dev
from test_window_gpu import _attention_within_bars

pytestmark = pytest.mark.gpu

RATIO, CHUNKS, QUESTION = 0.5, 6, 7
NEVER = 1 << 14          # the twin's budget: never reached, so the twin only stores its scores


class _BudgetDriver(_Driver):
    """test_rewind_gpu's driver at ratio 0.5 around ONE cache built from a config that carries the two budget keys, with a
    key-patch mask on every video chunk.  float32 models run without the native attention (it serves 16-bit rows)."""

    def __init__(self, protocol, ids, dtype, L, B=None, S=0, reserve=None, reforge=True, fp8=False, **extra):
        import retake.longvideo_cache as lc

        cfg = _cfg(reforge, fp8, compression_ratio=RATIO, **extra)
        self.attend = dtype is not torch.float32
        if not self.attend:
            cfg.longvideo_kwargs["attention_kernel"] = None
        if B is not None:   # ("off": the keys spelled out with their defaults)
            cfg.longvideo_kwargs.update(video_budget_rows=None if B == "off" else B, video_budget_slack=S)
        self.cache = lc.build_kvcache(cfg, **({"reserve_tokens": reserve} if reserve else {}))
        self.protocol, self.mrope, self.dtype, self.L, self.prompt = protocol, ids == "mrope", dtype, L, 0
        self.sec = SEC if self.mrope else None
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.t_next = 0
        self.log = []

    def step(self, seed, n, video=False, t0=None, after_forward=True, layers=range(LAYERS)):
        cache = self.cache
        pos = self._video_ids(n, 0) if video else self._text_ids(n, t0)
        cache.keypatches_mask_chunk = _mask(seed, n) if video else None
        for l in layers:
            q, k, v = _qkv(1000 * seed + l, n, self.dtype)
            qr, kk, vv = self._feed(l, q, k, v, pos, video)
            if self.attend:
                out = cache.attention(qr, kk, vv, layer_idx=l)
                assert out is not None
                self.log.append((qr.clone(), kk.clone(), vv.clone(), out.clone()))
        cache.keypatches_mask_chunk = None
        try:
            if video and after_forward:
                cache.after_forward()
        finally:
            cache.kvcache_compression = False


def _mask(seed, n):
    return torch.from_numpy(np.random.default_rng(seed).uniform(size=n) < 0.3).to(dev())


_driver = _BudgetDriver


def _alive(u, B, S, chunks_so_far, keep):
    """Per layer: (alive region indices, dropped, evictions) after `chunks_so_far` chunks, simulated on the twin's scores."""
    out = []
    for l in range(LAYERS):
        s = u.cache.row_scores(l)
        assert s.dtype == torch.float32 and s.numel() == chunks_so_far * keep, (l, s.shape)
        out.append(br.simulate(list(s.cpu().split(keep)), B, S)[-1])
    return out


def _pick(t, alive, dim=2):
    """[pinned rows | region rows at `alive`] of the twin's tensor."""
    idx = torch.cat([torch.arange(TEXT), TEXT + alive]).to(t.device)
    return t.index_select(dim, idx)


def _check_twin(w, u, alive, what):
    """The budget cache against the twin, every layer: K, V, ids, scores, the last temporal id."""
    pw, pu = w.cache.position_cache, u.cache.position_cache
    assert len(pw) == len(pu), what                      # (no reforging: no ids are kept, by either)
    for l in range(LAYERS):
        a = alive[l][0]
        assert w.cache.get_seq_length(l) == TEXT + a.numel(), (what, l)
        _same(w.cache.key_cache[l], _pick(u.cache.key_cache[l], a), (what, "K", l))
        _same(w.cache.value_cache[l], _pick(u.cache.value_cache[l], a), (what, "V", l))
        if l < len(pu) and isinstance(pu[l], torch.Tensor):
            _same(pw[l], _pick(pu[l], a, pu[l].ndim - 1), (what, "ids", l))
        _same(w.cache.row_scores(l), u.cache.row_scores(l)[a.to(dev())], (what, "scores", l))
        assert int(w.cache.get_prev_temporal_idx(l)) == int(u.cache.get_prev_temporal_idx(l)), (what, l)


def _check_counters(cache, c, L, keep, alive, what):
    dropped = [a[1] for a in alive]
    assert cache.num_evicted_tokens == [(c + 1) * (L - keep) + d for d in dropped], what
    assert (cache.budget_dropped or [0] * LAYERS) == dropped, what
    assert [cache.get_seq_length(l) for l in range(LAYERS)] == [TEXT + a[0].numel() for a in alive], what
    assert cache.window_dropped == [], what


def _stored_scores_are_what_the_selection_saw(u, chunks, keep, L):
    """The last layer's last chunk: the stored scores are score[keep_idx[r]] of the chunk's score row as the selection left
    it - AFTER the key-patch override, so every kept key-patch token holds exactly 1.0 (not every key-patch token is kept:
    a score above 1.0 outranks it, as in the reference)."""
    idx = u.cache.last_keep_indices
    stored = u.cache.row_scores(LAYERS - 1)[-keep:]
    _same(stored, u.cache.last_scores[idx], "scores of the last chunk")
    patch = _mask(2 + chunks - 1, L)[idx]
    assert int(patch.sum()) > 0 and bool((stored[patch] == 1.0).all())


def _run_twins(protocol, ids, dtype, L, S, chunks=CHUNKS, **kw):
    keep = int(RATIO * L)
    B = keep + keep // 2
    w = _driver(protocol, ids, dtype, L, B=B, S=S, **kw)
    u = _driver(protocol, ids, dtype, L, B=NEVER, **kw)
    for d in (w, u):
        d.step(1, TEXT)
    epoch = w.cache._epoch
    for c in range(chunks):
        for d in (w, u):
            d.step(2 + c, L, video=True)
        what = (protocol, ids, dtype, L, S, "chunk", c)
        alive = _alive(u, B, S, c + 1, keep)
        assert all(a[0].numel() <= B + S for a in alive)
        _check_twin(w, u, alive, what)
        _check_counters(w.cache, c, L, keep, alive, what)
        assert w.cache._epoch == epoch + alive[0][2], what      # an eviction, and nothing else here, moves the epoch
        assert w.cache.video_end is not None and w.cache.video_end.epoch == w.cache._epoch
    assert alive[0][2] >= 2 and u.cache.get_seq_length(0) == TEXT + chunks * keep and u.cache.budget_dropped == []
    _stored_scores_are_what_the_selection_saw(u, chunks, keep, L)
    return w, u, keep, B


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
    w, u, keep, B = _run_twins(protocol, ids, dtype, L, S)
    assert [st.pinned for st in w.cache._layers] == [TEXT] * LAYERS
    # the next chunk's attention reads the budget cache's rows: [pinned | survivors | chunk]
    at = len(w.log)
    n = w.cache.get_seq_length(0)
    w.step(2 + CHUNKS, L, video=True)
    assert w.log[at][1].shape[2] == n + L
    _attention_within_bars(w.log[at:], dtype)


@pytest.mark.parametrize("L", [64, 512])
def test_twin_run_fp32(L):
    _run_twins("update", "mrope", torch.float32, L, 0)


def test_twin_run_without_reforge():
    _run_twins("update", "mrope", torch.bfloat16, 512, 0, reforge=False)


@pytest.mark.parametrize("kw", [{"score_rounding": "fast"}, {"score_rounding": "reference"}, {"overlap_streams": 2},
                                {"flush_every_layers": 1}, {"in_place_compaction": False}],
                         ids=["score_fast", "score_reference", "overlap_streams", "flush_every_layers", "staged_eviction"])
def test_twin_run_beside_other_options(kw):
    _run_twins("update", "mrope", torch.bfloat16, 512, 0, chunks=4, **kw)


# ---------------------------------------------------------------------------------------------------
# 2. fp8 rows: the archive is the video region
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ["S0", "Skeep"])
@pytest.mark.parametrize("L", [64, 512])
def test_twin_run_fp8(L, S):
    import retake.longvideo_cache as lc

    keep = int(RATIO * L)
    B, S = keep + keep // 2, (keep if S == "Skeep" else 0)
    w = _driver("pre_rope", "mrope", torch.bfloat16, L, B=B, S=S, fp8=True)
    u = _driver("pre_rope", "mrope", torch.bfloat16, L, B=NEVER, fp8=True)
    for d in (w, u):
        d.step(1, TEXT)
    for c in range(CHUNKS):
        for d in (w, u):
            d.step(2 + c, L, video=True)
        what = ("fp8", L, S, "chunk", c)
        alive = _alive(u, B, S, c + 1, keep)
        pw, pu = w.cache.position_cache, u.cache.position_cache
        for l in range(LAYERS):
            a = alive[l][0].to(dev())
            assert w.cache.archive_len(l) == a.numel() and u.cache.archive_len(l) == (c + 1) * keep, what
            for name, x, y in zip(("k8", "v8", "ks8", "vs8"), w.cache.archive(l), u.cache.archive(l)):
                _same(x, y.index_select(2, a), (what, name, l))
            _same(pw[l], _pick(pu[l], alive[l][0], 2), (what, "ids", l))
            _same(w.cache.row_scores(l), u.cache.row_scores(l)[a], (what, "scores", l))
            # the dequantised dense copies, in sequence order: [text | archive]
            _same(w.cache.key_cache[l], _pick(u.cache.key_cache[l], alive[l][0]), (what, "K dense", l))
            _same(w.cache.value_cache[l], _pick(u.cache.value_cache[l], alive[l][0]), (what, "V dense", l))
            sw, su = w.cache._layers[l], u.cache._layers[l]          # the 16-bit rows: the text, untouched
            assert sw.length == su.length == TEXT and sw.archive_at == TEXT
            _same(sw.k[:, :, :TEXT], su.k[:, :, :TEXT], (what, "K16", l))
            _same(sw.v[:, :, :TEXT], su.v[:, :, :TEXT], (what, "V16", l))
            assert int(w.cache.get_prev_temporal_idx(l)) == int(u.cache.get_prev_temporal_idx(l))
        _check_counters(w.cache, c, L, keep, alive, what)
    assert alive[0][2] >= 2
    # the next chunk's attention over [archive survivors | text | chunk], against float64 on the dequantised rows
    at = len(w.log)
    w.step(2 + CHUNKS, L, video=True, after_forward=False)
    import attention_ref as ar

    for l, (q, k16, v16, out) in enumerate(w.log[at:]):
        a = w.cache.archive(l)
        k = torch.cat([lc.fp8_dequantize_rows(a[0], a[2], torch.bfloat16), k16], dim=2)
        v = torch.cat([lc.fp8_dequantize_rows(a[1], a[3], torch.bfloat16), v16], dim=2)
        ref = ar.attention_fp64(q, k, v)
        err = (out.double() - ref).abs().max().item()
        e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(torch.bfloat16, ref.abs().max().item()))
        print(f"budget attention fp8[layer {l}]: native {err:.3e}  eager E {e:.3e}  bar {bar:.3e}")
        assert err <= bar, (l, err, bar)
    w.cache.after_forward()


# ---------------------------------------------------------------------------------------------------
# 3. marks, rewind, fork, questions
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,protocol", [(64, "update"), (512, "pre_rope")])
def test_marks_and_questions_across_an_eviction(L, protocol):
    keep = int(RATIO * L)
    B = keep + keep // 2
    a = _driver(protocol, "mrope", torch.bfloat16, L, B=B)
    u = _driver(protocol, "mrope", torch.bfloat16, L, B=NEVER)
    for d in (a, u):
        d.step(1, TEXT)
        d.step(2, L, video=True)
    early = a.cache.mark()                      # before the first eviction (chunk 2 brings the region to 2 keep > B)
    old_end = a.cache.video_end
    for d in (a, u):
        d.step(3, L, video=True)
    assert a.cache.budget_dropped == [2 * keep - B] * LAYERS
    before = _state(a.cache)
    scores = [a.cache.row_scores(l) for l in range(LAYERS)]
    for m in (early, old_end):
        with pytest.raises(ValueError, match="rewritten wholesale"):
            a.cache.rewind(m)
    _same_state(a.cache, before, "a mark from before the eviction")
    # video_end, taken right after the eviction, is good: a question, then back, and the stream goes on
    ve = a.cache.video_end
    assert ve is not None and ve.epoch == a.cache._epoch and ve.layers[0].length == TEXT + B and ve.layers[0].sc_len == B
    t = a.t_next
    a.step(10, QUESTION)
    assert a.cache.get_seq_length(0) == TEXT + B + QUESTION
    a.cache.rewind(ve)
    a.t_next = t
    _same_state(a.cache, before, "after the question and the rewind")
    for l in range(LAYERS):
        _same(a.cache.row_scores(l), scores[l], ("scores after the rewind", l))
    for c in (2, 3):
        for d in (a, u):
            d.step(2 + c, L, video=True)
        alive = _alive(u, B, 0, c + 1, keep)
        _check_twin(a, u, alive, ("after the rewind, chunk", c))
        _check_counters(a.cache, c, L, keep, alive, ("after the rewind, chunk", c))
    # a question left in place: its rows carry no score, the next eviction raises and changes nothing
    a.step(11, QUESTION)
    epoch, dropped = a.cache._epoch, list(a.cache.budget_dropped)
    with pytest.raises(ValueError, match="video_end"):
        a.step(6, L, video=True)
    assert a.cache._epoch == epoch and a.cache.budget_dropped == dropped
    assert a.cache.get_seq_length(0) == TEXT + B + QUESTION + keep            # the chunk itself was flushed


def test_a_branch_forked_before_an_eviction_is_dead():
    L = 64
    keep = int(RATIO * L)
    a = _driver("update", "mrope", torch.bfloat16, L, B=keep + keep // 2)
    a.step(1, TEXT)
    a.step(2, L, video=True)
    br_ = a.cache.fork()
    br_.mark()                                  # alive
    assert br_.video_budget_rows is None and all(st.sc is None for st in br_._layers)   # a fork needs no score buffer
    a.step(3, L, video=True)                    # the parent evicts
    assert a.cache.budget_dropped[0] > 0
    with pytest.raises(ValueError, match="parent cache"):
        br_.mark()
    q, k, v = _qkv(9000, 1, torch.bfloat16)
    with pytest.raises(ValueError, match="parent cache"):
        br_.update(k, v, 0, {})
    live = a.cache.fork()                       # a branch forked after the eviction is fine
    live.mark()


# ---------------------------------------------------------------------------------------------------
# 4. the plateau
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_capacity_stops_growing(fp8):
    L, S = 64, 0
    keep = int(RATIO * L)
    B = keep + keep // 2
    a = _driver("pre_rope" if fp8 else "update", "mrope", torch.bfloat16, L, B=B, S=S, reserve=TEXT + B + S + L + QUESTION, fp8=fp8)
    a.step(1, TEXT)

    def pointers():
        out = []
        for st in a.cache._layers:
            out.append(tuple((t.data_ptr(), tuple(t.shape)) for t in (st.k, st.v, st.pos, st.k8, st.v8, st.ks8, st.vs8, st.sc)
                             if t is not None))
        return out

    seen = {}
    for c in range(12):
        a.step(2 + c, L, video=True)
        a.log.clear()
        if c + 1 in (4, 12):
            seen[c + 1] = (pointers(), a.cache.memory_footprint())
    assert seen[4][0] == seen[12][0]
    assert seen[4][1] == seen[12][1] and seen[4][1]["row_scores"] > 0
    assert a.cache.get_seq_length(0) == TEXT + B and a.cache.budget_dropped == [12 * keep - B] * LAYERS
    assert all(st.k.shape[2] >= TEXT + (0 if fp8 else B + S) + L + QUESTION for st in a.cache._layers)


def test_growth_is_sized_for_the_budget():
    """A layer that outgrows its first buffer before the budget is full grows ONCE, to pinned + B + S + one chunk."""
    L, B, S = 512, 2000, 100
    a = _driver("update", "mrope", torch.bfloat16, L, B=B, S=S)
    a.step(1, TEXT)
    assert a.cache._layers[0].k.shape[2] == 1024
    for c in range(5):
        a.step(2 + c, L, video=True)
        a.log.clear()
    assert a.cache.budget_dropped == [] and a.cache.get_seq_length(0) == TEXT + 5 * int(RATIO * L)
    assert all(st.k.shape[2] == st.v.shape[2] == TEXT + B + S + L for st in a.cache._layers)
    assert all(st.sc.numel() == B + S + L for st in a.cache._layers)


# ---------------------------------------------------------------------------------------------------
# 5. budget off, and the launch counts
# ---------------------------------------------------------------------------------------------------
def _launches(fn, names=("keep_scores", "budget_select", "squeeze_units")):
    import retake._native as nv

    kids = nv.profile_kernel_ids()
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable_mask(sum(1 << kids[n] for n in names))
    try:
        fn()
        got = nv.profile_read()
        return tuple(got.get(n, (0, 0.0))[0] for n in names)
    finally:
        nv.lib.rtk_profile_enable(0)
        nv.lib.rtk_profile_reset()


def _chunks(d, L, n=CHUNKS):
    d.step(1, TEXT)
    for c in range(n):
        d.step(2 + c, L, video=True)


@pytest.mark.parametrize("L", [64, 512])
def test_budget_off_changes_nothing_and_launches_nothing(L):
    keep = int(RATIO * L)
    off = _driver("update", "mrope", torch.bfloat16, L, B="off")
    assert "video_budget_rows" in off.cache.config.longvideo_kwargs and off.cache.video_budget_rows is None
    twin = _driver("update", "mrope", torch.bfloat16, L)                  # a config that never heard of the keys
    assert _launches(lambda: _chunks(off, L)) == (0, 0, 0)
    _chunks(twin, L)
    _same_state(off.cache, twin.cache, "budget off")
    assert off.cache.budget_dropped == [] and off.cache._epoch == twin.cache._epoch
    assert off.cache.num_evicted_tokens == [CHUNKS * (L - keep)] * LAYERS
    assert all(st.sc is None for st in off.cache._layers) and "row_scores" not in off.cache.memory_footprint()
    # with the budget on: one score gather per flush, ONE select and ONE squeeze launch per eviction, all layers in them
    on = _driver("update", "mrope", torch.bfloat16, L, B=keep + keep // 2)
    evictions = br.simulate([torch.zeros(keep)] * CHUNKS, keep + keep // 2, 0)[-1][2]
    assert _launches(lambda: _chunks(on, L)) == (CHUNKS, evictions, evictions)


def test_no_after_forward_no_budget():
    """Evictions happen in after_forward only: a caller that never calls it keeps every row."""
    L = 64
    keep = int(RATIO * L)
    a = _driver("update", "mrope", torch.bfloat16, L, B=keep + keep // 2)
    a.step(1, TEXT)
    for c in range(3):
        a.step(2 + c, L, video=True, after_forward=False)
    assert a.cache.get_seq_length(0) == TEXT + 3 * keep and a.cache.budget_dropped == []
    assert a.cache.row_scores(0).numel() == 3 * keep                      # ... and the scores are kept all the same

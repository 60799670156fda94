"""video_budget_rescore over fp8 archive rows (archive_rescore) at cache level: the step simulation of
tests/test_budget_rescore_gpu.py with kv_cache_dtype="fp8_e4m3".  2 layers, Hq 4 / Hkv 2 / D 128, 5 text rows, chunks of 256
rows keeping 64, B = 600 with slack 64 - the region crosses one key-range boundary (512) and is evicted twice in 13 chunks -
and, because chunks below 512 rows leave the fused pre-RoPE route, one run with chunks of 512 keeping 128 on that route.

Bit for bit: a chunk is fed without after_forward, the archive (codes, scales), the ids, the scores and the observed queries
are snapshot, the 16-BIT kernel (rtk_pivotkv_rescore_batched) runs from the test on a dequantised copy of the archive's key
rows, the budget's rule (tests/budget_ref.py) picks the survivors of the blended scores, and after `after_forward` the cache
must hold exactly those codes, scales, ids and scores, with the counters of the 16-bit case.  Rule 5 of the fp8 rows makes the
dequantised rows exact, so no tolerance enters.

The heavy-hitter test is the one that fails without the feature (build_kvcache refuses the keys together on the parent)."""
import pytest
import torch

import budget_ref as br
import rescore_ref as rr
from test_budget_gpu import QUESTION, _check_counters
from test_budget_rescore_gpu import ALPHA, KEY, ROWS, _heavy_hitter_chunk, _RescoreDriver
from test_prompt_score_gpu import BAR
from test_rescore_gpu import rescore
from test_rewind_gpu import LAYERS, TEXT, Hkv, Hq, D, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

ON = "archive_rescore"
B, S = 600, 64


def _fp8_driver(protocol, ids, dtype, L, ratio, top, **kw):
    d = _RescoreDriver(protocol, ids, dtype, L, top=top, fp8=True, **kw)
    # (_BudgetDriver builds its config at ratio 0.5: the keep of this file's chunks goes in beside the other keys)
    cfg = d.cache.config
    cfg.longvideo_kwargs["kvcache_compression_kwargs"]["compression_ratio"] = ratio
    import retake.longvideo_cache as lc

    d.cache = lc.build_kvcache(cfg)
    return d


def _region(cache, l):
    """Clones of the layer's scores (this flushes), archive (k8, v8, ks8, vs8), ids, observed queries and 16-bit rows."""
    sc = cache.row_scores(l)
    pos = cache.position_cache
    ids = pos[l].clone() if l < len(pos) and isinstance(pos[l], torch.Tensor) else None
    st = cache._layers[l]
    return (sc, tuple(t.clone() for t in cache.archive(l)), ids, cache.observed_queries(l),
            (st.k[:, :, :st.length].clone(), st.v[:, :, :st.length].clone()))


def _blend_by_the_16_bit_kernel(sc, k8, ks8, oq, n_old, dtype):
    from retake.native_attention import fp8_dequantize_rows

    if n_old == 0:
        return sc
    k = fp8_dequantize_rows(k8[:, :, :n_old].contiguous(), ks8[:, :, :n_old].contiguous(), dtype)[0].contiguous()
    return rescore([(oq, k, sc, n_old)], Hq, Hkv, oq.shape[1], D, dtype, ALPHA)[0]


def _pick_ids(t, idx):
    return t.index_select(t.ndim - 1, torch.cat([torch.arange(TEXT), TEXT + idx]).to(t.device))


def _simulate(protocol, ids, dtype, L=256, ratio=0.25, W=None, chunks=13, **kw):
    keep = int(ratio * L)
    top = {KEY: ALPHA, ON: True, "video_budget_rows": B, "video_budget_slack": S}
    if W is not None:
        top[ROWS] = W
    d = _fp8_driver(protocol, ids, dtype, L, ratio, top, **kw)
    cache = d.cache
    assert cache.archive_rescore is True and cache.kv_cache_dtype == "fp8_e4m3" and cache.video_budget_rows == B
    d.step(1, TEXT)
    seen = [rr.Seen() for _ in range(LAYERS)]
    dropped, evictions, rescored, crossed = [0] * LAYERS, 0, [0] * LAYERS, False
    for c in range(chunks):
        d.step(2 + c, L, video=True, after_forward=False)
        d.log.clear()
        snap = [_region(cache, l) for l in range(LAYERS)]
        expect = []
        for l, (sc, arch, pid, oq, _) in enumerate(snap):
            what = (protocol, ids, dtype, L, "chunk", c, "layer", l)
            n = sc.numel()
            assert n == arch[0].shape[2] == (c + 1) * keep - dropped[l], what
            assert oq.shape == (Hq, min(W or 64, L), D) and oq.dtype == dtype, what
            n_old = seen[l].rescore(n)
            rescored[l] += n_old > 0
            crossed |= n_old > 512
            blended = _blend_by_the_16_bit_kernel(sc, arch[0], arch[2], oq, n_old, dtype)
            assert torch.equal(blended[n_old:], sc[n_old:]), what
            if n > B + S:
                surv = br.survivors(blended, B)
                dropped[l] += n - B
                seen[l].evict(B)
            else:
                surv = torch.arange(n)
            expect.append((blended, surv))
        evictions += snap[0][0].numel() > B + S
        cache.after_forward()
        for l, ((sc, arch, pid, oq, rows16), (blended, surv)) in enumerate(zip(snap, expect)):
            what = (protocol, ids, dtype, L, "chunk", c, "layer", l)
            assert cache.archive_len(l) == surv.numel(), what
            for name, got, was in zip(("k8", "v8", "ks8", "vs8"), cache.archive(l), arch):
                _same(got, was.index_select(2, surv.to(dev())), (what, name))
            _same(cache.row_scores(l), blended[surv.to(dev())], (what, "scores"))
            if pid is not None:
                _same(cache.position_cache[l], _pick_ids(pid, surv), (what, "ids"))
            st = cache._layers[l]
            assert st.length == TEXT and st.archive_at == TEXT, what
            _same(st.k[:, :, :TEXT], rows16[0], (what, "K16"))
            _same(st.v[:, :, :TEXT], rows16[1], (what, "V16"))
        what = (protocol, ids, dtype, L, "chunk", c)
        assert cache.budget_rescored == rescored or (not any(rescored) and cache.budget_rescored == []), what
        _check_counters(cache, c, L, keep, [(expect[l][1], dropped[l], evictions) for l in range(LAYERS)], what)
        assert cache.video_end is not None and cache.video_end.epoch == cache._epoch
        assert [m.sc_seen for m in cache.video_end.layers] == [s.n_old for s in seen], what
    assert evictions >= 2 and all(r == chunks - 1 for r in rescored) and crossed
    return d


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("protocol", ["update", "pre_rope"])
def test_step_simulation(protocol, ids, dtype):
    _simulate(protocol, ids, dtype, W=8 if ids == "plain" else None)


def test_step_simulation_on_the_fused_pre_rope_route():
    _simulate("pre_rope", "mrope", torch.bfloat16, L=512, chunks=7)


def test_step_simulation_without_reforge():
    _simulate("update", "mrope", torch.bfloat16, reforge=False)


# ---------------------------------------------------------------------------------------------------
# a heavy hitter survives: fails without the feature
# ---------------------------------------------------------------------------------------------------
def test_a_heavy_hitter_survives_under_fp8():
    """test_budget_rescore_gpu's heavy hitter on fp8 rows: the lowest-scored archive row of chunk 1 is what the last queries
    of chunk 2 put all their mass on.  Without video_budget_rescore it is evicted, with it (and archive_rescore) it survives
    with score (1 - alpha) old + alpha keep."""
    L, dtype = 64, torch.bfloat16
    keep = int(0.5 * L)
    Bh = keep + keep // 2
    off = _RescoreDriver("update", "mrope", dtype, L, B=Bh, S=0, fp8=True)
    on = _RescoreDriver("update", "mrope", dtype, L, B=Bh, S=0, fp8=True, top={KEY: ALPHA, ROWS: 8, ON: True})
    assert off.cache.video_budget_rescore is None and on.cache.video_budget_rescore == ALPHA and on.cache.archive_rescore
    for d in (off, on):
        d.step(1, TEXT)
        _heavy_hitter_chunk(d, 2, L)
    tails, v_star, old = [], [], []
    for l in range(LAYERS):
        s = on.cache.row_scores(l)
        _same(s, off.cache.row_scores(l), ("chunk 1", l))
        j = int(torch.argmin(s))
        k = on.cache.key_cache[l][0, :, TEXT + j]                     # [Hkv, D]: the archive row, dequantised
        tails.append((4 * k.float()).to(dtype).repeat_interleave(Hq // Hkv, dim=0)[:, None, :].expand(Hq, 8, D))
        old.append(float(s[j]))
        v_star.append(on.cache.archive(l)[1][0, :, j].clone())        # its V codes
        K = on.cache.key_cache[l][0, :, TEXT:TEXT + keep].double()
        logits = 4 * torch.einsum("gd,gjd->gj", k.double(), K) / D ** 0.5
        rest = torch.cat([logits[:, :j], logits[:, j + 1:]], dim=1)
        assert float((logits[:, j] - rest.max(dim=1).values).min()) > 50, l
    for d in (off, on):
        _heavy_hitter_chunk(d, 3, L, tails)
    assert on.cache.budget_rescored == [1] * LAYERS and off.cache.budget_rescored == []
    for l in range(LAYERS):
        def where(cache):
            return (cache.archive(l)[1][0] == v_star[l][:, None, :]).all(dim=2).all(dim=0).nonzero().flatten().tolist()
        assert where(off.cache) == [], (l, "the seed no longer evicts j* with the key off: pick another")
        at = where(on.cache)
        assert len(at) == 1, (l, "j* did not survive")
        got = float(on.cache.row_scores(l)[at[0]])
        want = 0.5 * old[l] + 0.5 * keep                              # obs = n_old: all of every query row's mass
        bar = ALPHA * (keep / 8) * BAR[dtype] * 8 + 4 * 2.0 ** -24 * want
        print(f"fp8 heavy hitter layer {l}: score {old[l]:.4f} -> {got:.6f} (want {want:.6f}, bar {bar:.2e})")
        assert abs(got - want) <= bar, (l, got, want)
    assert on.cache.num_evicted_tokens == off.cache.num_evicted_tokens and on.cache.budget_dropped == off.cache.budget_dropped


# ---------------------------------------------------------------------------------------------------
# off is off
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [{}, {ON: False}, {ON: True}], ids=["absent", "false", "on_without_rescore"])
def test_without_video_budget_rescore_no_observe_buffer_exists(top):
    L = 64
    keep = int(0.5 * L)
    d = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=keep + keep // 2, fp8=True, top=top)
    twin = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=keep + keep // 2, fp8=True)
    for x in (d, twin):
        x.step(1, TEXT)
        for c in range(4):
            x.step(2 + c, L, video=True)
    _same_state(d.cache, twin.cache, "rescore off")
    for l in range(LAYERS):
        _same(d.cache.row_scores(l), twin.cache.row_scores(l), ("scores", l))
    assert d.cache.budget_rescored == [] and d.cache.budget_dropped == twin.cache.budget_dropped and d.cache.budget_dropped[0] > 0
    assert all(st.oq is None and st.sc_seen == twin.cache._layers[i].sc_seen for i, st in enumerate(d.cache._layers))
    assert "observe_queries" not in d.cache.memory_footprint() and not any("rescore" in k for k in d.cache._ws)


# ---------------------------------------------------------------------------------------------------
# marks
# ---------------------------------------------------------------------------------------------------
def test_a_mark_below_a_rescoring():
    """As test_budget_rescore_gpu.test_marks_and_questions, on fp8 rows: a question behind `video_end` and a rewind leave
    the blended scores and the count of seen rows; the stream then goes on as one that never saw the question."""
    L = 64
    keep = int(0.5 * L)
    Bm = keep + keep // 2
    top = {KEY: ALPHA, ROWS: 16, ON: True}
    a = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=Bm, fp8=True, top=top)
    b = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=Bm, fp8=True, top=top)
    for d in (a, b):
        d.step(1, TEXT)
        for c in range(3):
            d.step(2 + c, L, video=True)
    assert a.cache.budget_rescored == [2] * LAYERS and a.cache.budget_dropped[0] > 0
    ve = a.cache.video_end
    assert ve is not None and ve.epoch == a.cache._epoch and ve.layers[0].sc_len == Bm and ve.layers[0].sc_seen == Bm
    before = _state(a.cache)
    scores = [a.cache.row_scores(l) for l in range(LAYERS)]
    t = a.t_next
    a.step(10, QUESTION)
    assert a.cache.get_seq_length(0) == TEXT + Bm + QUESTION
    a.cache.rewind(ve)
    a.t_next = t
    _same_state(a.cache, before, "after the question and the rewind")
    for l in range(LAYERS):
        _same(a.cache.row_scores(l), scores[l], ("blended scores stay after the rewind", l))
    assert [st.sc_seen for st in a.cache._layers] == [Bm] * LAYERS
    for c in (3, 4):
        for d in (a, b):
            d.step(2 + c, L, video=True)
        _same_state(a.cache, b.cache, ("the stream after the rewind, chunk", c))
        for l in range(LAYERS):
            _same(a.cache.row_scores(l), b.cache.row_scores(l), ("scores after the rewind, chunk", c, l))
    assert a.cache.budget_rescored == b.cache.budget_rescored == [4] * LAYERS

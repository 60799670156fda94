"""video_budget_rescore at cache level, on test_budget_gpu's driver and shapes: 2 layers, Hq 4 / Hkv 2 / D 128, 5 text rows,
chunks of L = 64 (selection inside update) and 512 (the batched flush), ratio 0.5, B = 1.5 x keep, slack 0 and keep.

The step simulation is bit for bit: a chunk is fed without after_forward, the region (scores, K, V, ids) and the observed
queries are snapshot, rtk_pivotkv_rescore_batched runs from the test on COPIES of them (other addresses, another key head
stride, a call of one unit: the kernel's sums are layout-independent), the budget's rule (tests/budget_ref.py) picks the
survivors of the blended scores, and after `after_forward` the cache must hold exactly those rows with exactly those
scores.  The blended scores themselves are checked against tests/rescore_ref.py under test_rescore_gpu's bar.

The heavy-hitter test is the one that fails without the feature."""
import pytest
import torch

import budget_ref as br
import rescore_ref as rr
import synth
from test_budget_gpu import CHUNKS, QUESTION, RATIO, _BudgetDriver, _check_counters, _launches
from test_prompt_score_gpu import BAR
from test_rescore_gpu import rescore
from test_rewind_gpu import LAYERS, TEXT, Hkv, Hq, D, _qkv, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

KEY, ROWS = "video_budget_rescore", "video_budget_observe_rows"
ALPHA = 0.5


class _RescoreDriver(_BudgetDriver):
    """test_budget_gpu's driver around a cache whose config also carries `top` (the re-scoring's keys, the position keys).
    token_ids: plain video ids are an arange per token (as test_position_rebase_gpu's), so that every eviction opens id gaps."""

    def __init__(self, protocol, ids, dtype, L, top=None, reserve=None, token_ids=False, **kw):
        import retake.longvideo_cache as lc

        super().__init__(protocol, ids, dtype, L, reserve=reserve, **kw)
        self.token_ids = token_ids
        cfg = self.cache.config
        cfg.longvideo_kwargs.update(top or {})
        self.cache = lc.build_kvcache(cfg, **({"reserve_tokens": reserve} if reserve else {}))


    def _video_ids(self, Lv, Lp):
        if self.mrope or not self.token_ids:
            return super()._video_ids(Lv, Lp)
        p = torch.arange(self.t_next, self.t_next + Lv, device=dev()).view(1, Lv)
        self.t_next += Lv
        return p.contiguous()


def _region(cache, l):
    """Clones of the layer's scores (this flushes), K, V, ids and observed queries."""
    sc = cache.row_scores(l)
    pos = cache.position_cache
    ids = pos[l].clone() if l < len(pos) and isinstance(pos[l], torch.Tensor) else None
    return sc, cache.key_cache[l].clone(), cache.value_cache[l].clone(), ids, cache.observed_queries(l)


def _blend_on_copies(sc, K, oq, n_old, dtype, what):
    """The blended scores of a region by the kernel run from here on copies, checked against float64 under the bar."""
    if n_old == 0:
        return sc
    Wc = oq.shape[1]
    k = K[0, :, TEXT:TEXT + n_old].contiguous()
    got = rescore([(oq, k, sc, n_old)], Hq, Hkv, Wc, D, dtype, ALPHA)[0]
    m64 = rr.mass(oq, k, n_old)
    want = rr.rescored(sc, oq, k, n_old, ALPHA).to(dev())
    err = (got.double() - want).abs()
    bar = rr.bar(ALPHA, n_old, Wc, BAR[dtype], m64, want[:n_old])
    print(f"budget rescore {what}: n_old {n_old} Wc {Wc}: max |got - float64| = {err.max().item():.3e} "
          f"({(err[:n_old] / bar).max().item():.3f} of the bar)")
    assert bool((err[:n_old] <= bar).all()), what
    assert torch.equal(got[n_old:], sc[n_old:]), (what, "rows >= n_old keep their arrival score")
    return got


def _pick(t, idx, dim):
    return t.index_select(dim, torch.cat([torch.arange(TEXT), TEXT + idx]).to(t.device))


def _simulate(protocol, ids, dtype, L, S, W=None, chunks=5, moved=False, **kw):
    """moved: the position keys may re-rotate K and shift the temporal ids after an eviction - where they did, the comparison
    is taken on what the move does not touch: V, the scores and (M-RoPE) the id rows 1 and 2, which identify the survivors."""
    keep = int(RATIO * L)
    B = keep + keep // 2
    top = dict(kw.pop("top", {}), **{KEY: ALPHA})
    if W is not None:
        top[ROWS] = W
    d = _RescoreDriver(protocol, ids, dtype, L, B=B, S=S, top=top, **kw)
    cache = d.cache
    d.step(1, TEXT)
    seen = [rr.Seen() for _ in range(LAYERS)]
    dropped, evictions, rescored = [0] * LAYERS, 0, [0] * LAYERS
    for c in range(chunks):
        d.step(2 + c, L, video=True, after_forward=False)
        d.log.clear()
        snap = [_region(cache, l) for l in range(LAYERS)]
        expect = []
        for l, (sc, K, V, pid, oq) in enumerate(snap):
            what = (protocol, ids, dtype, L, S, "chunk", c, "layer", l)
            n = sc.numel()
            assert n == K.shape[2] - TEXT and oq.shape == (Hq, min(W or 64, L), D) and oq.dtype == dtype, what
            n_old = seen[l].rescore(n)
            rescored[l] += n_old > 0
            blended = _blend_on_copies(sc, K, oq, n_old, dtype, what)
            if n > B + S:
                surv = br.survivors(blended, B)
                dropped[l] += n - B
                seen[l].evict(B)
            else:
                surv = torch.arange(n)
            expect.append((blended, surv))
        evictions += snap[0][0].numel() > B + S
        offsets = [int(cache.position_offset(l)) for l in range(LAYERS)]
        cache.after_forward()
        for l, ((sc, K, V, pid, oq), (blended, surv)) in enumerate(zip(snap, expect)):
            what = (protocol, ids, dtype, L, S, "chunk", c, "layer", l)
            _same(cache.value_cache[l], _pick(V, surv, 2), (what, "V"))
            _same(cache.row_scores(l), blended[surv.to(dev())], (what, "scores"))
            pos = cache.position_cache
            if not moved or int(cache.position_offset(l)) == offsets[l]:   # (no move at this eviction: every bit stays)
                _same(cache.key_cache[l], _pick(K, surv, 2), (what, "K"))
                if pid is not None:
                    _same(pos[l], _pick(pid, surv, pid.ndim - 1), (what, "ids"))
            elif pid is not None and pid.ndim == 3:
                _same(pos[l][1:], _pick(pid, surv, 2)[1:], (what, "ids of the h / w axes"))
        what = (protocol, ids, dtype, L, S, "chunk", c)
        assert cache.budget_rescored == rescored or (not any(rescored) and cache.budget_rescored == []), what
        _check_counters(cache, c, L, keep, [(torch.empty(min(snap[l][0].numel(), B if snap[l][0].numel() > B + S else 1 << 30)),
                                             dropped[l], evictions) for l in range(LAYERS)], what)
        assert cache.video_end is not None and cache.video_end.epoch == cache._epoch
        assert [m.sc_seen for m in cache.video_end.layers] == [s.n_old for s in seen], what
    assert evictions >= 2 and all(r == chunks - 1 for r in rescored)
    return d


@pytest.mark.parametrize("S", ["S0", "Skeep"])
@pytest.mark.parametrize("L", [64, 512])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("protocol", ["update", "pre_rope"])
def test_step_simulation(protocol, ids, dtype, L, S):
    keep = int(RATIO * L)
    _simulate(protocol, ids, dtype, L, keep if S == "Skeep" else 0, W=8 if S == "S0" else None)


@pytest.mark.parametrize("L", [64, 512])
def test_step_simulation_fp32(L):
    _simulate("update", "mrope", torch.float32, L, 0)


def test_step_simulation_without_reforge():
    _simulate("update", "mrope", torch.bfloat16, 512, 0, reforge=False)


@pytest.mark.parametrize("L,protocol", [(64, "update"), (512, "pre_rope")])
def test_step_simulation_beside_the_position_keys(L, protocol):
    """The re-scoring reads the rows before the move: same survivors, same scores, whatever the re-base does afterwards."""
    d = _simulate(protocol, "plain", torch.bfloat16, L, 0, moved=True, token_ids=True,
                  top={"video_position_limit": 0, "video_position_gap": 1})
    for l in range(LAYERS):   # limit 0, gap 1, one id per token: evictions open id gaps, so the moves did happen
        assert int(d.cache.position_offset(l)) > 0


# ---------------------------------------------------------------------------------------------------
# a heavy hitter survives: fails without the feature
# ---------------------------------------------------------------------------------------------------
def _heavy_hitter_chunk(d, seed, L, tails=None):
    """One video chunk on the `update` route, without a key-patch mask (the mask's exact ties at 1.0 go to the oldest row,
    so a tied minimum of chunk 1 would outlive chunk 2's whatever its score); tails: the last 8 ROTATED query rows of every
    head are `tails[l]` [Hq, 8, D]."""
    cache = d.cache
    pos0 = d._video_ids(L, 0)
    for l in range(LAYERS):
        q, k, v = _qkv(1000 * seed + l, L, d.dtype)
        cache.kvcache_compression = True
        pos = pos0.clone()
        cache.shift_temporal_ids_(pos, l)
        qr = synth.rope_forward(q.float(), pos, d.rot, d.sec).to(d.dtype)
        kr = synth.rope_forward(k.float(), pos, d.rot, d.sec).to(d.dtype)
        if tails is not None:
            qr[0, :, L - 8:] = tails[l]
        cache.update(kr, v, l, {"query_states": qr, "position_ids": pos, "rotary_emb": d.rot, "mrope_section": d.sec})
    cache.after_forward()
    cache.kvcache_compression = False


def test_a_heavy_hitter_survives():
    L, dtype = 64, torch.bfloat16
    keep = int(RATIO * L)
    B = keep + keep // 2
    off = _RescoreDriver("update", "mrope", dtype, L, B=B, S=0)
    on = _RescoreDriver("update", "mrope", dtype, L, B=B, S=0, top={KEY: ALPHA, ROWS: 8})
    assert off.cache.video_budget_rescore is None and on.cache.video_budget_rescore == ALPHA
    for d in (off, on):
        d.step(1, TEXT)
        _heavy_hitter_chunk(d, 2, L)
    tails, star, v_star, old = [], [], [], []
    for l in range(LAYERS):
        s = on.cache.row_scores(l)
        _same(s, off.cache.row_scores(l), ("chunk 1", l))
        j = int(torch.argmin(s))                                      # the lowest-scored region row
        k = on.cache.key_cache[l][0, :, TEXT + j]                     # [Hkv, D], rotated, as stored
        tails.append((4 * k.float()).to(dtype).repeat_interleave(Hq // Hkv, dim=0)[:, None, :].expand(Hq, 8, D))
        star.append(j)
        old.append(float(s[j]))
        v_star.append(on.cache.value_cache[l][0, :, TEXT + j].clone())
        # the logit margin that puts all mass on j*: 4 |k|^2 / sqrt(D) against 4 k . k' / sqrt(D)
        K = on.cache.key_cache[l][0, :, TEXT:TEXT + keep].double()
        logits = 4 * torch.einsum("gd,gjd->gj", k.double(), K) / D ** 0.5
        rest = torch.cat([logits[:, :j], logits[:, j + 1:]], dim=1)
        assert float((logits[:, j] - rest.max(dim=1).values).min()) > 50, l
    for d in (off, on):
        _heavy_hitter_chunk(d, 3, L, tails)
    assert on.cache.budget_rescored == [1] * LAYERS and off.cache.budget_rescored == []
    for l in range(LAYERS):
        def where(cache):
            hit = (cache.value_cache[l][0, :, TEXT:] == v_star[l][:, None, :]).all(dim=2).all(dim=0).nonzero().flatten()
            return hit.tolist()
        # the precondition, on today's behaviour: without the key j* is evicted at chunk 2
        assert where(off.cache) == [], (l, "the seed no longer evicts j* with the key off: pick another")
        at = where(on.cache)
        assert len(at) == 1, (l, "j* did not survive")
        got = float(on.cache.row_scores(l)[at[0]])
        want = 0.5 * old[l] + 0.5 * keep                              # obs = n_old: all of every query row's mass
        bar = ALPHA * (keep / 8) * BAR[dtype] * 8 + 4 * 2.0 ** -24 * want
        print(f"heavy hitter layer {l}: j* = {star[l]}, score {old[l]:.4f} -> {got:.6f} (want {want:.6f}, bar {bar:.2e})")
        assert abs(got - want) <= bar, (l, got, want)
    # everything else about chunk 2 is equal in both caches
    _same(on.cache.last_keep_indices, off.cache.last_keep_indices, "kept indices of chunk 2")
    _same(on.cache.last_scores, off.cache.last_scores, "scores of chunk 2")
    assert on.cache.num_evicted_tokens == off.cache.num_evicted_tokens and on.cache.budget_dropped == off.cache.budget_dropped


# ---------------------------------------------------------------------------------------------------
# off is off
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 512])
def test_off_is_off(L):
    keep = int(RATIO * L)
    B = keep + keep // 2
    names = ("score_pass1", "score_pass2", "keep_scores", "budget_select", "squeeze_units")

    def run(d):
        d.step(1, TEXT)
        for c in range(CHUNKS):
            d.step(2 + c, L, video=True)
        d.log.clear()

    off = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=B, top={KEY: None, ROWS: 64})
    twin = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=B)     # a config that never heard of the keys
    assert KEY in off.cache.config.longvideo_kwargs and KEY not in twin.cache.config.longvideo_kwargs
    n_off, n_twin = _launches(lambda: run(off), names), _launches(lambda: run(twin), names)
    assert n_off == n_twin                                               # nothing new is launched
    _same_state(off.cache, twin.cache, "rescore off")
    for l in range(LAYERS):
        _same(off.cache.row_scores(l), twin.cache.row_scores(l), ("scores", l))
    assert off.cache.budget_rescored == [] and off.cache.budget_dropped == twin.cache.budget_dropped
    assert all(st.oq is None and st.sc_seen == twin.cache._layers[i].sc_seen for i, st in enumerate(off.cache._layers))
    assert "observe_queries" not in off.cache.memory_footprint() and not any("rescore" in k for k in off.cache._ws)
    # with the key on: per re-scoring ONE call for both layers - the range pass and its merge, then the column pass
    on = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=B, top={KEY: ALPHA})
    n_on = _launches(lambda: run(on), names)
    calls = CHUNKS - 1
    assert n_on == (n_twin[0] + 2 * calls, n_twin[1] + calls) + n_twin[2:]
    assert on.cache.budget_rescored == [calls] * LAYERS


# ---------------------------------------------------------------------------------------------------
# marks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,protocol", [(64, "update"), (512, "pre_rope")])
def test_marks_and_questions(L, protocol):
    keep = int(RATIO * L)
    B = keep + keep // 2
    top = {KEY: ALPHA, ROWS: 16}
    a = _RescoreDriver(protocol, "mrope", torch.bfloat16, L, B=B, top=top)
    b = _RescoreDriver(protocol, "mrope", torch.bfloat16, L, B=B, top=top)     # the same stream without the question
    for d in (a, b):
        d.step(1, TEXT)
        for c in range(3):
            d.step(2 + c, L, video=True)
    assert a.cache.budget_rescored == [2] * LAYERS and a.cache.budget_dropped[0] > 0
    ve = a.cache.video_end                                               # taken after a re-scoring and an eviction: good
    assert ve is not None and ve.epoch == a.cache._epoch and ve.layers[0].sc_len == B and ve.layers[0].sc_seen == B
    before = _state(a.cache)
    scores = [a.cache.row_scores(l) for l in range(LAYERS)]
    t = a.t_next
    a.step(10, QUESTION)
    assert a.cache.get_seq_length(0) == TEXT + B + QUESTION
    a.cache.rewind(ve)
    a.t_next = t
    _same_state(a.cache, before, "after the question and the rewind")
    for l in range(LAYERS):
        _same(a.cache.row_scores(l), scores[l], ("blended scores stay after the rewind", l))
    assert [st.sc_seen for st in a.cache._layers] == [B] * LAYERS
    for c in (3, 4):
        for d in (a, b):
            d.step(2 + c, L, video=True)
        _same_state(a.cache, b.cache, ("the stream after the rewind, chunk", c))
        for l in range(LAYERS):
            _same(a.cache.row_scores(l), b.cache.row_scores(l), ("scores after the rewind, chunk", c, l))
    assert a.cache.budget_rescored == b.cache.budget_rescored == [4] * LAYERS
    # a question left in place: its rows carry no score - the layers are not rescored, the eviction raises as it always did
    a.step(11, QUESTION)
    scores = [a.cache.row_scores(l) for l in range(LAYERS)]
    epoch, done = a.cache._epoch, list(a.cache.budget_rescored)
    with pytest.raises(ValueError, match="video_end"):
        a.step(7, L, video=True)
    assert a.cache._epoch == epoch and a.cache.budget_rescored == done
    for l in range(LAYERS):
        _same(a.cache.row_scores(l)[:B], scores[l][:B], ("no blend behind a question", l))


# ---------------------------------------------------------------------------------------------------
# the plateau
# ---------------------------------------------------------------------------------------------------
def test_capacity_stops_growing():
    L, S = 64, 0
    keep = int(RATIO * L)
    B = keep + keep // 2
    a = _RescoreDriver("update", "mrope", torch.bfloat16, L, B=B, S=S, reserve=TEXT + B + S + L + QUESTION, top={KEY: ALPHA})
    a.step(1, TEXT)

    def pointers():
        out = [tuple((t.data_ptr(), tuple(t.shape)) for t in (st.k, st.v, st.pos, st.sc, st.oq) if t is not None)
               for st in a.cache._layers]
        return out + [(name, t.data_ptr(), t.numel()) for name, t in sorted(a.cache._ws.items())]

    seen = {}
    for c in range(12):
        a.step(2 + c, L, video=True)
        a.log.clear()
        if c + 1 in (4, 12):
            seen[c + 1] = (pointers(), a.cache.memory_footprint())
    assert seen[4][0] == seen[12][0]
    assert seen[4][1] == seen[12][1]
    assert seen[4][1]["observe_queries"] == LAYERS * Hq * 64 * D * 2 and any("rescore" in k for k in a.cache._ws)
    assert a.cache.budget_rescored == [11] * LAYERS and a.cache.get_seq_length(0) == TEXT + B

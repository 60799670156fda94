"""video_position_gap at cache level, on the GPU: every case is a TWIN comparison against the same bounded cache (same budget
or window) WITHOUT the keys, stepped alongside.  The rule is this project's own; the reference has no counterpart and answer
quality is not evaluated.

Shapes and driver: tests/test_position_rebase_gpu.py's (2 layers, Hq 4 / Hkv 2, D 128, 5 pinned text rows, 6 chunks), and only
its setup (a): update_pre_rope with prologue_operands="pre_rope" at L = 512, ratio 0.5 - the scores read the pre-RoPE
projections, so neither the selection nor the budget's survivors can depend on the ids and twins keep identical rows (asserted:
the kept indices and V are equal).  The bound is B (or W) = 1.5 x keep, slack 0: from the second chunk on every after_forward
moves rows.

What a renumbering is expected to do is SIMULATED from the twin: the region ids the rule predicts so far, the twin's ids of
the rows the chunk appended minus the offset so far behind them, the survivors of the move found by matching the twin's V
rows before and after it (no rule touches V), and tests/renumber_ref.py's integers on what survives.

Keys.  Rows that were in the cache before a move: rebase_ref.bar against rebase_ref.rotate(row as it was before that
after_forward, d of the row in that move) - a snapshot is taken; rows with d = 0 bit-equal.  Rows appended after a renumbering:
the bar test_position_rebase_gpu.py uses for them (rope_ref.rotate_bound against float64 at the ids stored for them)."""
import numpy as np
import pytest
import torch

import rebase_ref as rr
import renumber_ref as nr
import synth
from test_position_rebase_gpu import CHUNKS, NEVER, QUESTION, SETUPS, _check_new_rows, _ids, _np, _RebaseDriver
from test_rewind_gpu import SEC, A, D, LAYERS, TEXT, _cfg, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

KERNELS = ("rebase_decide", "rebase_apply", "renumber_scan", "renumber_apply")


class _Driver(_RebaseDriver):
    """_RebaseDriver with video_position_gap in the config of the cache under test."""

    def __init__(self, ids, dtype, bound, P=None, G=None):
        import retake.longvideo_cache as lc

        protocol, L, ratio, extra = SETUPS["a"]
        keep = int(ratio * L)
        self.keep, self.rows = keep, keep + keep // 2
        cfg = _cfg(True, False, compression_ratio=ratio, **extra)
        cfg.longvideo_kwargs.update({f"video_{bound}_rows": self.rows, f"video_{bound}_slack": 0})
        if P is not None:
            cfg.longvideo_kwargs["video_position_limit"] = P
        if G is not None:
            cfg.longvideo_kwargs["video_position_gap"] = G
        self.cache = lc.build_kvcache(cfg)
        self.protocol, self.mrope, self.dtype, self.L, self.prompt = protocol, ids == "mrope", dtype, L, 0
        self.sec = SEC if self.mrope else None
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.t_next = 0
        self.log = []


def _launches(fn):
    """Launch counts of the four kernels while fn runs, through the profile mask."""
    import retake._native as nv

    kids = nv.profile_kernel_ids()
    nv.lib.rtk_profile_reset()
    mask = 0
    for k in KERNELS:
        mask |= 1 << kids[k]
    nv.lib.rtk_profile_enable_mask(mask)
    try:
        fn()
        got = nv.profile_read()
        return tuple(got.get(k, (0, 0.0))[0] for k in KERNELS)
    finally:
        nv.lib.rtk_profile_enable(0)
        nv.lib.rtk_profile_reset()


def _rows_as_bytes(v):
    """[1, H, n, D] -> n byte strings, a row over all heads."""
    x = v[0].transpose(0, 1).contiguous().cpu()
    x = x.view(torch.int32 if x.dtype == torch.float32 else torch.int16).numpy().reshape(x.shape[0], -1)
    return [r.tobytes() for r in x]


def _survivors(v_pre, v_post):
    """Indices into the rows before the move of the rows after it, matched through V."""
    at = {}
    for i, r in enumerate(_rows_as_bytes(v_pre)):
        assert at.setdefault(r, i) == i, "two equal V rows: the inputs cannot tell the survivors"
    out = np.array([at[r] for r in _rows_as_bytes(v_post)])
    assert np.all(np.diff(out) > 0)
    return out


def _run(ids, dtype, bound, P, G, patches=False, chunks=CHUNKS, check_new_rows=True):
    """The cache under test (limit P, gap G) beside its twin without the keys -> (driver, twin, totals per chunk and layer)."""
    w, u = _Driver(ids, dtype, bound, P=P, G=G), _Driver(ids, dtype, bound)
    for d in (w, u):
        d.step(1, TEXT)
    off = [0] * LAYERS
    sim = [np.zeros(0, dtype=np.int64) for _ in range(LAYERS)]      # the region ids the rule predicts
    inv = synth.inv_freq(D)
    pshape = 3 if ids == "mrope" else 1
    dtype_name = str(dtype).split(".")[-1]
    on = torch.from_numpy(np.concatenate([rr.temporal_pairs(D, pshape, w.sec)] * 2))
    totals = []
    for c in range(chunks):
        seed = 2 + c
        for d in (w, u):
            if patches:      # every row of the chunk is a key patch: it scores 1.0
                d.cache.keypatches_mask_chunk = torch.ones(d.L, dtype=torch.bool, device=dev())
            d.step(seed, d.L, video=True, after_forward=False)
            d.cache.keypatches_mask_chunk = None
        pre = []
        for l in range(LAYERS):      # (reading the caches flushes: the chunk's kept rows are in place, nothing has moved)
            pre.append((w.cache.key_cache[l].clone(), _ids(w.cache, l), u.cache.value_cache[l].clone(), _ids(u.cache, l)))
            bw, bu = w.cache._batch, u.cache._batch
            assert torch.equal(bw.keep_idx[bw.slot(l)], bu.keep_idx[bu.slot(l)]), ("kept indices differ", c, l)
        moves = c >= 1
        counts = _launches(w.cache.after_forward)
        assert counts == ((0, 0, 1, 1) if moves else (0, 0, 0, 0)), (c, counts)      # one scan + one apply per move, no re-base
        u.cache.after_forward()
        w.cache.kvcache_compression = u.cache.kvcache_compression = False
        row = []
        for l in range(LAYERS):
            what = (ids, dtype, bound, P, G, "chunk", c, "layer", l)
            k_pre, ids_pre, v_pre_u, ids_pre_u = pre[l]
            if check_new_rows and off[l]:
                _check_new_rows("a", w, seed, l, k_pre, ids_pre, what)
            # the simulation, from the twin alone
            sim_pre = np.concatenate([sim[l], ids_pre_u[0, -w.keep:].numpy() - off[l]])
            surv = _survivors(v_pre_u, u.cache.value_cache[l])
            assert surv[:TEXT].tolist() == list(range(TEXT)) and len(surv) == TEXT + (w.rows if moves else len(sim_pre)), what
            s = sim_pre[surv[TEXT:] - TEXT]
            dl, total = np.zeros(len(s), dtype=np.int64), 0
            if moves:
                dl, total = nr.decide(np.concatenate([ids_pre_u[0, :TEXT].numpy(), s]), TEXT, TEXT + len(s), P, G)
            sim[l] = s - dl
            off[l] += total
            row.append(total)
            # ids
            got, tw = _ids(w.cache, l), _ids(u.cache, l)
            assert torch.equal(got[:, :TEXT], tw[:, :TEXT]) and torch.equal(got[1:], tw[1:]), (what, "pinned ids / id rows 1 - 2")
            assert np.array_equal(got[0, TEXT:].numpy(), sim[l]), (what, "ids != renumber_ref on the simulated ids")
            diff = (tw[0, TEXT:] - got[0, TEXT:]).numpy()
            assert np.all(diff >= 0) and np.all(np.diff(diff) >= 0), (what, "twin - cache is not a non-decreasing delta")
            assert int(diff[-1]) == off[l] == int(w.cache.position_offset(l)), (what, "offset", int(diff[-1]), off[l])
            assert int(w.cache.get_prev_temporal_idx(l)) == int(u.cache.get_prev_temporal_idx(l)) - off[l], what
            # V and keys
            kw = w.cache.key_cache[l]
            _same(w.cache.value_cache[l], u.cache.value_cache[l], (what, "V"))
            _same(kw[:, :, :TEXT], k_pre[:, :, :TEXT], (what, "pinned K"))
            src = k_pre[0][:, torch.from_numpy(surv[TEXT:])]
            new = kw[0, :, TEXT:]
            still = torch.from_numpy(dl == 0)
            _same(new[:, still], src[:, still], (what, "rows with d = 0"))
            _same(new[..., ~on], src[..., ~on], (what, "non-temporal channels"))
            for v in np.unique(dl[dl > 0]):
                at = torch.from_numpy(dl == v)
                x = _np(src[:, at])
                ref = rr.rotate(x, int(v), inv, pshape, w.sec)
                err, bar = np.abs(_np(new[:, at]) - ref), rr.bar(dtype_name, ref, x)
                assert np.all(err <= bar), (what, "d", int(v), "worst error / bar", float((err / bar).max()))
        totals.append(row)
        assert w.cache.video_end is not None and w.cache.video_end.epoch == w.cache._epoch
        w.log.clear()
        u.log.clear()
    return w, u, totals


# ---------------------------------------------------------------------------------------------------
# 1. the case the key is for: under the budget the uniform rule never triggers
# ---------------------------------------------------------------------------------------------------
def test_the_budget_keeps_an_old_row_and_only_the_gap_rule_bounds_the_ids():
    """The first region row carries a key-patch mask bit, so it scores 1.0 and survives every eviction: the region's first
    id stays right behind the pinned rows.  (A score averages 1 over a chunk, so a bit on that row alone does not do it - rows
    of later chunks outscore 1.0, measured: the row was evicted.  Here EVERY row of every chunk is a key patch: all scores tie
    at 1.0 and the budget's ties go to the oldest, so the region is its oldest B - 1 rows and the newest one, with one hole in
    front of the newest row that grows with every chunk.)  With video_position_limit = 0 alone the uniform delta is 0 at every
    move - position_offset stays 0 and the last id grows like the unbounded run's (past the span bound in these six
    chunks); with video_position_gap = 1 the last id stays within the span bound 1 + (B - 1) G behind the pinned rows after
    every move."""
    G = 1
    w, u, totals = _run("plain", torch.bfloat16, "budget", 0, G, patches=True, check_new_rows=False)
    only_limit = _Driver("plain", torch.bfloat16, "budget", P=0)
    only_limit.step(1, TEXT)
    for c in range(CHUNKS):
        only_limit.cache.keypatches_mask_chunk = torch.ones(only_limit.L, dtype=torch.bool, device=dev())
        only_limit.step(2 + c, only_limit.L, video=True)
        only_limit.cache.keypatches_mask_chunk = None
        only_limit.log.clear()
    for l in range(LAYERS):
        t_u, t_l, t_w = _ids(u.cache, l)[0], _ids(only_limit.cache, l)[0], _ids(w.cache, l)[0]
        assert int(t_u[TEXT]) == TEXT, "the first region row did not survive: the construction does not hold"
        assert int(only_limit.cache.position_offset(l)) == 0 and torch.equal(t_l, t_u)      # the uniform rule never triggered
        assert int(t_l[-1]) > TEXT + (w.rows - 1) * G                                           # ... and its last id left the span
        assert all(row[l] > 0 for row in totals[1:]), totals
        assert int(w.cache.position_offset(l)) > 0
        assert int(t_w[-1]) <= TEXT + (w.rows - 1) * G, (int(t_w[-1]), "the span bound")
        assert int(t_w[-1]) + int(w.cache.position_offset(l)) == int(t_u[-1])                    # the newest row: stored + offset


# ---------------------------------------------------------------------------------------------------
# 2. / 3. the twin runs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound,ids,dtype,P,G,least", [
    ("budget", "plain", torch.bfloat16, 0, 2, 2),
    ("budget", "plain", torch.bfloat16, 950, 2, 2),       # some moves trigger, some do not
    ("budget", "mrope", torch.bfloat16, 0, 1, 0),      # (64 rows an id: a gap opens only where a whole frame goes)
    ("window", "plain", torch.bfloat16, 0, 2, 2),
    ("window", "mrope", torch.bfloat16, 0, 1, 2),
    ("budget", "plain", torch.float32, 0, 4, 2),
    ("window", "mrope", torch.float32, 0, 1, 2),
], ids=["budget-plain", "budget-plain-P950", "budget-mrope", "window-plain", "window-mrope", "budget-plain-fp32",
        "window-mrope-fp32"])
def test_twin_run(bound, ids, dtype, P, G, least):
    w, u, totals = _run(ids, dtype, bound, P, G)
    counts = [sum(1 for row in totals if row[l] > 0) for l in range(LAYERS)]
    assert all(n >= least for n in counts), totals
    if P:
        assert all(n < CHUNKS - 1 for n in counts), totals
    print(f"renumberings per layer: {counts}, totals {totals}, offsets {[int(w.cache.position_offset(l)) for l in range(LAYERS)]}")


# ---------------------------------------------------------------------------------------------------
# 4. nothing triggers; marks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", ["budget", "window"])
def test_a_limit_no_id_reaches_is_the_cache_without_the_gap(bound):
    w, u, totals = _run("plain", torch.bfloat16, bound, NEVER, 2, chunks=4)
    assert all(t == 0 for row in totals for t in row)
    only_limit = _Driver("plain", torch.bfloat16, bound, P=NEVER)
    only_limit.step(1, TEXT)
    for c in range(4):
        only_limit.step(2 + c, only_limit.L, video=True)
        only_limit.log.clear()
    _same_state(w.cache, only_limit.cache, "no trigger: the whole state is that of the cache without the gap")
    _same_state(w.cache, u.cache, "... and of the cache without either key")
    assert [int(w.cache.position_offset(l)) for l in range(LAYERS)] == [0] * LAYERS
    assert w.cache._epoch == only_limit.cache._epoch == u.cache._epoch


def test_marks_across_a_renumbering():
    a = _Driver("plain", torch.bfloat16, "budget", P=0, G=1)
    a.step(1, TEXT)
    a.step(2, a.L, video=True)
    early, old_end = a.cache.mark(), a.cache.video_end
    a.step(3, a.L, video=True)
    a.step(4, a.L, video=True)
    assert int(a.cache.position_offset(0)) > 0
    before = _state(a.cache)
    for m in (early, old_end):
        with pytest.raises(ValueError, match="rewritten wholesale"):
            a.cache.rewind(m)
    _same_state(a.cache, before, "a mark from before the renumbering")
    ve = a.cache.video_end
    assert ve is not None and ve.epoch == a.cache._epoch
    t = a.t_next
    a.step(10, QUESTION)
    assert a.cache.get_seq_length(0) == TEXT + a.rows + QUESTION
    a.cache.rewind(ve)
    a.t_next = t
    _same_state(a.cache, before, "after the question and the rewind")
    a.step(5, a.L, video=True)                   # the stream goes on
    # P = 0, G = 1: the region follows the pinned rows and every step is 0 (reforged ids repeat) or 1
    t = _ids(a.cache, 0)[0].numpy()
    assert int(t[TEXT]) == TEXT and set(np.diff(t[TEXT:]).tolist()) <= {0, 1}
    assert int(a.cache.get_prev_temporal_idx(0)) == int(t[-1]) <= TEXT + a.rows - 1


# ---------------------------------------------------------------------------------------------------
# 5. launches
# ---------------------------------------------------------------------------------------------------
def test_keys_off_launch_nothing_and_the_limit_alone_launches_the_rebase():
    for P, want in ((None, (0, 0, 0, 0)), (0, (2, 2, 0, 0))):
        d = _Driver("plain", torch.bfloat16, "budget", P=P)
        d.step(1, TEXT)

        def run():
            for c in range(3):
                d.step(2 + c, d.L, video=True)

        assert _launches(run) == want, P
    assert d.cache.video_position_gap is None

"""video_position_limit at cache level, on the GPU: every case is a TWIN comparison against the same bounded cache (same
window or budget) WITHOUT the key.  The rule is this project's own; the reference has no counterpart.

Shapes: 2 layers, Hq 4 / Hkv 2, D 128 (the driver of tests/test_rewind_gpu.py), 5 pinned text rows, 6 chunks.  Plain ids are an
arange per token (LLaVA style), M-RoPE ids are that driver's.  Only setups in which the selection cannot depend on the ids are
used, so twins keep identical rows by construction (asserted: the kept indices are equal):
  (a) update_pre_rope with prologue_operands="pre_rope" at L = 512, ratio 0.5 - the scores read the pre-RoPE projections;
  (b) the `update` protocol at L = 64, ratio 1.0 - every row is kept.
The bound is W (or B) = 1.5 x keep, slack 0: from the second chunk on every after_forward moves rows.

What a re-base is expected to do is computed from the TWIN's ids with the rule restated in tests/rebase_ref.py (integers):
after every move, delta = decide(twin ids - offset so far).  Limits: one found by simulating that rule on the twin's ids so
that exactly two re-bases happen, one so high that none does, and 0.

Bars.  Rows that were in the cache before a re-base: the kernel test's bar, rebase_ref.bar, against rebase_ref.rotate of the
rows as they were before that re-base (for the first re-base those ARE the twin's rows, bit for bit - asserted).  Rows
appended after a re-base: the bar the project already uses for re-rotated keys against float64, rope_ref.rotate_bound
(tests/rope_ref.py: 4 u (|x1 cos| + |x2 sin|), 6 u in fp32, plus a subnormal), against rope_ref.rotate_truth of the pre-RoPE
projections at the ids the cache stored for them - setup (a), where the kept key is one rotation of the projection.  In setup
(b) the kept key is the caller's rotation (1 rounding), the un-rotation (5: table, two products, sum, division) and the
re-rotation (4): the same accounting gives 10 u."""
import numpy as np
import pytest
import torch

import rebase_ref as rr
import rope_ref
import synth
from test_rewind_gpu import SEC, A, D, LAYERS, TEXT, _cfg, _Driver, _qkv, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

CHUNKS, QUESTION = 6, 7
SETUPS = {"a": ("pre_rope", 512, 0.5, {"prologue_operands": "pre_rope"}), "b": ("update", 64, 1.0, {})}
NEVER = 10 ** 9


class _RebaseDriver(_Driver):
    """test_rewind_gpu's driver around ONE cache built from a config that carries the bound and, for the cache under test,
    video_position_limit; plain video ids are an arange per token."""

    def __init__(self, setup, ids, dtype, bound="window", P=None):
        import retake.longvideo_cache as lc

        protocol, L, ratio, extra = SETUPS[setup]
        keep = int(ratio * L)
        self.keep, self.rows = keep, keep + keep // 2
        cfg = _cfg(True, False, compression_ratio=ratio, **extra)
        cfg.longvideo_kwargs.update({f"video_{bound}_rows": self.rows, f"video_{bound}_slack": 0})
        if P is not None:
            cfg.longvideo_kwargs["video_position_limit"] = P
        self.cache = lc.build_kvcache(cfg)
        self.protocol, self.mrope, self.dtype, self.L, self.prompt = protocol, ids == "mrope", dtype, L, 0
        self.sec = SEC if self.mrope else None
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.t_next = 0
        self.log = []

    def _video_ids(self, Lv, Lp):
        if self.mrope:
            return super()._video_ids(Lv, Lp)
        p = torch.arange(self.t_next, self.t_next + Lv, device=dev()).view(1, Lv)
        self.t_next += Lv
        return p.contiguous()


def _ids(cache, l):
    """The layer's stored ids as [P, n] on the host."""
    p = cache.position_cache[l]
    return p.reshape(p.shape[0], p.shape[-1]).cpu()


def _run_twin(setup, ids, dtype, bound):
    """The bounded cache without the key: per chunk, per layer its ids after the chunk's after_forward, and the driver."""
    u = _RebaseDriver(setup, ids, dtype, bound)
    u.step(1, TEXT)
    trace = []
    for c in range(CHUNKS):
        u.step(2 + c, u.L, video=True)
        u.log.clear()
        trace.append([_ids(u.cache, l) for l in range(LAYERS)])
    return u, trace


def _simulate(trace, P):
    """The rule on the twin's ids: per chunk and layer the delta a cache with limit P applies (moves: every chunk but the first)."""
    off = [0] * LAYERS
    out = []
    for c, layers in enumerate(trace):
        row = []
        for l, ids in enumerate(layers):
            t = ids[0].numpy().copy()
            t[TEXT:] -= off[l]
            d = rr.decide(t, TEXT, len(t), P) if c >= 1 else 0
            off[l] += d
            row.append(d)
        out.append(row)
    return out


def _limit_for_two(trace):
    lasts = sorted({int(ids[0][-1]) + k for layers in trace for ids in layers for k in (0, 1)}, reverse=True)
    for P in lasts:
        sim = _simulate(trace, P)
        if all(sum(1 for row in sim if row[l] > 0) == 2 for l in range(LAYERS)):
            return P
    raise AssertionError("no limit gives exactly two re-bases on these ids")


def _rebase_launches(fn):
    import retake._native as nv

    kids = nv.profile_kernel_ids()
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable_mask((1 << kids["rebase_decide"]) | (1 << kids["rebase_apply"]))
    try:
        fn()
        got = nv.profile_read()
        return got.get("rebase_decide", (0, 0.0))[0], got.get("rebase_apply", (0, 0.0))[0]
    finally:
        nv.lib.rtk_profile_enable(0)
        nv.lib.rtk_profile_reset()


def _np(t):
    return t.double().cpu().numpy()


def _check_new_rows(setup, d, seed, l, k_pre, ids_pre, what):
    """The chunk's kept rows as the flush stored them (before the move) against float64 at the ids stored for them."""
    keep, L = d.keep, d.L
    k0 = _qkv(1000 * seed + l, L, d.dtype)[1][0].cpu()                      # [Hkv, L, D] pre-RoPE
    b = d.cache._batch
    idx = b.keep_idx[b.slot(l)].cpu()
    ang = rope_ref.angles(ids_pre[:, -keep:].numpy(), synth.inv_freq(D), D, d.sec)
    truth, mag = rope_ref.rotate_truth(k0[:, idx], ang, A)
    u = rope_ref.UNIT_ROUNDOFF[d.dtype]
    if setup == "a":
        bound = rope_ref.rotate_bound(d.dtype, mag)
    else:   # the round trip of the `update` protocol: 1 + 5 + 4 roundings, on the full magnitude A (|x1| + |x2|)
        x = np.abs(_np(k0[:, idx]))
        m = A * (x[..., :D // 2] + x[..., D // 2:])
        bound = 10.0 * u * np.concatenate([m, m], axis=-1) + rope_ref.SUBNORMAL[d.dtype]
    err = np.abs(_np(k_pre[0, :, -keep:]) - truth)
    assert np.all(err <= bound), (what, "appended rows: worst error / bar", float((err / bound).max()))


def _run(setup, ids, dtype, P, bound="window"):
    """The cache under test beside its twin; returns (driver, twin, deltas per chunk and layer)."""
    u, trace = _run_twin(setup, ids, dtype, bound)
    if P == "two":
        P = _limit_for_two(trace)
    sim = _simulate(trace, P)
    w = _RebaseDriver(setup, ids, dtype, bound, P=P)
    u2 = _RebaseDriver(setup, ids, dtype, bound)        # a second twin, stepped alongside: its rows after each move
    for d in (w, u2):
        d.step(1, TEXT)
    off = [0] * LAYERS
    arrive = [0] * LAYERS
    inv = synth.inv_freq(D)
    pshape = 3 if ids == "mrope" else 1
    for c in range(CHUNKS):
        seed = 2 + c
        u2.step(seed, u2.L, video=True)
        w.step(seed, w.L, video=True, after_forward=False)
        pre = []
        for l in range(LAYERS):
            bw, bu = w.cache._batch, u2.cache._batch
            k_pre = w.cache.key_cache[l].clone()         # (flushes: the chunk's kept rows are in place, nothing has moved)
            assert torch.equal(bw.keep_idx[bw.slot(l)], bu.keep_idx[bu.slot(l)]), ("kept indices differ", c, l)
            pre.append((k_pre, _ids(w.cache, l)))
        assert torch.equal(w.cache.last_keep_indices, u2.cache.last_keep_indices), ("kept indices differ", c)
        launches = _rebase_launches(w.cache.after_forward)
        assert launches == ((1, 1) if c >= 1 else (0, 0)), (c, launches)     # one call per move, none without a move
        w.cache.kvcache_compression = False
        for l in range(LAYERS):
            what = (setup, ids, dtype, P, bound, "chunk", c, "layer", l)
            k_pre, ids_pre = pre[l]
            if off[l]:
                _check_new_rows(setup, w, seed, l, k_pre, ids_pre, what)
            tw = trace[c][l]
            assert torch.equal(_ids(u2.cache, l), tw), what
            delta = sim[c][l]
            off[l] += delta
            got = _ids(w.cache, l)
            n = got.shape[1] - TEXT
            assert int(w.cache.position_offset(l)) == off[l], (what, "offset")
            want = tw.clone()
            want[0, TEXT:] -= off[l]
            assert torch.equal(got, want), (what, "ids = the twin's - offset; rows 1 - 2 and the pinned ids equal")
            assert int(w.cache.get_prev_temporal_idx(l)) == int(u2.cache.get_prev_temporal_idx(l)) - off[l], what
            kw, ku = w.cache.key_cache[l], u2.cache.key_cache[l]
            _same(w.cache.value_cache[l], u2.cache.value_cache[l], (what, "V"))
            _same(kw[:, :, :TEXT], ku[:, :, :TEXT], (what, "pinned K"))
            assert kw.shape == ku.shape and kw.shape[2] == TEXT + n
            if off[l] == 0:
                _same(kw, ku, (what, "no re-base so far: K is the twin's"))
                continue
            if bound == "window":        # the move is [pinned | last n rows] of what the layer held
                src = torch.cat([k_pre[:, :, :TEXT], k_pre[:, :, k_pre.shape[2] - n:]], dim=2)
            elif off[l] == delta:        # the budget's survivors: the twin's rows, equal to this cache's until its first re-base
                src = ku
            else:
                src = None
            if delta == 0 and src is not None:
                _same(kw, src, (what, "a move without a re-base only moves"))
            elif src is not None:
                ref = rr.rotate(_np(src[0, :, TEXT:]), delta, inv, pshape, w.sec)
                err = np.abs(_np(kw[0, :, TEXT:]) - ref)
                bar = rr.bar(str(dtype).split(".")[-1], ref, _np(src[0, :, TEXT:]))
                assert np.all(err <= bar), (what, "re-based rows: worst error / bar", float((err / bar).max()))
                on = torch.from_numpy(np.concatenate([rr.temporal_pairs(D, pshape, w.sec)] * 2))
                _same(kw[0, :, TEXT:][..., ~on], src[0, :, TEXT:][..., ~on], (what, "non-temporal channels"))
            # after a move the region is below the limit, or dense behind the pinned rows
            t = got[0]
            if c >= 1:
                assert int(t[-1]) < P or int(t[TEXT]) <= int(t[TEXT - 1]) + 1, (what, "neither below the limit nor re-based")
        assert w.cache.video_end is not None and w.cache.video_end.epoch == w.cache._epoch
        w.log.clear()
        u2.log.clear()
    _same_state(u2.cache, u.cache, "the two twins")
    return w, u2, sim, P


# ---------------------------------------------------------------------------------------------------
# 1. the twin runs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ["two", 0], ids=["two_rebases", "P0"])
@pytest.mark.parametrize("ids", ["plain", "mrope"])
@pytest.mark.parametrize("setup", ["a", "b"])
def test_twin_run(setup, ids, P):
    w, u, sim, P = _run(setup, ids, torch.bfloat16, P)
    counts = [sum(1 for row in sim if row[l] > 0) for l in range(LAYERS)]
    if P != 0:
        assert counts == [2] * LAYERS, counts
    else:
        assert all(n >= 3 for n in counts), counts      # P = 0: wherever a move leaves a gap
    print(f"re-bases per layer: {counts}, limit {P}, offsets {[int(w.cache.position_offset(l)) for l in range(LAYERS)]}")


@pytest.mark.parametrize("setup,ids", [("a", "plain"), ("b", "mrope")])
def test_a_limit_no_id_reaches_changes_nothing(setup, ids):
    w, u, sim, _ = _run(setup, ids, torch.bfloat16, NEVER)
    assert all(d == 0 for row in sim for d in row)
    _same_state(w.cache, u.cache, "no trigger: the whole state is the twin's")
    assert [int(w.cache.position_offset(l)) for l in range(LAYERS)] == [0] * LAYERS
    assert w.cache._epoch == u.cache._epoch and w.cache.window_dropped == u.cache.window_dropped


def test_twin_run_fp32():
    _, _, sim, _ = _run("a", "plain", torch.float32, "two")
    assert [sum(1 for row in sim if row[l] > 0) for l in range(LAYERS)] == [2] * LAYERS


def test_twin_run_under_the_budget():
    w, _, sim, _ = _run("a", "plain", torch.bfloat16, 0, bound="budget")
    assert any(d > 0 for row in sim for d in row)
    assert w.cache.budget_dropped[0] > 0


def test_the_last_id_stays_bounded():
    """Plain ids, setup (a): a chunk brings `keep` ids (256) and every after_forward from the second chunk on moves, so with
    the limit P the stored last id stays below P + keep: it is below P after a move, or the region has just been re-based to
    span pinned + W ids (which the chosen P exceeds)."""
    w, u, _, P = _run("a", "plain", torch.bfloat16, "two")
    assert P > TEXT + w.rows
    for extra in range(4):
        for d in (w, u):
            d.step(20 + extra, d.L, video=True)
            d.log.clear()
        for l in range(LAYERS):
            assert int(w.cache.get_prev_temporal_idx(l)) < P + w.keep, (extra, l)
    assert int(u.cache.get_prev_temporal_idx(0)) > P + w.keep      # the twin's ids went on growing


# ---------------------------------------------------------------------------------------------------
# 2. marks
# ---------------------------------------------------------------------------------------------------
def test_marks_across_a_rebase():
    a = _RebaseDriver("b", "plain", torch.bfloat16, P=0)
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
    _same_state(a.cache, before, "a mark from before the re-base")
    ve = a.cache.video_end
    assert ve is not None and ve.epoch == a.cache._epoch
    t = a.t_next
    a.step(10, QUESTION)
    assert a.cache.get_seq_length(0) == TEXT + a.rows + QUESTION
    a.cache.rewind(ve)
    a.t_next = t
    _same_state(a.cache, before, "after the question and the rewind")
    a.step(5, a.L, video=True)                   # the stream goes on
    assert int(a.cache.get_prev_temporal_idx(0)) == TEXT + a.rows - 1      # P = 0, plain ids: id = position in cache


def test_rows_behind_the_region_move_with_it():
    """A question left in place under the window: its 16-bit rows lie behind the video rows, the slide moves them, and the
    re-base shifts their ids and re-rotates their keys with the region's."""
    w, u = _RebaseDriver("b", "plain", torch.bfloat16, P=0), _RebaseDriver("b", "plain", torch.bfloat16)
    for d in (w, u):
        d.step(1, TEXT)
        d.step(2, d.L, video=True)
        d.step(3, d.L, video=True)
        d.step(10, QUESTION)
        d.log.clear()
    off0 = [int(w.cache.position_offset(l)) for l in range(LAYERS)]
    assert all(o > 0 for o in off0)
    u.step(4, u.L, video=True)
    w.step(4, w.L, video=True, after_forward=False)
    pre = [w.cache.key_cache[l].clone() for l in range(LAYERS)]
    w.cache.after_forward()
    w.cache.kvcache_compression = False
    inv = synth.inv_freq(D)
    for l in range(LAYERS):
        tw, got = _ids(u.cache, l), _ids(w.cache, l)
        n = got.shape[1] - TEXT
        assert n == w.rows
        off = int(w.cache.position_offset(l))
        delta = off - off0[l]
        t = tw[0].clone()
        t[TEXT:] -= off0[l]
        assert delta == rr.decide(t.numpy(), TEXT, tw.shape[1], 0) > 0
        want = tw.clone()
        want[0, TEXT:] -= off
        assert torch.equal(got, want), l
        _same(w.cache.value_cache[l], u.cache.value_cache[l], ("V", l))
        kw, src = w.cache.key_cache[l], pre[l][:, :, pre[l].shape[2] - n:]
        _same(kw[:, :, :TEXT], pre[l][:, :, :TEXT], ("pinned K", l))
        ref = rr.rotate(_np(src[0]), delta, inv)
        assert np.all(np.abs(_np(kw[0, :, TEXT:]) - ref) <= rr.bar("bfloat16", ref, _np(src[0]))), l
    # the question's rows are among the moved ones: the window holds [.. video | question | video] and dropped from the front
    assert w.cache.get_seq_length(0) == TEXT + w.rows


def test_key_off_launches_nothing():
    u = _RebaseDriver("b", "plain", torch.bfloat16)
    u.step(1, TEXT)

    def run():
        for c in range(3):
            u.step(2 + c, u.L, video=True)

    assert _rebase_launches(run) == (0, 0)
    assert int(u.cache.position_offset(0)) == 0 and u.cache._position_offsets == {}

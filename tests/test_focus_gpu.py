"""PivotKVCache.watch_question / focus at cache level, on the stand-in modules the other cache tests use (tests/synth.py).

Geometry: 2 layers, D 128, Hq 4 / Hkv 2 and Hq 7 / Hkv 1, 8 pinned text rows, chunks of L = 256 at ratio 0.25 (64 kept rows a
chunk), 5 chunks (n = 320: one key range of the re-scoring, masked) and 10 chunks (n = 640: two ranges, the merge runs), a
question of 12 rows watched with watch_question(8) (Wc = 8) and watch_question(64) (Wc = 12), keep_rows 96.  A budget parent
holds video_budget_rows = n - 32 and has evicted once (at its last chunk), so its region holds n - 32 rows with id holes.

The prefilled parents are made once per (ids, dtype, heads, chunks, budget) and shared: `focus` does not write its parent -
which check 4 verifies - and every test begins by rewinding the parent to `video_end` and disarming it.  Tests that write a
parent's rows (the planted key) or move its `video_end` build their own."""
import functools
import types

import pytest
import torch

import attention_ref as ar
import budget_ref as br
import rescore_ref as rr
import synth
from test_prompt_score_gpu import BAR
from test_rewind_gpu import A, SEC, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

LAYERS, D, RATIO, L, TEXT, QUESTION, KEEP = 2, 128, 0.25, 256, 8, 12, 96
KEPT = int(RATIO * L)
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]
# heads, chunks, watch rows: every value of the three appears in the full parametrisation, the other pairings once below
SHAPES = {"Hq4-n320-w8": (4, 2, 5, 8), "Hq7-n640-w64": (7, 1, 10, 64)}
MIXED = {"Hq4-n640-w64": (4, 2, 10, 64), "Hq7-n320-w8": (7, 1, 5, 8)}


@functools.lru_cache(maxsize=None)
def _qkv(seed, n, dtype, Hq, Hkv):
    """Pre-RoPE projections of one (step, layer) in the projection layout; shared, nothing writes them."""
    return tuple(torch.from_numpy(x).to(dev()).to(dtype).transpose(1, 2).contiguous().transpose(1, 2)
                 for x in synth.qkv_chunk(seed, Hq, Hkv, n, D))


class _Drv:
    """One parent cache and the calls the attention patches make, layer by layer, on it or on a cache focused from it.
    route "update": ids shifted by the continuity rule, q / k rotated, `update` with query_states in cache_kwargs;
    "pre_rope": `append_pre_rope`, which must take the segment.  Video chunks of 256 rows go through `update` (the
    one-call prologue serves chunks from 512 rows on)."""

    def __init__(self, ids, dtype, Hq, Hkv, B=None, **top):
        import retake.longvideo_cache as lc

        kw = {"compression_ratio": RATIO, "compression_method": "pivotkv", "pos_embed_reforge": True}
        top = dict({"kvcache_compression": True, "kvcache_compression_kwargs": kw}, **top)
        if dtype is not torch.float32:               # (the native attention serves 16-bit rows)
            top["attention_kernel"] = "hip"
        if B is not None:
            top.update(video_budget_rows=B, video_budget_slack=0)
        cfg = types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq,
                                    num_key_value_heads=Hkv, longvideo_kwargs=top)
        self.cache = lc.build_kvcache(cfg)
        self.mrope, self.dtype, self.Hq, self.Hkv = ids == "mrope", dtype, Hq, Hkv
        self.sec = SEC if self.mrope else None
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.t_next = 0

    def text_ids(self, n):
        p = torch.arange(self.t_next, self.t_next + n, device=dev()).view(1, 1, n)
        self.t_next += n
        return p.expand(3, 1, n).contiguous() if self.mrope else p[0].contiguous()

    def video_ids(self, n):
        g = n // 64
        p = torch.from_numpy(synth.mrope_position_ids(self.t_next, g, 8, 8, hw0=self.t_next)).to(dev())
        self.t_next += g
        return p.contiguous() if self.mrope else p[0].contiguous()

    def feed(self, cache, seed, pos, route="update", video=False, queries=None, with_queries=True, layers=range(LAYERS)):
        """One forward of pos.shape[-1] rows -> [(rotated q, K view, V view)] per layer.  queries[l] [Hq, w, D]: the last w
        ROTATED query rows of layer l are replaced by them (route "update")."""
        n, outs = pos.shape[-1], []
        for l in layers:
            q, k, v = _qkv(1000 * seed + l, n, self.dtype, self.Hq, self.Hkv)
            cache.kvcache_compression = video
            p = pos.clone()
            if route == "pre_rope" and not video:
                out = cache.append_pre_rope(q.clone(), k, v, l, p, self.rot, self.sec)
                assert out is not None, "append_pre_rope declined the segment"
            else:
                cache.shift_temporal_ids_(p, l)
                qr = synth.rope_forward(q.float(), p, self.rot, self.sec).to(q.dtype)
                kr = synth.rope_forward(k.float(), p, self.rot, self.sec).to(q.dtype)
                if queries is not None:
                    qr[0, :, n - queries[l].shape[1]:] = queries[l]
                kw = {"position_ids": p, "rotary_emb": self.rot, "mrope_section": self.sec}
                if with_queries:
                    kw["query_states"] = qr
                out = (qr,) + tuple(cache.update(kr, v, l, kw))
            outs.append(out)
        try:
            if video:
                cache.after_forward()
        finally:
            cache.kvcache_compression = False
        return outs

    def prefill(self, chunks):
        self.feed(self.cache, 1, self.text_ids(TEXT))
        for c in range(chunks):
            self.feed(self.cache, 2 + c, self.video_ids(L), video=True)
        self.t_video = self.t_next
        return self

    def fresh(self):
        """Back to the end of the video, disarmed."""
        self.cache.unwatch_question()
        self.cache.rewind(self.cache.video_end)
        self.t_next = self.t_video
        return self

    def ask(self, route, watch, seed=50, **kw):
        self.cache.watch_question(watch)
        return self.feed(self.cache, seed, self.text_ids(QUESTION), route, **kw)


def _build(ids, dtype, Hq, Hkv, chunks, budget, **top):
    d = _Drv(ids, dtype, Hq, Hkv, chunks * KEPT - 32 if budget else None, **top).prefill(chunks)
    n = chunks * KEPT - (32 if budget else 0)
    assert d.cache.get_seq_length(0) == TEXT + n and (d.cache.budget_dropped == [32] * LAYERS if budget else True)
    return d


@functools.lru_cache(maxsize=None)
def _shared(ids, dtype, Hq, Hkv, chunks, budget):
    return _build(ids, dtype, Hq, Hkv, chunks, budget)


def _parent(*key):
    return _shared(*key).fresh()


def _geometry(cache, l):
    """(first, ve, n, length) of a parent's layer."""
    st = cache._layers[l]
    ve = cache.video_end.layers[l].length
    return st.pinned, ve, ve - st.pinned, st.c.length


def _rows(first, idx, ve, length):
    return torch.cat([torch.arange(first), first + idx.long().cpu(), torch.arange(ve, length)]).to(dev())


def _attend(cache, q, k, v, l):
    """The cache's attention over the views a feed returned, [1, Lq, Hq, D]; float32 rows take SDPA."""
    if q.dtype is not torch.float32:
        out = cache.attention(q, k, v, layer_idx=l)
        assert out is not None
        return out
    G = q.shape[1] // k.shape[1]
    rep = lambda t: t[:, :, None].expand(1, k.shape[1], G, t.shape[2], D).reshape(1, q.shape[1], t.shape[2], D)   # noqa: E731
    return torch.nn.functional.scaled_dot_product_attention(q, rep(k), rep(v), is_causal=q.shape[2] > 1).transpose(1, 2)


def _check_focus(d, route, watch, budget):
    """Checks 1 - 4 and 6 on a prefilled parent."""
    cache, dtype, Hq, Hkv = d.cache, d.dtype, d.Hq, d.Hkv
    branch = cache.fork(cache.video_end) if dtype is not torch.float32 else None
    asked = d.ask(route, watch)
    Wc = min(watch, QUESTION)
    assert cache.memory_footprint()["focus_queries"] == LAYERS * Hq * watch * D * asked[0][0].element_size()
    before = _state(cache)
    books = lambda: ([(st.c.length, st.c.pos_len, st.pinned, st.sc_len, st.sc_seen) for st in cache._layers],   # noqa: E731
                     cache._epoch, cache._mark_serial, cache._dead_marks, cache.video_end.serial, cache._flushes,
                     list(cache.budget_dropped), list(cache.num_evicted_tokens))
    books0 = books()
    scores0 = [cache.row_scores(l) for l in range(LAYERS)] if budget else None
    small = cache.focus(KEEP)
    # 4. the parent is not written to
    _same_state(cache, before, "the parent after focus")
    assert books() == books0
    if budget:
        for l in range(LAYERS):
            _same(cache.row_scores(l), scores0[l], ("row scores", l))
    if branch is not None:
        branch._branch_check()
        assert branch.get_seq_length(0) == before["len0"] - QUESTION
    pos = before["pos"]
    for l in range(LAYERS):
        first, ve, n, length = _geometry(cache, l)
        what = (route, dtype, Hq, watch, budget, "layer", l)
        assert first == TEXT and length == ve + QUESTION and n >= 288
        # 1. the observation against float64, under tests/rescore_ref.py's own bar at alpha = 1
        Q = cache.watched_queries(l)
        assert Q.shape == (Hq, Wc, D) and Q.dtype == dtype
        _same(Q, asked[l][0][0, :, QUESTION - Wc:], (what, "the question's last rotated query rows"))
        K = before[f"k{l}"][0, :, first:ve]
        got = small.focus_scores(l)
        assert got.shape == (n,) and got.dtype == torch.float32
        m64, want = rr.mass(Q, K, n), rr.obs(Q, K, n)
        bar = rr.bar(1.0, n, Wc, BAR[dtype], m64, want)
        err = (got.double() - want).abs()
        mean = got.double().mean().item()
        print(f"focus {what}: n {n} Wc {Wc}: max |obs - float64| = {err.max().item():.3e} ({(err / bar).max().item():.3f} of the "
              f"bar), mean obs - 1 = {mean - 1:.3e} (bar {bar.mean().item():.3e})")
        assert bool((err <= bar).all()), what
        assert abs(mean - 1.0) <= bar.mean().item(), what     # |mean got - mean want| <= mean |err|, and mean want is 1
        # 2. the kept list is the rule applied to the device's own scores: exact
        keep = min(KEEP, n)
        idx = small.focus_kept(l)
        assert idx.dtype == torch.int32 and torch.equal(idx.long().cpu(), br.survivors(got, keep)), what
        # 3. the focused rows are the parent's, bit for bit
        rows = _rows(first, idx, ve, length)
        _same(small.key_cache[l], before[f"k{l}"].index_select(2, rows), (what, "K"))
        _same(small.value_cache[l], before[f"v{l}"].index_select(2, rows), (what, "V"))
        _same(small.position_cache[l], pos[l].index_select(pos[l].ndim - 1, rows), (what, "ids"))
        assert small.get_seq_length(l) == first + keep + QUESTION
        assert small.num_evicted_tokens[l] == cache.num_evicted_tokens[l] + n - keep and small.focus_dropped[l] == n - keep
        assert int(small.get_prev_temporal_idx(l)) == before[f"prev{l}"]
        assert int(small.position_offset(l)) == int(cache.position_offset(l))
    assert "focus_queries" not in small.memory_footprint() and small.video_budget_rows is None and small._watch is None
    # 6. one decoded token on the focused cache: the attention over exactly the gathered rows
    from retake.native_attention import chunk_attention

    snap = _state(small)
    t = d.t_next
    token = d.feed(small, 60, d.text_ids(1), route)
    d.t_next = t
    for l, (q, kk, vv) in enumerate(token):
        what = (route, dtype, Hq, watch, budget, "decode, layer", l)
        Kg, Vg = torch.cat([snap[f"k{l}"], kk[:, :, -1:]], dim=2), torch.cat([snap[f"v{l}"], vv[:, :, -1:]], dim=2)
        _same(kk, Kg, (what, "K view"))
        _same(vv, Vg, (what, "V view"))
        out = _attend(small, q, kk, vv, l)
        if dtype is not torch.float32:
            direct = chunk_attention(q, Kg, Vg, workspace={})
            assert direct is not None
            _same(out, direct, (what, "chunk_attention on the gathered tensors"))
        ref = ar.attention_fp64(q, Kg, Vg)
        err = (out.double() - ref).abs().max().item()
        e = (ar.attention_eager_reference(q, Kg, Vg).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(dtype, ref.abs().max().item()))
        print(f"focus {what}: |out - float64| = {err:.3e}, eager {e:.3e}, bar {bar:.3e}")
        assert err <= bar, (what, err, bar)
    # ... and the parent still rewinds
    cache.rewind(cache.video_end)
    assert cache.get_seq_length(0) == before["len0"] - QUESTION
    return small


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("parent", ["unbounded", "budget"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("route", ["update", "pre_rope"])
def test_focus(route, ids, dtype, parent, shape):
    Hq, Hkv, chunks, watch = SHAPES[shape]
    _check_focus(_parent(ids, dtype, Hq, Hkv, chunks, parent == "budget"), route, watch, parent == "budget")


@pytest.mark.parametrize("shape", list(MIXED))
def test_focus_other_pairings(shape):
    Hq, Hkv, chunks, watch = MIXED[shape]
    _check_focus(_parent("mrope", torch.bfloat16, Hq, Hkv, chunks, False), "pre_rope", watch, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("ids", ["mrope", "plain"])
def test_keeping_every_row_decodes_like_the_parent(ids, dtype):
    """5. keep_rows >= n: one decoded token, fed the same projections through append_pre_rope + attention, gives bit-equal
    outputs on the focused cache and on the parent, in every layer."""
    d = _parent(ids, dtype, 4, 2, 5, True)
    cache = d.cache
    d.ask("pre_rope", 64)
    small = cache.focus(10 ** 6)
    assert small.focus_dropped == [0] * LAYERS and small.num_evicted_tokens == cache.num_evicted_tokens
    for l in range(LAYERS):
        n = _geometry(cache, l)[2]
        assert torch.equal(small.focus_kept(l).cpu(), torch.arange(n, dtype=torch.int32))
    pos = d.text_ids(1)
    a, b = d.feed(small, 61, pos, "pre_rope"), d.feed(cache, 61, pos, "pre_rope")
    for l in range(LAYERS):
        for x, y, name in zip(a[l], b[l], ("q", "K", "V")):
            _same(x, y, (name, l))
        _same(_attend(small, *a[l], l), _attend(cache, *b[l], l), ("attention", l))
    _same_state(small, cache, "the focused cache and the parent after the token")


def test_the_packed_attention_routes():
    """The focused cache carries the parent's attention options: one decoded token takes the packed kernel, four the wide
    packed one, each bit-equal to chunk_attention called with the same options on the gathered tensors."""
    from retake.native_attention import chunk_attention

    d = _build("mrope", torch.bfloat16, 4, 2, 5, False, decode_attention="packed", multi_token_attention="packed")
    d.ask("pre_rope", 64)
    small = d.cache.focus(KEEP)
    assert small.decode_attention == "packed" and small.multi_token_attention == "packed" and small.attention_kernel == "hip"
    for rows, counter in ((1, "decode_attention_calls"), (4, "wide_attention_calls")):
        calls = getattr(small, counter)
        token = d.feed(small, 62 + rows, d.text_ids(rows), "pre_rope")
        q, kk, vv = token[LAYERS - 1]
        out = small.attention(q, kk, vv, layer_idx=LAYERS - 1)
        took = getattr(small, counter) - calls
        route = []
        direct = chunk_attention(q, kk.contiguous(), vv.contiguous(), workspace={}, packed_gqa=True, packed_wide=took > 0 and rows > 1,
                                 route=route)
        _same(out, direct, (rows, "rows", route))
        if rows == 1:
            assert took == 1 and route == ["packed"]


def test_a_planted_row():
    """7. One region key set to 4 x the mean watched query of its kv group, at the region row with the lowest arrival score
    of a budget parent: the focus keeps it, a ranking by arrival score would not, and it is absent when the question's
    queries are replaced by ones orthogonal to it."""
    dtype, Hq, Hkv = torch.bfloat16, 4, 2
    d = _build("mrope", dtype, Hq, Hkv, 5, True)
    cache = d.cache
    asked = d.ask("update", 8)
    stars, planted, ortho = [], [], []
    for l in range(LAYERS):
        first, ve, n, _ = _geometry(cache, l)
        sc = cache.row_scores(l)
        j = int(torch.argmin(sc[:n - 1]))
        assert j not in br.survivors(sc, KEEP).tolist()
        Q = cache.watched_queries(l).float()                                  # [Hq, 8, D]
        key = (4 * Q.view(Hkv, -1, D).mean(dim=1)).to(dtype)                  # [Hkv, D]
        cache.key_cache[l][0, :, first + j] = key
        u = torch.nn.functional.normalize(key.double(), dim=1).repeat_interleave(Hq // Hkv, dim=0)[:, None, :]
        ortho.append((Q.double() - (Q.double() * u).sum(-1, keepdim=True) * u).to(dtype))
        stars.append(j)
        planted.append(key)
    small = cache.focus(KEEP)
    for l in range(LAYERS):
        kept = small.focus_kept(l).tolist()
        obs = small.focus_scores(l)
        print(f"planted row, layer {l}: row {stars[l]}, obs {float(obs[stars[l]]):.3f} (rank {int((obs > obs[stars[l]]).sum())})")
        assert stars[l] in kept, l
        _same(small.key_cache[l][0, :, TEXT + kept.index(stars[l])], planted[l], ("the planted key", l))
    d.fresh()
    d.ask("update", 8, queries=ortho)
    small = cache.focus(KEEP)
    for l in range(LAYERS):
        _same(cache.watched_queries(l), ortho[l], ("the replaced queries", l))
        obs = small.focus_scores(l)
        print(f"orthogonal queries, layer {l}: obs {float(obs[stars[l]]):.4f} (rank {int((obs > obs[stars[l]]).sum())})")
        assert stars[l] not in small.focus_kept(l).tolist(), l


def test_the_focused_cache_is_a_cache():
    """8. mark / rewind / crop within its own rows; NotImplementedError for a compressing update, fork, focus, watch_question."""
    d = _parent("mrope", torch.bfloat16, 4, 2, 5, False)
    d.ask("pre_rope", 64)
    small = d.cache.focus(KEEP, reserve_tokens=TEXT + KEEP + QUESTION + 2)    # (the third token outgrows the buffers)
    rows = TEXT + KEEP + QUESTION
    assert small.get_seq_length(0) == rows and small.video_end is not None and small.focused_from is not None
    assert small._layers[0]._k.shape[2] == rows + 2
    at_focus = _state(small)
    m = small.mark()
    for i in range(3):
        d.feed(small, 70 + i, d.text_ids(1), ("pre_rope", "update")[i % 2])
    assert small.get_seq_length(0) == rows + 3
    three = _state(small)
    small.crop(-2)
    assert small.get_seq_length(0) == rows + 1
    _same(small.key_cache[0], three["k0"][:, :, :rows + 1], "crop")
    with pytest.raises(ValueError, match="compressed video rows"):
        small.crop(rows - 1)                                                  # below its own focus point
    with pytest.raises(ValueError):
        small.rewind(m)                                                       # (a crop voids the marks behind video_end)
    small.rewind(small.video_end)
    _same_state(small, at_focus, "rewound to the focus point")
    q, k, v = _qkv(99, L, torch.bfloat16, 4, 2)
    pos = d.video_ids(L)
    small.kvcache_compression = True
    with pytest.raises(NotImplementedError, match="focused cache"):
        small.update(k, v, 0, {"query_states": q, "position_ids": pos, "rotary_emb": d.rot, "mrope_section": d.sec})
    with pytest.raises(NotImplementedError, match="focused cache"):
        small.update_pre_rope(q.clone(), k, v, 0, pos, d.rot, d.sec)
    with pytest.raises(NotImplementedError, match="focused cache"):
        small.append_pre_rope(q.clone(), k, v, 0, pos, d.rot, d.sec)
    small.kvcache_compression = False
    for call in (small.fork, lambda: small.focus(KEEP), small.watch_question):
        with pytest.raises(NotImplementedError, match="focused cache"):
            call()
    _same_state(small, at_focus, "after the refusals")


def test_refusals():
    """9. Every refusal raises its class before anything is launched, and the parent is unchanged."""
    d = _build("mrope", torch.bfloat16, 4, 2, 5, False)
    cache = d.cache

    def refused(exc, match, who=None, **kw):
        before, ws = _state(cache), dict(cache._ws)
        with pytest.raises(exc, match=match):
            (who or cache).focus(KEEP, **kw)
        _same_state(cache, before, match)
        assert dict(cache._ws) == ws

    refused(ValueError, "not armed")
    cache.watch_question(8)
    refused(ValueError, "nothing lies behind")                                # armed, no question yet
    d.feed(cache, 50, d.text_ids(QUESTION), with_queries=False)               # rows, but no query_states: nothing was captured
    refused(ValueError, "no watched queries")
    d.fresh()
    d.ask("update", 8, layers=[0])                                            # the question never reached layer 1
    refused(ValueError, "nothing lies behind")
    d.fresh()
    d.ask("update", 8)
    with pytest.raises(ValueError, match="keep_rows"):
        cache.focus(0)
    branch = cache.fork()
    refused(NotImplementedError, "branch", who=branch)
    with pytest.raises(NotImplementedError, match="branch"):
        branch.watch_question(8)
    cache.rewind(cache.video_end)
    refused(ValueError, "nothing lies behind")                                # the question is gone
    t = d.t_next = d.t_video
    m = cache.mark()
    d.ask("update", 8)
    d.t_next = t
    cache.rewind(m)
    d.feed(cache, 7, d.video_ids(L), video=True)                              # a chunk since arming: video_end moved
    d.t_video = d.t_next
    d.feed(cache, 50, d.text_ids(QUESTION))
    refused(ValueError, "no longer the mark")
    d.fresh()
    d.ask("pre_rope", 8)
    assert cache.focus(KEEP).get_seq_length(0) == TEXT + KEEP + QUESTION      # armed afresh: served
    # (kv_cache_dtype and defer_rerotation refuse before the cache is looked at: tests/test_focus_cpu.py)


def test_off_is_off():
    """10. A twin that never calls watch_question goes through the same chunks and question: bit-equal rows, no buffer."""
    for route in ("update", "pre_rope"):
        watched = _parent("mrope", torch.bfloat16, 4, 2, 5, False)
        a = watched.ask(route, 64)
        twin = _build("mrope", torch.bfloat16, 4, 2, 5, False)
        b = twin.feed(twin.cache, 50, twin.text_ids(QUESTION), route)
        for l in range(LAYERS):
            for x, y, name in zip(a[l], b[l], ("q", "K", "V")):
                _same(x, y, (route, name, l))
        _same_state(watched.cache, twin.cache, route)
        assert twin.cache._watch is None and "focus_queries" not in twin.cache.memory_footprint()
        assert "focus_queries" in watched.cache.memory_footprint()
        with pytest.raises(ValueError, match="watch_question"):
            twin.cache.watched_queries(0)


@pytest.mark.parametrize("route", ["update", "pre_rope"])
def test_re_arming(route):
    """11. The watched rows are those of the last uncompressed segment; a decode token replaces them with one row;
    unwatch_question frees them."""
    d = _parent("plain", torch.float16, 7, 1, 5, False)
    cache = d.cache
    asked = d.ask(route, 8)
    token = d.feed(cache, 80, d.text_ids(1), route)
    for l in range(LAYERS):
        _same(cache.watched_queries(l), token[l][0][0], ("the decode token's row", l))
        assert cache.watched_queries(l).shape == (7, 1, D)
    small = cache.focus(KEEP)                                                 # Wc = 1: the token's queries choose
    for l in range(LAYERS):
        first, ve, n, _ = _geometry(cache, l)
        want = rr.obs(token[l][0][0], cache.key_cache[l][0, :, first:ve], n)
        bar = rr.bar(1.0, n, 1, BAR[torch.float16], rr.mass(token[l][0][0], cache.key_cache[l][0, :, first:ve], n), want)
        assert bool(((small.focus_scores(l).double() - want).abs() <= bar).all()), l
        assert small.get_seq_length(l) == TEXT + KEEP + QUESTION + 1
    cache.watch_question(64)                                                  # arming again drops what was captured
    assert cache.watched_queries(0).numel() == 0 and cache.memory_footprint()["focus_queries"] == 0
    d.fresh()
    again = d.ask(route, 64)
    for l in range(LAYERS):
        _same(cache.watched_queries(l), again[l][0][0], ("the whole question", l))
        _same(again[l][0], asked[l][0], ("the same question", l))
    cache.unwatch_question()
    assert cache._watch is None and "focus_queries" not in cache.memory_footprint()
    with pytest.raises(ValueError, match="watch_question"):
        cache.watched_queries(0)
    with pytest.raises(ValueError, match="not armed"):
        cache.focus(KEEP)

"""PivotKVCache.watch_question / focus on an fp8 parent (kv_cache_dtype="fp8_e4m3" with archive_rescore=True), on
tests/test_focus_gpu.py's driver and geometry: 2 layers, D 128, Hq 4 / Hkv 2, 8 pinned text rows, chunks of 256 rows keeping
64, 5 chunks (n = 320: one key range) and 10 (n = 640: two), a question of 12 rows, keep_rows 96.  A budget parent holds
video_budget_rows = n - 32 and has evicted once.

The expected scores need no tolerance: rule 5 of the fp8 rows makes the dequantised archive exact in the model dtype, so
`focus_scores` must equal, bit for bit, the 16-BIT kernel (rtk_pivotkv_rescore_batched) at alpha = 1 on the dequantised
archive.  The focused cache is an fp8 cache: its archive holds the parent's codes and scales at the kept rows, its 16-bit
buffers the parent's 16-bit rows as they lie."""
import functools

import pytest
import torch

import attention_ref as ar
import budget_ref as br
from test_focus_gpu import D, KEEP, KEPT, L, LAYERS, QUESTION, TEXT, _Drv, _rows
from test_rescore_gpu import rescore
from test_rewind_gpu import _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu

Hq, Hkv = 4, 2
FP8 = {"kv_cache_dtype": "fp8_e4m3", "archive_rescore": True}


def _build(ids, dtype, chunks, budget, **top):
    d = _Drv(ids, dtype, Hq, Hkv, chunks * KEPT - 32 if budget else None, **dict(FP8, **top)).prefill(chunks)
    n = chunks * KEPT - (32 if budget else 0)
    assert d.cache.get_seq_length(0) == TEXT + n and d.cache.archive_len(0) == n
    assert d.cache.budget_dropped == [32] * LAYERS if budget else True
    return d


@functools.lru_cache(maxsize=None)
def _shared(ids, dtype, chunks, budget):
    return _build(ids, dtype, chunks, budget)


def _parent(*key):
    return _shared(*key).fresh()


def _dequant(codes, scales, dtype):
    from retake.native_attention import fp8_dequantize_rows

    return fp8_dequantize_rows(codes.contiguous(), scales.contiguous(), dtype)


def _sixteen_bit_scores(Q, k8, ks8, n, dtype):
    """obs [n] by rtk_pivotkv_rescore_batched at alpha = 1 into zeros, on the dequantised key rows."""
    k = _dequant(k8[:, :, :n], ks8[:, :, :n], dtype)[0].contiguous()
    return rescore([(Q.contiguous(), k, torch.zeros(n, dtype=torch.float32, device=dev()), n)], Hq, Hkv, Q.shape[1], D, dtype, 1.0)[0]


def _check_focus(d, route, watch, budget):
    from retake.native_attention import chunk_attention

    cache, dtype = d.cache, d.dtype
    asked = d.ask(route, watch)
    Wc = min(watch, QUESTION)
    before = _state(cache)
    rows16 = [(st.k[:, :, :st.length].clone(), st.v[:, :, :st.length].clone()) for st in cache._layers]
    books = lambda: ([(st.c.length, st.c.pos_len, st.len8, st.archive_at, st.pinned, st.sc_len, st.sc_seen)   # noqa: E731
                      for st in cache._layers], cache._epoch, cache._mark_serial, cache._dead_marks, cache.video_end.serial,
                     cache._flushes, list(cache.budget_dropped), list(cache.num_evicted_tokens))
    books0 = books()
    scores0 = [cache.row_scores(l) for l in range(LAYERS)] if budget else None
    small = cache.focus(KEEP)
    # the parent equals its snapshot: rows, lengths, marks and scores
    _same_state(cache, before, "the parent after focus")
    assert books() == books0
    if budget:
        for l in range(LAYERS):
            _same(cache.row_scores(l), scores0[l], ("row scores", l))
    assert small.kv_cache_dtype == "fp8_e4m3" and small.focused_from is not None
    pos = before["pos"]
    for l in range(LAYERS):
        st, what = cache._layers[l], (route, dtype, watch, budget, "layer", l)
        first, n, length = st.archive_at, st.len8, st.c.length
        assert first == TEXT and length == TEXT + QUESTION and n == before[f"len8_{l}"] >= 288
        # the scores: the bits of the 16-bit kernel at alpha = 1 on the dequantised archive
        Q = cache.watched_queries(l)
        assert Q.shape == (Hq, Wc, D) and Q.dtype == dtype
        _same(Q, asked[l][0][0, :, QUESTION - Wc:], (what, "the question's last rotated query rows"))
        got = small.focus_scores(l)
        want = _sixteen_bit_scores(Q, before[f"k8_{l}"], before[f"ks8_{l}"], n, dtype)
        assert got.shape == (n,) and got.dtype == torch.float32
        print(f"focus fp8 {what}: n {n} Wc {Wc}: {(got.view(torch.int32) != want.view(torch.int32)).sum().item()} scores differ "
              f"from the 16-bit kernel on the dequantised archive; mean obs - 1 = {got.double().mean().item() - 1:.3e}")
        _same(got, want, (what, "focus_scores"))
        # the kept list is the rule applied to the device's own scores
        keep = min(KEEP, n)
        idx = small.focus_kept(l)
        assert idx.dtype == torch.int32 and torch.equal(idx.long().cpu(), br.survivors(got, keep)), what
        # the focused archive, ids and 16-bit rows are the parent's at [pinned | kept | tail], bit for bit
        assert small.archive_len(l) == keep
        sst = small._layers[l]
        assert sst.k8.shape[2] == keep and sst.archive_at == first and sst.length == length and sst.len8 == keep
        for name, t in zip(("k8", "v8", "ks8", "vs8"), small.archive(l)):
            _same(t, before[f"{name}_{l}"].index_select(2, idx.long()), (what, name))
        _same(sst.k[:, :, :length], rows16[l][0], (what, "K16"))
        _same(sst.v[:, :, :length], rows16[l][1], (what, "V16"))
        rows = _rows(first, idx, first + n, first + n + QUESTION)
        _same(small.position_cache[l], pos[l].index_select(pos[l].ndim - 1, rows), (what, "ids"))
        _same(small.key_cache[l], before[f"k{l}"].index_select(2, rows), (what, "K dense"))
        _same(small.value_cache[l], before[f"v{l}"].index_select(2, rows), (what, "V dense"))
        assert small.get_seq_length(l) == first + keep + QUESTION
        assert small.num_evicted_tokens[l] == cache.num_evicted_tokens[l] + n - keep and small.focus_dropped[l] == n - keep
        assert int(small.get_prev_temporal_idx(l)) == before[f"prev{l}"]
    assert "focus_queries" not in small.memory_footprint() and small.video_budget_rows is None and small._watch is None
    # one decoded token on the focused cache: chunk_attention with the gathered archive, and float64 on the dequantised rows
    archives = [tuple(t.clone() for t in small.archive(l)) for l in range(LAYERS)]
    t = d.t_next
    token = d.feed(small, 60, d.text_ids(1), route)
    d.t_next = t
    for l, (q, kk, vv) in enumerate(token):
        what = (route, dtype, watch, budget, "decode, layer", l)
        _same(kk[:, :, :-1], rows16[l][0], (what, "K view"))
        out = small.attention(q, kk, vv, layer_idx=l)
        assert out is not None
        direct = chunk_attention(q, kk, vv, workspace={}, archive=archives[l])
        assert direct is not None
        _same(out, direct, (what, "chunk_attention with the gathered archive"))
        a = archives[l]
        Kg, Vg = torch.cat([_dequant(a[0], a[2], dtype), kk], dim=2), torch.cat([_dequant(a[1], a[3], dtype), vv], dim=2)
        ref = ar.attention_fp64(q, Kg, Vg)
        err = (out.double() - ref).abs().max().item()
        e = (ar.attention_eager_reference(q, Kg, Vg).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(dtype, ref.abs().max().item()))
        print(f"focus fp8 {what}: |out - float64| = {err:.3e}, eager {e:.3e}, bar {bar:.3e}")
        assert err <= bar, (what, err, bar)
    cache.rewind(cache.video_end)
    assert cache.get_seq_length(0) == before["len0"] - QUESTION
    return small


@pytest.mark.parametrize("parent", ["unbounded", "budget"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("route,ids,chunks,watch", [("update", "mrope", 5, 8), ("pre_rope", "plain", 10, 64)],
                         ids=["update-mrope-n320-w8", "pre_rope-plain-n640-w64"])
def test_focus(route, ids, chunks, watch, dtype, parent):
    _check_focus(_parent(ids, dtype, chunks, parent == "budget"), route, watch, parent == "budget")


@pytest.mark.parametrize("parent", ["unbounded", "budget"])
def test_keeping_every_row_gives_the_parents_rows(parent):
    d = _parent("mrope", torch.bfloat16, 5, parent == "budget")
    cache = d.cache
    d.ask("pre_rope", 64)
    small = cache.focus(10 ** 6)
    assert small.focus_dropped == [0] * LAYERS and small.num_evicted_tokens == cache.num_evicted_tokens
    for l in range(LAYERS):
        assert torch.equal(small.focus_kept(l).cpu(), torch.arange(cache.archive_len(l), dtype=torch.int32))
    _same_state(small, cache, "the focused cache and the parent")
    pos = d.text_ids(1)
    a, b = d.feed(small, 61, pos, "pre_rope"), d.feed(cache, 61, pos, "pre_rope")
    for l in range(LAYERS):
        for x, y, name in zip(a[l], b[l], ("q", "K", "V")):
            _same(x, y, (name, l))
        _same(small.attention(*a[l], layer_idx=l), cache.attention(*b[l], layer_idx=l), ("attention", l))


def test_a_planted_row():
    """One archive key row set to the quantised 4 x mean watched query of its kv group, at the region row with the lowest
    arrival score of a budget parent: the focus keeps it, a ranking by arrival score would not, and it is dropped once the
    question's queries are replaced by ones orthogonal to the (dequantised) planted key."""
    from retake.native_attention import fp8_quantize_rows

    dtype = torch.bfloat16
    d = _build("mrope", dtype, 5, True)
    cache = d.cache
    d.ask("update", 8)
    stars, planted, ortho = [], [], []
    for l in range(LAYERS):
        st = cache._layers[l]
        n = st.len8
        sc = cache.row_scores(l)
        j = int(torch.argmin(sc[:n - 1]))
        assert j not in br.survivors(sc, KEEP).tolist()
        Q = cache.watched_queries(l).float()                                  # [Hq, 8, D]
        key = (4 * Q.view(Hkv, -1, D).mean(dim=1)).to(dtype)                  # [Hkv, D]
        codes, scales = fp8_quantize_rows(key[None, :, None, :].contiguous())
        st.k8[0, :, j], st.ks8[0, :, j] = codes[0, :, 0], scales[0, :, 0]
        key8 = _dequant(codes, scales, dtype)[0, :, 0]                        # what the kernel sees
        u = torch.nn.functional.normalize(key8.double(), dim=1).repeat_interleave(Hq // Hkv, dim=0)[:, None, :]
        ortho.append((Q.double() - (Q.double() * u).sum(-1, keepdim=True) * u).to(dtype))
        stars.append(j)
        planted.append((codes[0, :, 0].clone(), scales[0, :, 0].clone()))
    small = cache.focus(KEEP)
    for l in range(LAYERS):
        kept = small.focus_kept(l).tolist()
        obs = small.focus_scores(l)
        print(f"fp8 planted row, layer {l}: row {stars[l]}, obs {float(obs[stars[l]]):.3f} (rank {int((obs > obs[stars[l]]).sum())})")
        assert stars[l] in kept, l
        at = kept.index(stars[l])
        _same(small.archive(l)[0][0, :, at], planted[l][0], ("the planted codes", l))
        _same(small.archive(l)[2][0, :, at], planted[l][1], ("the planted scales", l))
    d.fresh()
    d.ask("update", 8, queries=ortho)
    small = cache.focus(KEEP)
    for l in range(LAYERS):
        _same(cache.watched_queries(l), ortho[l], ("the replaced queries", l))
        obs = small.focus_scores(l)
        print(f"fp8 orthogonal queries, layer {l}: obs {float(obs[stars[l]]):.4f} (rank {int((obs > obs[stars[l]]).sum())})")
        assert stars[l] not in small.focus_kept(l).tolist(), l


def test_rewind_and_crop_stop_at_the_focus_point():
    d = _parent("mrope", torch.bfloat16, 5, False)
    d.ask("pre_rope", 64)
    small = d.cache.focus(KEEP)
    rows = TEXT + KEEP + QUESTION
    assert small.get_seq_length(0) == rows and small.video_end is not None
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
    for call in (small.fork, lambda: small.focus(KEEP), small.watch_question):
        with pytest.raises(NotImplementedError, match="focused cache"):
            call()
    _same_state(small, at_focus, "after the refusals")


def test_refusals():
    """Key off, not armed, `video_end` moved since arming: each raises before anything is launched, the parent unchanged."""
    off = _Drv("mrope", torch.bfloat16, Hq, Hkv, None, kv_cache_dtype="fp8_e4m3").prefill(2)
    off.ask("update", 8)
    before = _state(off.cache)
    with pytest.raises(ValueError, match="kv_cache_dtype") as ei:
        off.cache.focus(KEEP)
    assert "archive_rescore" in str(ei.value)
    _same_state(off.cache, before, "key off")

    d = _build("mrope", torch.bfloat16, 5, False)
    cache = d.cache

    def refused(match):
        before, ws = _state(cache), dict(cache._ws)
        with pytest.raises(ValueError, match=match):
            cache.focus(KEEP)
        _same_state(cache, before, match)
        assert dict(cache._ws) == ws

    refused("not armed")
    cache.watch_question(8)
    refused("nothing lies behind")                                            # armed, no question yet
    t = d.t_next = d.t_video
    m = cache.mark()
    d.ask("update", 8)
    d.t_next = t
    cache.rewind(m)
    d.feed(cache, 7, d.video_ids(L), video=True)                              # a chunk since arming: video_end moved
    d.t_video = d.t_next
    d.feed(cache, 50, d.text_ids(QUESTION))
    refused("no longer the mark")
    d.fresh()
    d.ask("pre_rope", 8)
    assert cache.focus(KEEP).get_seq_length(0) == TEXT + KEEP + QUESTION      # armed afresh: served

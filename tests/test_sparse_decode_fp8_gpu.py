"""sparse_decode(cache, keep_rows, archive=True) on fp8 parents (kv_cache_dtype="fp8_e4m3"), on the driver of
tests/test_focus_gpu.py: 2 layers, D 128, Hq 4 / Hkv 2, 8 pinned text rows, a question of 12 rows, keep_rows 96 (3 pages).

Parents: chunks through `update` (5 chunks of 256 rows keeping 64: n = 320 archive rows, 10 pages) and through
`update_pre_rope` (3 chunks of 512 rows keeping 128: n = 384, 12 pages); both RoPE flavours, bf16 / fp16; unbounded, and with
video_budget_rows = n - 27, which leaves a partial last page of 5 rows.  The shared parents are only read, armed and disarmed;
a test that writes rows or moves `video_end` builds its own."""
import functools

import pytest
import torch

import retake._sparse_decode as sd
import sparse_decode_ref as sr
from sparse_decode_ref import dequant as _dequant, token as _token
from test_attention_decode_gpu import _against_fp64
from test_focus_gpu import D, LAYERS, QUESTION, TEXT, _Drv, _qkv
from test_rewind_gpu import _bits, _same, _same_state, _state, dev

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
Hq, Hkv, PAGE = 4, 2, 32
KEEP_ROWS = 96   # 3 pages
SHAPE = {"update": (5, 256), "pre_rope": (3, 512)}   # chunks, rows a chunk; a quarter of the rows is kept
PARENTS = [("update", "mrope", False), ("pre_rope", "plain", True), ("update", "plain", True), ("pre_rope", "mrope", False)]
PARENT_IDS = ["update-mrope-unbounded", "pre_rope-plain-budget", "update-plain-budget", "pre_rope-mrope-unbounded"]


class _Drv8(_Drv):
    """test_focus_gpu's driver on an fp8 cache; route "pre_rope" sends video chunks through `update_pre_rope`."""

    def feed(self, cache, seed, pos, route="update", video=False, **kw):
        if not (video and route == "pre_rope"):
            return super().feed(cache, seed, pos, route, video, **kw)
        n, outs = pos.shape[-1], []
        cache.kvcache_compression = True
        try:
            for l in range(LAYERS):
                q, k, v = _qkv(1000 * seed + l, n, self.dtype, self.Hq, self.Hkv)
                out = cache.update_pre_rope(q.clone(), k, v, l, pos.clone(), self.rot, self.sec)
                assert out is not None, "update_pre_rope declined the chunk"
                outs.append(out)
            cache.after_forward()
        finally:
            cache.kvcache_compression = False
        return outs

    def prefill8(self, route):
        chunks, rows = SHAPE[route]
        self.feed(self.cache, 1, self.text_ids(TEXT))
        for c in range(chunks):
            self.feed(self.cache, 2 + c, self.video_ids(rows), route, video=True)
        self.t_video = self.t_next
        return self


def _rows_of(route, budget):
    chunks, rows = SHAPE[route]
    return chunks * rows // 4 - (27 if budget else 0)


def _build(route, ids, dtype, budget, **top):
    n = _rows_of(route, budget)
    d = _Drv8(ids, dtype, Hq, Hkv, n if budget else None, **dict({"kv_cache_dtype": "fp8_e4m3"}, **top)).prefill8(route)
    for l in range(LAYERS):
        assert d.cache.archive_len(l) == n and d.cache._layers[l].c.length == TEXT, (l, d.cache.archive_len(l))
    assert d.cache.get_seq_length(0) == TEXT + n
    return d


@functools.lru_cache(maxsize=None)
def _shared(route, ids, dtype, budget):
    return _build(route, ids, dtype, budget)


def _parent(*key):
    d = _shared(*key)
    sd.dense_decode(d.cache)
    return d.fresh()


def _dequant_keys(cache, l, dtype):
    """The layer's archived keys as the attention uses them, [Hkv, n, D]."""
    a = cache.archive(l)
    return _dequant(a[0], a[2], dtype)[0]


def _gathered(cache, l, lists):
    """(k8, v8, k_scale, v_scale) of the pages each kv head's list names: their existing rows, in list order."""
    return sr.gather_archive(cache.archive(l), cache.archive_len(l), lists)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route,ids,budget", PARENTS, ids=PARENT_IDS)
def test_armed_decode_tokens_take_the_sparse_route(route, ids, budget, dtype):
    from retake.native_attention import chunk_attention

    d = _parent(route, ids, dtype, budget)
    cache, n = d.cache, _rows_of(route, budget)
    pages = sr.pages_of(n)
    base, built = cache.sparse_attention_calls, cache.page_summary_calls   # (the shared parent counts over all tests)
    try:
        # off is off: without the key the fp8 cache is refused as before, and nothing is launched
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            sd.sparse_decode(cache, KEEP_ROWS)
        assert cache._sparse is None and cache.page_summary_calls == built
        sd.sparse_decode(cache, KEEP_ROWS, archive=True)
        assert cache.page_summary_calls == built + 1
        foot = cache.memory_footprint()
        assert foot["page_summaries"] == LAYERS * Hkv * pages * 2 * D * 2
        for l in range(LAYERS):
            got = sd.page_summaries(cache, l)
            want = sr.summaries(_dequant_keys(cache, l, dtype), 0, n).to(dev())
            assert got.dtype == dtype and got.shape == (Hkv, pages, 2, D) and torch.equal(_bits(got), _bits(want)), ("summaries", l)
        # the question's own multi-row prefill takes the existing route, bit for bit
        asked = d.feed(cache, 50, d.text_ids(QUESTION), route)
        armed = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(asked)]
        assert cache.sparse_attention_calls == base
        for l, (q, k, v) in enumerate(asked):
            _same(armed[l], chunk_attention(q, k, v, workspace={}, archive=cache.archive(l)), ("the question's rows", l))
        calls = base
        for t in range(2):
            outs = _token(d, route, 60 + t)
            before = _state(cache)
            for l, (q, k, v) in enumerate(outs):
                out = cache.attention(q, k, v, layer_idx=l)
                calls += 1
                assert cache.sparse_attention_calls == calls and out.shape == (1, 1, Hq, D)
                ub, lists = sd.sparse_bounds(cache, l), sd.sparse_pages(cache, l)
                assert ub.shape == (Hkv, pages) and lists.shape == (Hkv, 3) and lists.dtype == torch.int32
                # the lists are the rule applied to the device's own bounds, exactly; the bounds are float64's under the bar
                assert torch.equal(lists.cpu(), sr.select(ub, 3)), ("lists", t, l)
                want, bar = sr.bound(q[0], sd.page_summaries(cache, l))
                assert ((ub.double().cpu() - want).abs() <= bar).all()
                # the pages the call chose, gathered: the packed fp8 call over them, bit for bit, and float64 on their
                # dequantised rows
                g = _gathered(cache, l, lists.cpu())
                assert g[0].shape[2] == 2 * PAGE + (n - PAGE * (pages - 1))
                tag = []
                direct = chunk_attention(q, k, v, workspace={}, archive=g, packed_gqa=True, route=tag)
                assert tag == ["packed"]
                _same(out, direct, ("chunk_attention over the gathered archive", t, l))
                kc, vc = torch.cat([_dequant(g[0], g[2], dtype), k], dim=2), torch.cat([_dequant(g[1], g[3], dtype), v], dim=2)
                _against_fp64(f"sparse fp8 {route} {ids} {dtype} token {t} layer {l}", q, kc, vc, out, dtype)
            # the parent's codes, scales, ids, 16-bit rows and counters are only read
            _same_state(cache, before, "the cache after routed calls")
        with pytest.raises(ValueError, match="layer_idx"):
            cache.attention(*outs[0])
    finally:   # (the parent is shared)
        sd.dense_decode(cache)
    foot = cache.memory_footprint()
    assert "page_summaries" not in foot and "sparse_workspace" not in foot


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route,ids,budget", PARENTS[:2], ids=PARENT_IDS[:2])
def test_keeping_every_page_is_the_unarmed_packed_call_bit_for_bit(route, ids, budget, dtype):
    d = _build(route, ids, dtype, budget, decode_attention="packed")
    cache, n = d.cache, _rows_of(route, budget)
    foot0 = cache.memory_footprint()
    d.feed(cache, 50, d.text_ids(QUESTION), "pre_rope")
    outs = _token(d, "pre_rope", 60)
    dense = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]   # never armed
    assert cache.decode_attention_calls == LAYERS and cache.sparse_attention_calls == 0
    sd.sparse_decode(cache, 10 ** 6, archive=True)
    sparse = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]
    assert cache.sparse_attention_calls == LAYERS
    pages = sr.pages_of(n)
    assert torch.equal(sd.sparse_pages(cache, 0).cpu(), torch.arange(pages, dtype=torch.int32).expand(Hkv, pages))
    foot = cache.memory_footprint()
    assert foot["page_summaries"] > 0 and foot["sparse_workspace"] > 0
    sd.dense_decode(cache)
    again = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]      # off is off again
    for a, b, c in zip(dense, sparse, again):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    cache.rewind(cache.video_end)
    foot = cache.memory_footprint()
    assert "page_summaries" not in foot and "sparse_workspace" not in foot and foot.keys() == foot0.keys()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_planted_key_moves_one_heads_list_only(dtype):
    """A key along u in an old page of kv head 1's archive only: that page enters head 1's list when head 1's queries point
    along u, not head 0's; it leaves head 1's list when the queries are made orthogonal to u.  The margins are checked on the
    CPU with the float64 reference, on the dequantised keys, to exceed the bound's bar a hundred times over."""
    from retake.native_attention import fp8_quantize_rows

    d = _build("update", "mrope", dtype, False)
    cache, n = d.cache, _rows_of("update", False)
    u = torch.zeros(D)
    u[:64] = 1.0
    w = 1.0 - u
    g = torch.Generator().manual_seed(4)
    q0 = (1.7 * torch.randn((2, 1, D), generator=g))   # the two query heads of kv head 0
    pages = sr.pages_of(n)

    def queries(direction):
        return [torch.cat([q0, (2.0 * direction).expand(2, 1, D)]).to(dtype).to(dev()) for _ in range(LAYERS)]

    # the old page head 0's queries rank lowest, by the reference, before anything is planted
    ub0, _ = sr.bound(queries(u)[0], sr.summaries(_dequant_keys(cache, 0, dtype), 0, n))
    P = int(ub0[0, :pages - 1].argmin())
    rows = (0.01 * torch.randn((1, 1, PAGE, D), generator=g)).to(dtype)
    rows[0, 0, 5] = (16.0 * u).to(dtype)
    codes, scales = fp8_quantize_rows(rows.to(dev()))
    for l in range(LAYERS):
        st = cache._layers[l]
        st.k8[0, 1, PAGE * P:PAGE * P + PAGE], st.ks8[0, 1, PAGE * P:PAGE * P + PAGE] = codes[0, 0], scales[0, 0]
    sd.sparse_decode(cache, KEEP_ROWS, archive=True)
    d.feed(cache, 50, d.text_ids(QUESTION), "update")
    for direction, inside in ((u, True), (w, False)):
        qs = queries(direction)
        outs = _token(d, "update", 70, queries=qs)
        for l, (q, k, v) in enumerate(outs):
            assert torch.equal(q[0, :, -1:], qs[l])
            want, bar = sr.bound(q[0], sr.summaries(_dequant_keys(cache, l, dtype), 0, n))
            others = torch.cat([want[:, :P], want[:, P + 1:pages - 1]], dim=1).sort(dim=1, descending=True).values
            # head 1: P is the best old page along u, the worst along w; head 0: P stays below its two best old pages
            if inside:
                assert want[1, P] - others[1, 0] > 100 * bar.max()
            else:
                assert others[1, 1] - want[1, P] > 100 * bar.max()
            assert others[0, 1] - want[0, P] > 100 * bar.max() or l > 0
            cache.attention(q, k, v, layer_idx=l)
            lists = sd.sparse_pages(cache, l).cpu()
            assert (P in lists[1].tolist()) == inside, (direction is u, l, lists)
            if l == 0:
                assert P not in lists[0].tolist()
    assert cache.sparse_attention_calls == 2 * LAYERS


def test_the_index_survives_a_rewind_and_a_chunk_voids_it():
    d = _build("update", "plain", torch.bfloat16, False)
    cache = d.cache
    sd.sparse_decode(cache, KEEP_ROWS, archive=True)
    built = cache.page_summary_calls
    summ = sd.page_summaries(cache, 1)
    for question in range(2):   # the second question pays nothing: no summary launch, the same index
        d.feed(cache, 50 + question, d.text_ids(QUESTION), "pre_rope")
        outs = _token(d, "pre_rope", 60 + question)
        for l, (q, k, v) in enumerate(outs):
            cache.attention(q, k, v, layer_idx=l)
        assert cache.sparse_attention_calls == (question + 1) * LAYERS and cache.page_summary_calls == built
        cache.rewind(cache.video_end)
        d.t_next = d.t_video
    assert torch.equal(_bits(sd.page_summaries(cache, 1)), _bits(summ))
    # a chunk after arming: the next routed call raises and says what to do
    d.feed(cache, 9, d.video_ids(256), video=True)
    outs = _token(d, "pre_rope", 61)
    with pytest.raises(ValueError, match="sparse_decode again"):
        cache.attention(*outs[0], layer_idx=0)
    sd.sparse_decode(cache, KEEP_ROWS, archive=True)   # armed again over 6 chunks
    assert cache.page_summary_calls == built + 1 and sd.page_summaries(cache, 0).shape[1] == 12
    assert cache.attention(*outs[0], layer_idx=0) is not None
    assert cache.sparse_attention_calls == 2 * LAYERS + 1

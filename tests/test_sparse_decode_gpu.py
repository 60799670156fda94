"""sparse_decode(cache) / dense_decode(cache) (retake/_sparse_decode.py) at cache level, on the stand-in modules and small chunks of
tests/test_focus_gpu.py (2 layers, D 128, Hq 4 / Hkv 2, chunks of 256 rows at ratio 0.25: 64 kept rows a chunk, 5 chunks:
n = 320 region rows = 10 pages behind 8 pinned rows; an ALIGNED parent has 32 pinned rows), both entry routes, bf16 / fp16.

Parents are built per test where the test writes rows or moves `video_end`; the shared ones of test_focus_gpu are only read,
armed and disarmed."""
import pytest
import torch

import retake._sparse_decode as sd
import sparse_decode_ref as sr
from sparse_decode_ref import token as _token
from test_attention_decode_gpu import _against_fp64
from test_focus_gpu import D, L, LAYERS, QUESTION, TEXT, _Drv, _build, _geometry, _parent
from test_rewind_gpu import _bits, _same_state, _state, dev

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
Hq, Hkv, CHUNKS, PAGE = 4, 2, 5, 32
KEEP_ROWS = 96   # 3 of the 10 pages


def _fresh(d):
    sd.dense_decode(d.cache)
    return d.fresh()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route", ["update", "pre_rope"])
def test_armed_decode_tokens_take_the_sparse_route(dtype, route):
    d = _fresh(_parent("mrope", dtype, Hq, Hkv, CHUNKS, False))
    cache = d.cache
    base, built = cache.sparse_attention_calls, cache.page_summary_calls   # (the shared parent counts over all tests)
    try:
        sd.sparse_decode(cache, KEEP_ROWS)
        assert cache.page_summary_calls == built + 1
        foot = cache.memory_footprint()
        assert foot["page_summaries"] == LAYERS * Hkv * 10 * 2 * D * 2
        for l in range(LAYERS):
            first, ve, n, _ = _geometry(cache, l)
            assert (first, n) == (TEXT, 320)
            got = sd.page_summaries(cache, l)
            want = sr.summaries(cache._layers[l]._k[0], first, n).to(dev())
            assert got.dtype == dtype and torch.equal(_bits(got), _bits(want)), ("summaries", l)
        # the question's own multi-row prefill takes the existing routes
        asked = d.feed(cache, 50, d.text_ids(QUESTION), route)
        for l, (q, k, v) in enumerate(asked):
            assert cache.attention(q, k, v, layer_idx=l) is not None
        assert cache.sparse_attention_calls == base
        calls = base
        for t in range(2):
            outs = _token(d, route, 60 + t)
            before = _state(cache)
            for l, (q, k, v) in enumerate(outs):
                first, ve, n, length = _geometry(cache, l)
                out = cache.attention(q, k, v, layer_idx=l)
                calls += 1
                assert cache.sparse_attention_calls == calls and out.shape == (1, 1, Hq, D)
                ub, lists = sd.sparse_bounds(cache, l), sd.sparse_pages(cache, l)
                assert ub.shape == (Hkv, 10) and lists.shape == (Hkv, 3) and lists.dtype == torch.int32
                # the lists are the rule applied to the device's own bounds, exactly; the bounds are float64's under the bar
                assert torch.equal(lists.cpu(), sr.select(ub, 3)), ("lists", t, l)
                want, bar = sr.bound(q[0], sd.page_summaries(cache, l))
                assert ((ub.double().cpu() - want).abs() <= bar).all()
                kc, vc = sr.gather(k, v, first, ve, length, lists.cpu())
                _against_fp64(f"sparse {route} {dtype} token {t} layer {l}", q, kc, vc, out, dtype)
            # the parent's rows, ids and counters are only read
            _same_state(cache, before, "the cache after routed calls")
        with pytest.raises(ValueError, match="layer_idx"):
            cache.attention(*outs[0])
    finally:   # (the parent is shared with tests/test_focus_gpu.py)
        sd.dense_decode(cache)
    assert "page_summaries" not in cache.memory_footprint()


def _aligned(dtype, **top):
    """A parent of its own with 32 pinned rows: first % 32 == 0 and n % 32 == 0."""
    d = _Drv("mrope", dtype, Hq, Hkv, **top)
    d.feed(d.cache, 1, d.text_ids(32))
    for c in range(CHUNKS):
        d.feed(d.cache, 2 + c, d.video_ids(L), video=True)
    d.t_video = d.t_next
    return d


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_keeping_every_page_is_the_unarmed_packed_call_bit_for_bit(dtype):
    d = _aligned(dtype, decode_attention="packed")
    cache = d.cache
    foot0 = cache.memory_footprint()
    d.feed(cache, 50, d.text_ids(QUESTION), "pre_rope")
    outs = _token(d, "pre_rope", 60)
    dense = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]   # never armed
    assert cache.decode_attention_calls == LAYERS and cache.sparse_attention_calls == 0
    sd.sparse_decode(cache, 10 ** 6)
    assert _geometry(cache, 0)[:3] == (32, 32 + 320, 320)
    sparse = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]
    assert cache.sparse_attention_calls == LAYERS
    assert torch.equal(sd.sparse_pages(cache, 0).cpu(), torch.arange(10, dtype=torch.int32).expand(Hkv, 10))
    sd.dense_decode(cache)
    again = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]      # off is off again
    for a, b, c in zip(dense, sparse, again):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    cache.rewind(cache.video_end)
    foot = cache.memory_footprint()
    assert "page_summaries" not in foot and "sparse_workspace" not in foot and foot.keys() == foot0.keys()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_planted_key_moves_one_heads_list_only(dtype):
    """A key along u in an old page of kv head 1 only: that page enters head 1's list when head 1's queries point along u,
    not head 0's; it leaves head 1's list when the queries are made orthogonal to u.  The margins are checked on the CPU
    with the float64 reference to exceed the bound's bar a hundred times over."""
    d = _build("mrope", dtype, Hq, Hkv, CHUNKS, False)
    cache = d.cache
    u = torch.zeros(D)
    u[:64] = 1.0
    w = 1.0 - u
    g = torch.Generator().manual_seed(4)
    q0 = (1.7 * torch.randn((2, 1, D), generator=g))   # the two query heads of kv head 0
    first, ve, n, _ = _geometry(cache, 0)
    pages = sr.pages_of(n)

    def queries(direction):
        return [torch.cat([q0, (2.0 * direction).expand(2, 1, D)]).to(dtype).to(dev()) for _ in range(LAYERS)]

    # the old page head 0's queries rank lowest, by the reference, before anything is planted
    summ0 = sr.summaries(cache._layers[0]._k[0], first, n)
    ub0, bar0 = sr.bound(queries(u)[0], summ0)
    P = int(ub0[0, :pages - 1].argmin())
    for l in range(LAYERS):
        k = cache._layers[l]._k
        rows = slice(first + PAGE * P, first + PAGE * P + PAGE)
        k[0, 1, rows] = (0.01 * torch.randn((PAGE, D), generator=g)).to(dtype).to(dev())
        k[0, 1, first + PAGE * P + 5] = (16.0 * u).to(dtype).to(dev())
    sd.sparse_decode(cache, KEEP_ROWS)
    d.feed(cache, 50, d.text_ids(QUESTION), "update")
    for direction, inside in ((u, True), (w, False)):
        qs = queries(direction)
        outs = _token(d, "update", 70, queries=qs)
        for l, (q, k, v) in enumerate(outs):
            assert torch.equal(q[0, :, -1:], qs[l])
            want, bar = sr.bound(q[0], sr.summaries(cache._layers[l]._k[0], first, n))
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
    d = _build("plain", torch.bfloat16, Hq, Hkv, CHUNKS, False)
    cache = d.cache
    sd.sparse_decode(cache, KEEP_ROWS)
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
    d.feed(cache, 9, d.video_ids(L), video=True)
    outs = _token(d, "pre_rope", 61)
    with pytest.raises(ValueError, match="sparse_decode again"):
        cache.attention(*outs[0], layer_idx=0)
    sd.sparse_decode(cache, KEEP_ROWS)   # armed again over 6 chunks
    assert cache.page_summary_calls == built + 1 and sd.page_summaries(cache, 0).shape[1] == 12
    assert cache.attention(*outs[0], layer_idx=0) is not None


def test_arming_refuses_an_fp32_model():
    d = _fresh(_parent("mrope", torch.float32, Hq, Hkv, CHUNKS, False))
    d.cache.attention_kernel = "hip"
    try:
        with pytest.raises(NotImplementedError, match="bfloat16 or float16"):
            sd.sparse_decode(d.cache)
    finally:
        d.cache.attention_kernel = None
    assert d.cache._sparse is None and d.cache.page_summary_calls == 0

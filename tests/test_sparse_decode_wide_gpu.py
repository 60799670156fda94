"""sparse_decode(cache, keep_rows, wide=True) (retake/_sparse_decode.py) at cache level: calls of 17 to 64 packed rows - the
verification call of assisted generation, a short follow-up - take ONE rtk_attention_decode_sparse_wide call, all their rows
sharing one page list per kv head.  On the stand-in modules and small chunks of tests/test_focus_gpu.py (2 layers, D 128,
chunks of 256 rows at ratio 0.25: 64 kept rows a chunk, 5 chunks: n = 320 region rows = 10 pages behind 8 pinned rows; an
ALIGNED parent has 32 pinned rows): 12 rows at Hq 4 / Hkv 2 and 6 rows at Hq 8 / Hkv 2 are 24 packed rows each.

Parents are built per test where the test writes rows or moves `video_end`; the shared ones of test_focus_gpu are only read,
armed and disarmed."""
import pytest
import torch

import retake._sparse_decode as sd
import sparse_decode_ref as sr
from test_attention_decode_gpu import _against_fp64
from test_focus_gpu import D, L, LAYERS, QUESTION, _Drv, _build, _geometry, _parent
from test_rewind_gpu import _bits, _same_state, _state, dev

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
Hkv, CHUNKS, PAGE = 2, 5, 32
KEEP_ROWS = 96   # 3 of the 10 pages
CALLS = [(4, QUESTION), (8, 6)]   # (Hq, new rows): G 2 x 12 and G 4 x 6 packed rows
CALL_IDS = ["Hq4-12rows", "Hq8-6rows"]


def _fresh(d):
    sd.dense_decode(d.cache)
    return d.fresh()


def _check_routed(cache, l, q, k, v, out, tag, dtype):
    """The layer's last routed call: its lists are the rule applied to the device's own bounds, exactly; the bounds are
    float64's (the max over the packed rows of EVERY position) under the bar; the output float64's on the gathered rows."""
    first, ve, n, length = _geometry(cache, l)
    ub, lists = sd.sparse_bounds(cache, l), sd.sparse_pages(cache, l)
    assert ub.shape == (Hkv, 10) and lists.shape == (Hkv, 3) and lists.dtype == torch.int32
    assert torch.equal(lists.cpu(), sr.select(ub, 3)), ("lists", tag, l)
    want, bar = sr.bound(q[0].contiguous(), sd.page_summaries(cache, l))
    assert ((ub.double().cpu() - want).abs() <= bar).all()
    kc, vc = sr.gather(k, v, first, ve, length, lists.cpu())
    _against_fp64(f"sparse wide {tag} layer {l}", q, kc, vc, out, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route", ["update", "pre_rope"])
@pytest.mark.parametrize("Hq,rows", CALLS, ids=CALL_IDS)
def test_armed_wide_calls_take_the_sparse_route(dtype, route, Hq, rows):
    d = _fresh(_parent("mrope", dtype, Hq, Hkv, CHUNKS, False))
    cache = d.cache
    base, built = cache.sparse_attention_calls, cache.page_summary_calls   # (the shared parent counts over all tests)
    try:
        sd.sparse_decode(cache, KEEP_ROWS, wide=True)
        assert cache.page_summary_calls == built + 1 and sd.sparse_wide_calls(cache) == 0
        outs = d.feed(cache, 50, d.text_ids(rows), route)
        before = _state(cache)
        for l, (q, k, v) in enumerate(outs):
            out = cache.attention(q, k, v, layer_idx=l)
            assert cache.sparse_attention_calls == base + l + 1 and sd.sparse_wide_calls(cache) == l + 1
            assert out.shape == (1, rows, Hq, D) and out.dtype == dtype
            _check_routed(cache, l, q, k, v, out, f"{route} {dtype} Hq{Hq}", dtype)
        # the parent's rows, ids and counters are only read
        _same_state(cache, before, "the cache after routed wide calls")
        # a decode token behind them takes the narrow call: counted as sparse, not as wide
        tok = d.feed(cache, 60, d.text_ids(1), route)
        assert cache.attention(*tok[0], layer_idx=0).shape == (1, 1, Hq, D)
        assert cache.sparse_attention_calls == base + LAYERS + 1 and sd.sparse_wide_calls(cache) == LAYERS
    finally:   # (the parent is shared with tests/test_focus_gpu.py)
        sd.dense_decode(cache)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Hq,rows", CALLS, ids=CALL_IDS)
def test_armed_without_wide_the_same_calls_go_where_they_went(dtype, Hq, rows):
    d = _fresh(_parent("mrope", dtype, Hq, Hkv, CHUNKS, False))
    cache = d.cache
    try:
        outs = d.feed(cache, 50, d.text_ids(rows), "pre_rope")
        unarmed = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]
        base, calls = cache.sparse_attention_calls, cache.attention_calls
        sd.sparse_decode(cache, KEEP_ROWS)
        armed = [cache.attention(q, k, v, layer_idx=l) for l, (q, k, v) in enumerate(outs)]
        assert cache.sparse_attention_calls == base and sd.sparse_wide_calls(cache) == 0
        assert cache.attention_calls == calls + LAYERS
        for a, b in zip(unarmed, armed):
            assert torch.equal(_bits(a), _bits(b))
    finally:
        sd.dense_decode(cache)


def _aligned(dtype, Hq):
    """A parent of its own with 32 pinned rows: first % 32 == 0 and n % 32 == 0."""
    d = _Drv("mrope", dtype, Hq, Hkv)
    d.feed(d.cache, 1, d.text_ids(32))
    for c in range(CHUNKS):
        d.feed(d.cache, 2 + c, d.video_ids(L), video=True)
    d.t_video = d.t_next
    return d


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_keeping_every_page_is_the_wide_packed_call_bit_for_bit(dtype):
    import retake.longvideo_cache as lc

    Hq = 4
    d = _aligned(dtype, Hq)
    cache = d.cache
    outs = d.feed(cache, 50, d.text_ids(QUESTION), "pre_rope")
    sd.sparse_decode(cache, 10 ** 6, wide=True)
    assert _geometry(cache, 0)[:3] == (32, 32 + 320, 320)
    for l, (q, k, v) in enumerate(outs):
        sparse = cache.attention(q, k, v, layer_idx=l)
        took = []
        dense = lc.chunk_attention(q, k, v, packed_gqa=True, packed_wide=True, route=took)
        assert took == ["wide"], took
        assert torch.equal(_bits(sparse), _bits(dense)), l
    assert cache.sparse_attention_calls == LAYERS == sd.sparse_wide_calls(cache)
    assert torch.equal(sd.sparse_pages(cache, 0).cpu(), torch.arange(10, dtype=torch.int32).expand(Hkv, 10))


def test_a_rejected_draft_is_cropped_and_the_next_verification_call_is_routed():
    """Arm, feed 6 draft rows and attend, give up three of them (`crop`), feed 6 again and attend: the second call is routed,
    no summary is built again, and its lists follow the new rows' queries."""
    Hq, dtype = 8, torch.bfloat16
    d = _build("mrope", dtype, Hq, Hkv, CHUNKS, False)
    cache = d.cache
    sd.sparse_decode(cache, KEEP_ROWS, wide=True)
    built = cache.page_summary_calls
    for step, seed in enumerate((60, 61)):
        outs = d.feed(cache, seed, d.text_ids(6), "pre_rope")
        for l, (q, k, v) in enumerate(outs):
            first, ve, n, length = _geometry(cache, l)
            assert length == ve + 6 + 3 * step and k.shape[2] == length
            out = cache.attention(q, k, v, layer_idx=l)
            assert sd.sparse_wide_calls(cache) == step * LAYERS + l + 1
            _check_routed(cache, l, q, k, v, out, f"draft step {step}", dtype)
        if step == 0:
            cache.crop(-3)
            d.t_next -= 3
            assert cache._sparse is not None and cache.get_seq_length(0) == _geometry(cache, 0)[1] + 3
    assert cache.page_summary_calls == built and cache.sparse_attention_calls == 2 * LAYERS


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_planted_key_enters_the_list_through_the_last_draft_row_alone(dtype):
    """A key along u in an old page of kv head 1: that page enters head 1's list when ONLY THE LAST of the 12 rows' queries
    points along u (the other 11 are orthogonal to u) - one list serves every row, so a page one row needs is ranked by that
    row - and leaves when that row is made orthogonal too.  The margins are checked on the CPU with the float64 reference
    to exceed the bound's bar a hundred times over."""
    Hq = 4
    d = _build("mrope", dtype, Hq, Hkv, CHUNKS, False)
    cache = d.cache
    u = torch.zeros(D)
    u[:64] = 1.0
    w = 1.0 - u
    g = torch.Generator().manual_seed(4)
    q0 = (1.7 * torch.randn((2, QUESTION, D), generator=g))   # the two query heads of kv head 0, every row
    first, ve, n, _ = _geometry(cache, 0)
    pages = sr.pages_of(n)

    def queries(direction):
        rows = torch.cat([(2.0 * w).expand(2, QUESTION - 1, D), (2.0 * direction).expand(2, 1, D)], dim=1)
        return [torch.cat([q0, rows]).to(dtype).to(dev()) for _ in range(LAYERS)]

    # the old page head 0's queries rank lowest, by the reference, before anything is planted
    summ0 = sr.summaries(cache._layers[0]._k[0], first, n)
    ub0, bar0 = sr.bound(queries(u)[0], summ0)
    P = int(ub0[0, :pages - 1].argmin())
    for l in range(LAYERS):
        k = cache._layers[l]._k
        rows = slice(first + PAGE * P, first + PAGE * P + PAGE)
        k[0, 1, rows] = (0.01 * torch.randn((PAGE, D), generator=g)).to(dtype).to(dev())
        k[0, 1, first + PAGE * P + 5] = (16.0 * u).to(dtype).to(dev())
    sd.sparse_decode(cache, KEEP_ROWS, wide=True)
    for direction, inside in ((u, True), (w, False)):
        qs = queries(direction)
        outs = d.feed(cache, 70, d.text_ids(QUESTION), "update", queries=qs)
        for l, (q, k, v) in enumerate(outs):
            assert torch.equal(q[0], qs[l])
            want, bar = sr.bound(q[0].contiguous(), sr.summaries(cache._layers[l]._k[0], first, n))
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
        cache.rewind(cache.video_end)
        d.t_next = d.t_video
    assert cache.sparse_attention_calls == 2 * LAYERS == sd.sparse_wide_calls(cache)


def test_the_index_survives_a_rewind_and_a_chunk_voids_it():
    Hq = 4
    d = _build("plain", torch.bfloat16, Hq, Hkv, CHUNKS, False)
    cache = d.cache
    sd.sparse_decode(cache, KEEP_ROWS, wide=True)
    built = cache.page_summary_calls
    summ = sd.page_summaries(cache, 1)
    for question in range(2):   # the second follow-up pays nothing: no summary launch, the same index
        outs = d.feed(cache, 50 + question, d.text_ids(QUESTION), "pre_rope")
        for l, (q, k, v) in enumerate(outs):
            cache.attention(q, k, v, layer_idx=l)
        assert cache.sparse_attention_calls == (question + 1) * LAYERS == sd.sparse_wide_calls(cache)
        assert cache.page_summary_calls == built
        cache.rewind(cache.video_end)
        d.t_next = d.t_video
    assert torch.equal(_bits(sd.page_summaries(cache, 1)), _bits(summ))
    # a chunk after arming: the next routed call raises and says what to do
    d.feed(cache, 9, d.video_ids(L), video=True)
    outs = d.feed(cache, 61, d.text_ids(QUESTION), "pre_rope")
    with pytest.raises(ValueError, match="sparse_decode again"):
        cache.attention(*outs[0], layer_idx=0)

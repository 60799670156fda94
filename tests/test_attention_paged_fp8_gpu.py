"""rtk_attention_decode_paged_fp8kv: the packed decode kernel over [listed pages of the e4m3 archive | 16-bit rows].

No tolerance except where stated.  With the identity list the call equals rtk_attention_decode_fp8kv over the archive as it
lies, BIT FOR BIT; with a list that names the partial last page in its last place or not at all - every list the selection
can produce - that call over the index_select-gathered codes and scales (the gathered archive has 32 (keep - 1) + r rows,
padded to 32 keep: the same tiles; the two workspace queries agree, asserted per case); with L8 % 32 == 0,
rtk_attention_decode_paged over [dequantised archive | 16-bit rows].  A list that names the partial page in a middle place
is held to the decode tests' float64 rule on the dequantised gathered rows.  A bad list is the clamped list; NaN behind L8,
behind Lk and in an unlisted page must not show."""
import pytest
import torch

import attention_ref as ar
import sparse_decode_ref as sr
from sparse_decode_ref import code as _code, dequant as _dequant, dev
from test_attention_decode_gpu import _against_fp64, _bits, _plan
from test_sparse_decode_fp8_cpu import refusals_of_the_fp8_paged_calls

pytestmark = pytest.mark.gpu
D, PAGE = 128, 32
SLACK = 37   # rows of every buffer behind its last row
N = PAGE * 9
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


class _Case:
    """q [1, Hq, Lq, D]; an archive of L8 rows and 16-bit buffers of Lk rows, each with SLACK rows of capacity behind."""

    def __init__(self, kind, seed, Hq, Hkv, Lq, L8, Lk, dtype):
        from retake.native_attention import fp8_quantize_rows

        q, k, v = ar.make_inputs(kind, seed, Hq, Hkv, Lq, L8 + Lk, D, dtype, dev())
        self.q, self.L8, self.Lk, self.Hkv, self.dtype = q, L8, Lk, Hkv, dtype
        (k8, ks), (v8, vs) = (fp8_quantize_rows(src[:, :, :L8].contiguous()) for src in (k, v))
        self.k8, self.v8 = sr.with_slack(k8, SLACK), sr.with_slack(v8, SLACK)
        self.ks, self.vs = sr.with_slack(ks, SLACK, 1), sr.with_slack(vs, SLACK, 1)
        self.k, self.v = sr.with_slack(k[:, :, L8:], SLACK), sr.with_slack(v[:, :, L8:], SLACK)

    def archive(self):
        n = self.L8
        return self.k8[:, :, :n], self.v8[:, :, :n], self.ks[:, :, :n], self.vs[:, :, :n]

    def gathered(self, lists):
        """(k8, v8, k_scale, v_scale) of the listed pages' existing rows, [1, Hkv, L', D] / [1, Hkv, L']."""
        return sr.gather_archive((self.k8, self.v8, self.ks, self.vs), self.L8, lists)


def _fp8kv(c, archive, off=None):
    """rtk_attention_decode_fp8kv over `archive` (k8, v8, k_scale, v_scale views) and the case's 16-bit rows."""
    import retake._native as nv

    q, (k8, v8, ks, vs) = c.q, archive
    _, Hq, Lq, _ = q.shape
    Hkv, Lk, L8 = c.Hkv, c.Lk, k8.shape[2]
    need = nv.lib.rtk_attention_decode_workspace_bytes_fp8kv(Hq, Hkv, Lq, Lk, L8, D, _code(q))
    assert need
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    nv.check(nv.lib.rtk_attention_decode_fp8kv(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(c.k), nv.ptr(c.v), c.k.stride(1), c.k.stride(2),
                                               nv.ptr(k8), nv.ptr(v8), nv.ptr(ks), nv.ptr(vs), L8, k8.stride(1), ks.stride(1),
                                               nv.ptr(out), Hq, Hkv, Lq, Lk, Lk - Lq if off is None else off, D, _code(q), D ** -0.5,
                                               nv.ptr(ws), need, nv.stream()), "rtk_attention_decode_fp8kv")
    return out, need


def _paged8(c, lists, off=None):
    """rtk_attention_decode_paged_fp8kv over the case's buffers; lists: [Hkv, keep_pages] ints.  -> (out, partial bytes)"""
    import retake._native as nv

    q = c.q
    _, Hq, Lq, _ = q.shape
    Hkv, Lk, L8 = c.Hkv, c.Lk, c.L8
    lst = torch.as_tensor(lists).to(torch.int32).to(dev()).contiguous()
    keep = lst.shape[1]
    need = nv.lib.rtk_attention_decode_paged_fp8kv_workspace_bytes(Hq, Hkv, Lq, Lk, L8, keep, D, _code(q))
    assert need == _plan(Hkv, PAGE * keep + Lk)[0] * Hq * Lq * (D + 2) * 4, nv.lib.rtk_last_error()
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    sr.call_painted("rtk_attention_decode_paged_fp8kv", need, lambda ws: nv.lib.rtk_attention_decode_paged_fp8kv(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(c.k), nv.ptr(c.v), c.k.stride(1), c.k.stride(2), nv.ptr(c.k8), nv.ptr(c.v8),
        nv.ptr(c.ks), nv.ptr(c.vs), L8, c.k8.stride(1), c.ks.stride(1), nv.ptr(out), Hq, Hkv, Lq, Lk, Lk - Lq if off is None else off, D,
        _code(q), D ** -0.5, nv.ptr(lst), keep, ws, need, nv.stream()))
    return out, need


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Hq", [4, 14])
@pytest.mark.parametrize("L8", [N, N + 5])
def test_the_identity_list_is_the_fp8kv_call_over_the_archive_as_it_lies(dtype, Hq, L8):
    pages = -(-L8 // PAGE)
    for Lk in (3, 40, 72):
        for Lq in (1, 2):
            c = _Case("synth", 17 * Hq + Lk + Lq, Hq, 2, Lq, L8, Lk, dtype)
            got, need = _paged8(c, [list(range(pages))] * 2)
            want, need_dense = _fp8kv(c, c.archive())
            assert need == need_dense
            assert torch.equal(_bits(got), _bits(want)), (dtype, Hq, L8, Lk, Lq)


# lists with the partial last page (page 9 of L8 = N + 5) in the last place or not at all, and lists over whole pages
LISTS = {(N + 5, "one"): [[9], [9]], (N + 5, "one, whole"): [[3], [5]], (N + 5, "four"): [[0, 3, 5, 9], [1, 2, 6, 9]],
         (N + 5, "four, whole"): [[7, 1, 6, 2], [0, 3, 5, 8]], (N + 5, "all"): [list(range(10))] * 2,
         (N, "one"): [[8], [3]], (N, "four"): [[0, 3, 5, 8], [7, 1, 6, 2]], (N, "all"): [list(range(9))] * 2}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Hq", [4, 14])
@pytest.mark.parametrize("which", list(LISTS), ids=[f"L8={k[0]}-{k[1]}" for k in LISTS])
def test_a_list_is_the_fp8kv_call_over_the_gathered_codes_and_scales(dtype, Hq, which):
    L8, lists = which[0], LISTS[which]
    for Lk in (3, 40, 72):
        for Lq in (1, 2):
            c = _Case("synth", 31 * Hq + Lk + Lq, Hq, 2, Lq, L8, Lk, dtype)
            got, need = _paged8(c, lists)
            want, need_gathered = _fp8kv(c, c.gathered(lists))
            assert need == need_gathered, "the plans differ"
            assert torch.equal(_bits(got), _bits(want)), (dtype, Hq, which, Lk, Lq)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_whole_pages_are_the_sixteen_bit_paged_call_over_the_dequantised_archive(dtype):
    import retake._native as nv

    Hq, Hkv, Lq, L8, Lk = 14, 2, 2, N, 40
    c = _Case("synth", 5, Hq, Hkv, Lq, L8, Lk, dtype)
    lists = [[0, 3, 5, 8], [7, 1, 6, 2]]
    got, _ = _paged8(c, lists)
    a = c.archive()
    k16 = torch.cat([_dequant(a[0], a[2], dtype), c.k], dim=2).contiguous()   # [dequantised archive | 16-bit rows | slack]
    v16 = torch.cat([_dequant(a[1], a[3], dtype), c.v], dim=2).contiguous()
    q, lst = c.q, torch.tensor(lists, dtype=torch.int32, device=dev())
    need = nv.lib.rtk_attention_decode_paged_workspace_bytes(Hq, Hkv, Lq, L8 + Lk, 0, L8, 4, D, _code(q))
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    want = torch.empty_like(got)
    nv.check(nv.lib.rtk_attention_decode_paged(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k16), nv.ptr(v16), k16.stride(1),
                                               k16.stride(2), nv.ptr(want), Hq, Hkv, Lq, L8 + Lk, L8 + Lk - Lq, D, _code(q), D ** -0.5,
                                               0, L8, nv.ptr(lst), 4, nv.ptr(ws), need, nv.stream()), "rtk_attention_decode_paged")
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_case_of_three_splits_and_a_wider_query_offset(dtype):
    Hq, Hkv, Lq, L8, Lk = 14, 2, 2, N + 5, 72
    assert _plan(Hkv, PAGE * 10 + Lk)[0] >= 3 and _plan(Hkv, PAGE * 4 + Lk)[0] >= 2
    c = _Case("synth", 3, Hq, Hkv, Lq, L8, Lk, dtype)
    for off in (Lk - Lq, Lk + 5):   # the diagonal inside the 16-bit rows; every row sees every key
        got, _ = _paged8(c, [list(range(10))] * 2, off=off)
        assert torch.equal(_bits(got), _bits(_fp8kv(c, c.archive(), off=off)[0])), off
        lists = LISTS[(N + 5, "four")]
        got, _ = _paged8(c, lists, off=off)
        assert torch.equal(_bits(got), _bits(_fp8kv(c, c.gathered(lists), off=off)[0])), ("four", off)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Hq,Lq", [(4, 1), (4, 2), (14, 1), (14, 2)])
def test_the_partial_page_in_a_middle_place_against_float64(dtype, Hq, Lq):
    Hkv, L8, Lk = 2, N + 5, 3
    lists = [[0, 9, 4], [9, 2, 3]]   # the partial page (5 rows) first and in the middle
    for kind in ("synth", "peaked"):
        c = _Case(kind, 31 * Hq + Lq, Hq, Hkv, Lq, L8, Lk, dtype)
        got, _ = _paged8(c, lists)
        g = c.gathered(lists)
        assert g[0].shape[2] == 2 * PAGE + 5
        kc = torch.cat([_dequant(g[0], g[2], dtype), c.k[:, :, :Lk]], dim=2)
        vc = torch.cat([_dequant(g[1], g[3], dtype), c.v[:, :, :Lk]], dim=2)
        _against_fp64(f"paged fp8 {kind} Hq{Hq} Lq{Lq} {dtype}", c.q, kc, vc, got, dtype)


def test_a_bad_list_is_the_clamped_list():
    c = _Case("synth", 9, 4, 2, 1, N + 5, 3, torch.bfloat16)
    bad, _ = _paged8(c, [[-5, 3, 10 + 7], [2, -1, 1 << 30]])
    good, _ = _paged8(c, [[0, 3, 9], [2, 0, 9]])
    assert torch.equal(_bits(bad), _bits(good))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_that_do_not_exist_contribute_nothing_whatever_they_hold(dtype):
    """NaN codes (0x7F) and NaN scales behind L8 - the rows the partial last page names -, NaN 16-bit rows behind Lk, NaN in
    an unlisted page: the clean and the dirty output are bit-equal."""
    Hq, Hkv, Lq, L8, Lk = 14, 2, 2, N + 5, 40
    lists = [[4, 9], [3, 9]]
    c = _Case("synth", 77, Hq, Hkv, Lq, L8, Lk, dtype)
    clean, _ = _paged8(c, lists)
    for codes, scales in ((c.k8, c.ks), (c.v8, c.vs)):
        codes[:, :, L8:] = 0x7F
        scales[:, :, L8:] = float("nan")
        codes[:, :, :PAGE] = 0x7F          # page 0: in no list
        scales[:, :, :PAGE] = float("nan")
    for t in (c.k, c.v):
        t[:, :, Lk:] = float("nan")
    dirty, _ = _paged8(c, lists)
    assert not torch.isnan(dirty.float()).any()
    assert torch.equal(_bits(clean), _bits(dirty))


def test_refusals_on_device_pointers():
    """Every RTK_EINVAL / RTK_EUNSUPPORTED of the two attention calls, before any launch (the list lives in the CPU test);
    then two of them on real device buffers, whose output and workspace stay as they were."""
    import retake._native as nv

    refusals_of_the_fp8_paged_calls()
    c = _Case("synth", 1, 4, 2, 1, N + 5, 3, torch.bfloat16)
    q = c.q
    lst = torch.zeros((2, 3), dtype=torch.int32, device=dev())
    ws = torch.full((1 << 16,), 0x5a, dtype=torch.uint8, device=dev())
    out = torch.full((1, 1, 4, D), 7.0, dtype=q.dtype, device=dev())
    for change, code in ((dict(off=1), nv.RTK_EINVAL), (dict(keep=11), nv.RTK_EINVAL), (dict(ws_bytes=64), nv.RTK_EINVAL)):
        s = dict(dict(off=2, keep=3, ws_bytes=ws.numel()), **change)
        rc = nv.lib.rtk_attention_decode_paged_fp8kv(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(c.k), nv.ptr(c.v), c.k.stride(1),
                                                     c.k.stride(2), nv.ptr(c.k8), nv.ptr(c.v8), nv.ptr(c.ks), nv.ptr(c.vs), c.L8,
                                                     c.k8.stride(1), c.ks.stride(1), nv.ptr(out), 4, 2, 1, 3, s["off"], D, _code(q),
                                                     D ** -0.5, nv.ptr(lst), s["keep"], nv.ptr(ws), s["ws_bytes"], nv.stream())
        assert rc == code, (change, rc, nv.lib.rtk_last_error())
    torch.cuda.synchronize()
    assert (ws == 0x5a).all() and (out == 7.0).all()

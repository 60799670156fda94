"""rtk_attention_decode_paged_wide / rtk_attention_decode_sparse_wide: the wide packed kernel (16 < G Lq <= 64 packed rows) with
its middle segment read through ONE page list per kv head, shared by all Lq rows.

Aligned shapes (first % 32 == 0, n % 32 == 0) equal, BIT FOR BIT, rtk_attention_decode_wide over
torch.cat([K[:, :first], K pages in list order, K[:, ve:]]); with the identity list, over the rows as they lie.  At most 16
packed rows through the wide entry is the narrow paged call.  Unaligned shapes are held to the decode tests' "2E" rule
against float64 on the gathered rows.  A bad list is the clamped list; NaN behind Lk, in the rows a padded head tile covers,
behind the partial last page and in an unlisted page must not show.  The sparse chain's lists are the rule applied to the
device's own bounds, and its output the paged call's given those lists."""
import pytest
import torch

import sparse_decode_ref as sr
from sparse_decode_ref import code as _code, dev
from test_attention_decode_gpu import _against_fp64, _bits, _plan
from test_attention_paged_gpu import LISTS, N, _make, _paged

pytestmark = pytest.mark.gpu
D, PAGE = 128, 32
# (Hq, Hkv, Lq): R = 21 (NCG 2), 35 (NCG 3), 63 (NCG 4, an idle column), 64 (NCG 4 full), 17 (G 1, one column in the second
# group), 33 (G 1, the diagonal over two tail tiles)
SHAPES = [(14, 2, 3), (14, 2, 5), (14, 2, 9), (16, 2, 8), (2, 2, 17), (2, 2, 33)]
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _wide(q, k, v, off=None):
    """rtk_attention_decode_wide over k / v [1, Hkv, Lk, D] views."""
    import retake._native as nv

    _, Hq, Lq, _ = q.shape
    _, Hkv, Lk, _ = k.shape
    need = nv.lib.rtk_attention_decode_wide_workspace_bytes(Hq, Hkv, Lq, Lk, D, _code(q))
    assert need, nv.lib.rtk_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    nv.check(nv.lib.rtk_attention_decode_wide(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2),
                                              nv.ptr(out), Hq, Hkv, Lq, Lk, Lk - Lq if off is None else off, D, _code(q), D ** -0.5,
                                              nv.ptr(ws), need, nv.stream()), "rtk_attention_decode_wide")
    return out


def _paged_wide(q, k, v, Lk, first, ve, lists, off=None):
    """rtk_attention_decode_paged_wide over the buffers k / v [1, Hkv, cap, D]; lists: int tensor [Hkv, keep_pages]."""
    import retake._native as nv

    _, Hq, Lq, _ = q.shape
    Hkv, keep = k.shape[1], lists.shape[1]
    lst = lists.to(torch.int32).to(dev()).contiguous()
    need = nv.lib.rtk_attention_decode_paged_wide_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, _code(q))
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    sr.call_painted("rtk_attention_decode_paged_wide", need, lambda ws: nv.lib.rtk_attention_decode_paged_wide(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2), nv.ptr(out), Hq, Hkv, Lq, Lk,
        Lk - Lq if off is None else off, D, _code(q), D ** -0.5, first, ve, nv.ptr(lst), keep, ws, need, nv.stream()))
    return out


@DTYPES
@pytest.mark.parametrize("Hq,Hkv,Lq", SHAPES)
def test_aligned_shapes_are_the_wide_call_over_the_concatenation(dtype, Hq, Hkv, Lq):
    for first in (0, 32):
        for tail in (Lq - 1, 40):   # Lq - 1: the edge q_offset = ve - 1
            ve = first + N
            Lk = ve + tail
            q, k, v = _make(17 * Hq + first + tail + Lq, Hq, Hkv, Lq, Lk, dtype)
            for which in LISTS:
                lists = torch.tensor(LISTS[which])
                got = _paged_wide(q, k, v, Lk, first, ve, lists)
                kc, vc = sr.gather(k, v, first, ve, Lk, lists)
                assert torch.equal(_bits(got), _bits(_wide(q, kc, vc))), (dtype, Hq, Lq, first, tail, which)
                if which == "all":   # the identity list: the rows as they lie, no copy
                    assert torch.equal(_bits(got), _bits(_wide(q, k[:, :, :Lk], v[:, :, :Lk]))), "identity list"


@DTYPES
def test_at_most_16_rows_through_the_wide_entry_is_the_narrow_paged_call(dtype):
    Hq, Hkv, Lq, first, tail = 4, 2, 2, 32, 3
    ve = first + N
    Lk = ve + tail
    q, k, v = _make(5, Hq, Hkv, Lq, Lk, dtype)
    lists = torch.tensor(LISTS["four"])
    assert torch.equal(_bits(_paged_wide(q, k, v, Lk, first, ve, lists)), _bits(_paged(q, k, v, Lk, first, ve, lists)))


@DTYPES
@pytest.mark.parametrize("Hq,Hkv,Lq", [(14, 2, 5), (2, 2, 33)])
def test_a_case_of_three_splits_and_a_wider_query_offset(dtype, Hq, Hkv, Lq):
    first, tail = 32, 40
    ve = first + N
    Lk = ve + tail
    assert _plan(Hkv, first + N + tail)[0] >= 3
    q, k, v = _make(3, Hq, Hkv, Lq, Lk, dtype)
    lists = torch.tensor(LISTS["all"])
    for off in (Lk - Lq, Lk + 5):   # the diagonal inside the tail; every row sees every key
        got = _paged_wide(q, k, v, Lk, first, ve, lists, off=off)
        assert torch.equal(_bits(got), _bits(_wide(q, k[:, :, :Lk], v[:, :, :Lk], off=off))), off


@DTYPES
@pytest.mark.parametrize("Hq,Hkv,Lq", SHAPES)
def test_unaligned_shapes_against_float64(dtype, Hq, Hkv, Lq):
    first, n, tail = 5, N + 5, max(3, Lq - 1)
    ve = first + n
    Lk = ve + tail
    lists = torch.tensor([[0, 4, 9], [2, 3, 9]])   # both name the partial last page (5 rows)
    for kind, gain in (("synth", 1.0), ("peaked", 8.0)):
        q, k, v = _make(31 * Hq + Lq, Hq, Hkv, Lq, Lk, dtype, gain)
        got = _paged_wide(q, k, v, Lk, first, ve, lists)
        kc, vc = sr.gather(k, v, first, ve, Lk, lists)
        assert kc.shape[2] == first + 2 * PAGE + 5 + tail
        _against_fp64(f"paged wide {kind} Hq{Hq} Lq{Lq} {dtype}", q, kc, vc, got, dtype)


@pytest.mark.parametrize("Hq,Hkv,Lq", [(14, 2, 3), (16, 2, 8)])
def test_a_bad_list_is_the_clamped_list(Hq, Hkv, Lq):
    first, tail = 32, Lq + 2
    ve = first + N
    Lk = ve + tail
    q, k, v = _make(9, Hq, Hkv, Lq, Lk, torch.bfloat16)
    bad = _paged_wide(q, k, v, Lk, first, ve, torch.tensor([[-5, 3, 9 + 7], [2, -1, 1 << 30]]))
    good = _paged_wide(q, k, v, Lk, first, ve, torch.tensor([[0, 3, 8], [2, 0, 8]]))
    assert torch.equal(_bits(bad), _bits(good))


@DTYPES
@pytest.mark.parametrize("Hq,Hkv,Lq", [(14, 2, 5), (2, 2, 33)])
def test_rows_that_do_not_exist_contribute_nothing_whatever_they_hold(dtype, Hq, Hkv, Lq):
    """NaN behind Lk; with first = 5 the head tile covers buffer rows 5 .. 31 - region rows (page 0) the list does not name;
    NaN in another unlisted page; NaN right behind the partial last page (Lk = ve: no tail row between).  None may reach
    the output: clean and dirty are bit-equal."""
    first, n = 5, N + 5
    ve = first + n
    lists = torch.tensor([[4, 9], [3, 9]])
    q, k, v = _make(77, Hq, Hkv, Lq, ve + Lq - 1, dtype)
    kd, vd = k.clone(), v.clone()
    for t in (kd, vd):
        t[:, :, first:first + PAGE] = float("nan")                    # page 0: buffer rows 5 .. 36
        t[:, :, first + 6 * PAGE:first + 7 * PAGE] = float("nan")     # page 6: in neither list
    for Lk in (ve + Lq - 1, ve):   # the edge q_offset = ve - 1 with a tail, and with none: NaN right behind the last page
        clean = _paged_wide(q, k, v, Lk, first, ve, lists, off=ve - 1)
        for t in (kd, vd):
            t[:, :, Lk:] = float("nan")
        dirty = _paged_wide(q, kd, vd, Lk, first, ve, lists, off=ve - 1)
        assert not torch.isnan(dirty.float()).any()
        assert torch.equal(_bits(clean), _bits(dirty)), Lk


@DTYPES
@pytest.mark.parametrize("Hq,Hkv,Lq", [(14, 2, 3), (14, 2, 9), (2, 2, 33)])
def test_the_sparse_chain_is_bound_then_selection_then_the_paged_call(dtype, Hq, Hkv, Lq):
    import retake._native as nv

    first, n, tail, keep = 5, N + 5, Lq + 1, 4
    ve, pages = first + n, sr.pages_of(N + 5)
    Lk = ve + tail
    q, k, v = _make(41 * Hq + Lq, Hq, Hkv, Lq, Lk, dtype)
    summ = sr.summaries(k[0], first, n).to(dev()).contiguous()
    need = nv.lib.rtk_attention_decode_sparse_wide_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, _code(q))
    a16 = lambda b: -(-b // 16) * 16   # noqa: E731
    partials = nv.lib.rtk_attention_decode_paged_wide_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, _code(q))
    assert need == a16(Hkv * pages * 4) + a16(Hkv * keep * 4) + partials
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev())
    ws[need:] = 0x5a
    out = torch.empty((1, Lq, Hq, D), dtype=dtype, device=dev())
    nv.check(nv.lib.rtk_attention_decode_sparse_wide(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2), nv.ptr(out), Hq, Hkv, Lq, Lk, Lk - Lq, D,
        _code(q), D ** -0.5, first, ve, nv.ptr(summ), summ.stride(0), keep, nv.ptr(ws), need, nv.stream()),
        "rtk_attention_decode_sparse_wide")
    torch.cuda.synchronize()
    assert (ws[need:] == 0x5a).all(), "the call wrote behind its workspace"
    ub = ws[:Hkv * pages * 4].view(torch.float32).view(Hkv, pages).clone()
    at = a16(Hkv * pages * 4)
    lists = ws[at:at + Hkv * keep * 4].view(torch.int32).view(Hkv, keep).clone()
    want, bar = sr.bound(q[0], summ)   # the max runs over the packed rows of every position
    assert ((ub.double().cpu() - want).abs() <= bar).all()
    assert torch.equal(lists.cpu(), sr.select(ub, keep))
    assert torch.equal(_bits(out), _bits(_paged_wide(q, k, v, Lk, first, ve, lists)))


def test_refusals_on_device_pointers():
    """Every RTK_EINVAL / RTK_EUNSUPPORTED of the two wide calls, before any launch (the list lives in the CPU test)."""
    from test_sparse_decode_wide_cpu import refusals_of_the_wide_paged_calls

    refusals_of_the_wide_paged_calls()

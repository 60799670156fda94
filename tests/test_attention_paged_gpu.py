"""rtk_attention_decode_paged: the packed decode kernel with its middle segment read through a page list.

Aligned shapes (first % 32 == 0, n % 32 == 0) equal, BIT FOR BIT, rtk_attention_decode over
torch.cat([K[:, :first], K pages in list order, K[:, ve:]]); with the identity list, over the rows as they lie.  Unaligned
shapes are held to the decode tests' "2E" rule against float64 on the gathered rows.  A bad list is the clamped list; NaN
behind Lk, and in the rows a padded head tile would touch, must not show."""
import pytest
import torch

import sparse_decode_ref as sr
from sparse_decode_ref import code as _code, dev
from test_attention_decode_gpu import _against_fp64, _bits, _plan
from test_sparse_decode_cpu import refusals_of_the_paged_calls

pytestmark = pytest.mark.gpu
D, PAGE = 128, 32
SLACK = 37   # rows of the buffers behind Lk


def _make(seed, Hq, Hkv, Lq, Lk, dtype, q_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    q = (q_gain * 1.7 * torch.randn((1, Hq, Lq, D), generator=g)).to(dtype).to(dev())
    k = (1.7 * torch.randn((1, Hkv, Lk + SLACK, D), generator=g)).to(dtype).to(dev())
    v = (1.7 * torch.randn((1, Hkv, Lk + SLACK, D), generator=g)).to(dtype).to(dev())
    return q, k, v


def _dense(q, k, v, off=None):
    """rtk_attention_decode over k / v [1, Hkv, Lk, D] views."""
    import retake._native as nv

    _, Hq, Lq, _ = q.shape
    _, Hkv, Lk, _ = k.shape
    need = nv.lib.rtk_attention_decode_workspace_bytes(Hq, Hkv, Lq, Lk, D, _code(q))
    assert need
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    nv.check(nv.lib.rtk_attention_decode(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2),
                                         nv.ptr(out), Hq, Hkv, Lq, Lk, Lk - Lq if off is None else off, D, _code(q), D ** -0.5,
                                         nv.ptr(ws), need, nv.stream()), "rtk_attention_decode")
    return out


def _paged(q, k, v, Lk, first, ve, lists, off=None):
    """rtk_attention_decode_paged over the buffers k / v [1, Hkv, cap, D]; lists: int tensor [Hkv, keep_pages]."""
    import retake._native as nv

    _, Hq, Lq, _ = q.shape
    Hkv, keep = k.shape[1], lists.shape[1]
    lst = lists.to(torch.int32).to(dev()).contiguous()
    need = nv.lib.rtk_attention_decode_paged_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, _code(q))
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    sr.call_painted("rtk_attention_decode_paged", need, lambda ws: nv.lib.rtk_attention_decode_paged(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2), nv.ptr(out), Hq, Hkv, Lq, Lk,
        Lk - Lq if off is None else off, D, _code(q), D ** -0.5, first, ve, nv.ptr(lst), keep, ws, need, nv.stream()))
    return out


N = PAGE * 9
LISTS = {"one": [[8], [3]], "four": [[0, 3, 5, 8], [7, 1, 6, 2]], "all": [list(range(9))] * 2}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Hq", [4, 14])
@pytest.mark.parametrize("first", [0, 32])
@pytest.mark.parametrize("tail", [0, 3, 40])
@pytest.mark.parametrize("which", list(LISTS))
def test_aligned_shapes_are_the_packed_call_over_the_concatenation(dtype, Hq, first, tail, which):
    Hkv, ve = 2, first + N
    Lk = ve + tail
    lists = torch.tensor(LISTS[which])
    for Lq in (1, 2):
        if Lq == 2 and tail < 1:
            continue   # Lq 2 needs q_offset = Lk - 2 >= ve - 1: at least one tail row
        q, k, v = _make(17 * Hq + first + tail + Lq, Hq, Hkv, Lq, Lk, dtype)
        got = _paged(q, k, v, Lk, first, ve, lists)
        kc, vc = sr.gather(k, v, first, ve, Lk, lists)
        want = _dense(q, kc, vc)
        assert torch.equal(_bits(got), _bits(want)), (dtype, Hq, first, tail, which, Lq)
        if which == "all":   # the identity list: the rows as they lie, no copy
            assert torch.equal(_bits(got), _bits(_dense(q, k[:, :, :Lk], v[:, :, :Lk]))), "identity list"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_case_of_three_splits_and_a_wider_query_offset(dtype):
    Hq, Hkv, first, tail = 14, 2, 32, 40
    ve = first + N
    Lk = ve + tail
    assert _plan(Hkv, first + N + tail)[0] >= 3
    q, k, v = _make(3, Hq, Hkv, 2, Lk, dtype)
    lists = torch.tensor(LISTS["all"])
    for off in (Lk - 2, Lk + 5):   # the diagonal inside the tail; every row sees every key
        got = _paged(q, k, v, Lk, first, ve, lists, off=off)
        assert torch.equal(_bits(got), _bits(_dense(q, k[:, :, :Lk], v[:, :, :Lk], off=off))), off


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Hq,Lq", [(4, 1), (4, 2), (14, 1), (14, 2)])
def test_unaligned_shapes_against_float64(dtype, Hq, Lq):
    Hkv, first, n, tail = 2, 5, N + 5, 3
    ve = first + n
    Lk = ve + tail
    lists = torch.tensor([[0, 4, 9], [2, 3, 9]])   # both name the partial last page (5 rows)
    for kind, gain in (("synth", 1.0), ("peaked", 8.0)):
        q, k, v = _make(31 * Hq + Lq, Hq, Hkv, Lq, Lk, dtype, gain)
        got = _paged(q, k, v, Lk, first, ve, lists)
        kc, vc = sr.gather(k, v, first, ve, Lk, lists)
        assert kc.shape[2] == first + 2 * PAGE + 5 + tail
        _against_fp64(f"paged {kind} Hq{Hq} Lq{Lq} {dtype}", q, kc, vc, got, dtype)


def test_a_bad_list_is_the_clamped_list():
    Hq, Hkv, first, tail = 4, 2, 32, 3
    ve = first + N
    Lk = ve + tail
    q, k, v = _make(9, Hq, Hkv, 1, Lk, torch.bfloat16)
    bad = _paged(q, k, v, Lk, first, ve, torch.tensor([[-5, 3, 9 + 7], [2, -1, 1 << 30]]))
    good = _paged(q, k, v, Lk, first, ve, torch.tensor([[0, 3, 8], [2, 0, 8]]))
    assert torch.equal(_bits(bad), _bits(good))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rows_that_do_not_exist_contribute_nothing_whatever_they_hold(dtype):
    """NaN behind Lk; and with first = 5 the head tile covers buffer rows 5 .. 31 - region rows (page 0) the list does not
    name: NaN there, in K and V, must not reach the output.  Neither must NaN behind the partial last page."""
    Hq, Hkv, first, n, tail = 14, 2, 5, N + 5, 3
    ve = first + n
    Lk = ve + tail
    lists = torch.tensor([[4, 9], [3, 9]])
    q, k, v = _make(77, Hq, Hkv, 2, Lk, dtype)
    clean = _paged(q, k, v, Lk, first, ve, lists)
    for t in (k, v):
        t[:, :, Lk:] = float("nan")
        t[:, :, first:first + PAGE] = float("nan")   # page 0: buffer rows 5 .. 36
    dirty = _paged(q, k, v, Lk, first, ve, lists)
    assert not torch.isnan(dirty.float()).any()
    assert torch.equal(_bits(clean), _bits(dirty))
    # no tail at all (Lk = ve, Lq 1, offset ve - 1): the rows right behind the partial last page hold NaN
    q1 = q[:, :, :1].contiguous()
    k2, v2 = k.clone(), v.clone()
    for t in (k2, v2):
        t[:, :, first:first + PAGE] = 1.0
        t[:, :, ve:] = float("nan")
    seen = _paged(q1, k2, v2, ve, first, ve, lists, off=ve - 1)
    assert not torch.isnan(seen.float()).any()


def test_refusals_on_device_pointers():
    """Every RTK_EINVAL / RTK_EUNSUPPORTED of the two attention calls, before any launch (the list lives in the CPU test)."""
    refusals_of_the_paged_calls()

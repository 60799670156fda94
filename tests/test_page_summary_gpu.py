"""rtk_pivotkv_page_summary_batched against torch.amax / amin per page (and tests/sparse_decode_ref.py), bit for bit: partial
pages, pinned rows in front, a head stride larger than the rows, several units of different n in one call, an empty unit;
NaN rows planted right outside the region must not show; guard bytes around the output stay."""
import pytest
import torch

import sparse_decode_ref as sr

pytestmark = pytest.mark.gpu
D, PAGE = 128, 32
GUARD = 64   # elements in front of and behind every head's summaries


def dev():
    return torch.device("cuda:0")


def _code(dtype):
    import retake._native as nv

    return nv.RTK_BF16 if dtype is torch.bfloat16 else nv.RTK_F16


def _unit(seed, Hkv, first, n, cap, dtype):
    """K [Hkv, cap, D] with NaN rows at first - 1 and first + n, and a guarded output buffer."""
    g = torch.Generator().manual_seed(seed)
    K = (1.7 * torch.randn((Hkv, cap, D), generator=g)).to(dtype).to(dev())
    if first > 0:
        K[:, first - 1] = float("nan")
    if first + n < cap:
        K[:, first + n] = float("nan")
    pages = sr.pages_of(n)
    stride = pages * 2 * D + 2 * GUARD
    buf = torch.full((Hkv * stride,), 7.0, dtype=dtype, device=dev())
    return K, buf, stride, pages


def _run(units, Hkv, dtype):
    import retake._native as nv

    arr = (nv.PageSummaryUnit * len(units))()
    for u, (K, buf, stride, pages, first, n) in zip(arr, units):
        u.k, u.k_stride_h, u.first, u.n = K.data_ptr(), K.stride(0), first, n
        u.summ, u.summ_stride_h = buf.data_ptr() + GUARD * 2, stride
    nv.check(nv.lib.rtk_pivotkv_page_summary_batched(arr, len(units), Hkv, D, _code(dtype), nv.stream()), "summary")
    torch.cuda.synchronize()


def _check(K, buf, stride, pages, first, n, what):
    Hkv = K.shape[0]
    got = buf.view(Hkv, stride)
    assert torch.equal(got[:, :GUARD], torch.full_like(got[:, :GUARD], 7.0)), (what, "guard in front")
    assert torch.equal(got[:, GUARD + pages * 2 * D:], torch.full_like(got[:, GUARD + pages * 2 * D:], 7.0)), (what, "guard behind")
    if n == 0:
        return
    got = got[:, GUARD:GUARD + pages * 2 * D].reshape(Hkv, pages, 2, D)
    assert not torch.isnan(got.float()).any(), (what, "a NaN row outside the region showed")
    for p in range(pages):
        rows = K[:, first + PAGE * p:first + min(PAGE * p + PAGE, n)]
        assert torch.equal(got[:, p, 0], rows.amax(dim=1)) and torch.equal(got[:, p, 1], rows.amin(dim=1)), (what, "page", p)
    want = sr.summaries(K, first, n).to(dev())
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (what, "against the reference rule")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("first", [0, 7, 32])
def test_summaries_are_amax_and_amin_per_page(dtype, Hkv, first):
    for i, n in enumerate([1, 31, 32, 33, 32 * 3 + 5]):
        K, buf, stride, pages = _unit(100 * first + i, Hkv, first, n, first + n + 9, dtype)   # (head stride > the rows)
        _run([(K, buf, stride, pages, first, n)], Hkv, dtype)
        _check(K, buf, stride, pages, first, n, (dtype, Hkv, first, n))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_units_of_different_n_and_an_empty_unit_in_one_call(dtype):
    Hkv = 2
    specs = [(7, 32 * 3 + 5), (0, 33), (5, 0), (32, 32 * 9)]
    units = []
    for i, (first, n) in enumerate(specs):
        K, buf, stride, pages = _unit(900 + i, Hkv, first, n, first + n + 3, dtype)
        units.append((K, buf, stride, pages, first, n))
    _run(units, Hkv, dtype)
    for u, spec in zip(units, specs):
        _check(*u, (dtype, spec))


def test_signed_zeros_follow_the_stated_rule():
    """Of -0 and +0 the max is +0 and the min -0, whatever their order in the page."""
    import retake._native as nv

    K = torch.zeros((1, 4, D), dtype=torch.bfloat16, device=dev())
    K[0, 1] = -0.0
    K[0, 3, :64] = -0.0
    buf = torch.full((2 * D,), 7.0, dtype=torch.bfloat16, device=dev())
    u = (nv.PageSummaryUnit * 1)()
    u[0].k, u[0].k_stride_h, u[0].first, u[0].n, u[0].summ, u[0].summ_stride_h = K.data_ptr(), K.stride(0), 0, 4, buf.data_ptr(), 2 * D
    nv.check(nv.lib.rtk_pivotkv_page_summary_batched(u, 1, 1, D, nv.RTK_BF16, nv.stream()), "summary")
    bits = buf.view(torch.int16).view(2, D)
    assert (bits[0] == 0).all() and (bits[1] == -32768).all()

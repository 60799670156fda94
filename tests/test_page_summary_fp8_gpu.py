"""rtk_pivotkv_page_summary_fp8k_batched against torch.amax / amin per page over rtk_fp8kv_dequant of the same codes and scales
(and the ordered rule of tests/sparse_decode_ref.py), as int16 bits, bf16 / fp16: partial pages and a page of one row, -0 beside
+0, code 0x7F (NaN) and NaN scales right behind n that must not be read, guard bytes around the output, two units of different
n in one call, bits independent of strides."""
import pytest
import torch

import sparse_decode_ref as sr

pytestmark = pytest.mark.gpu
D, PAGE = 128, 32
GUARD = 64   # elements in front of and behind every head's summaries
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def dev():
    return torch.device("cuda:0")


def _archive(seed, Hkv, n, cap, dtype):
    """Codes [1, Hkv, cap, D] and scales [1, Hkv, cap] of random rows; rows >= n hold code 0x7F (NaN) and NaN scales."""
    from retake.native_attention import fp8_quantize_rows

    g = torch.Generator().manual_seed(seed)
    x = (1.7 * torch.randn((1, Hkv, cap, D), generator=g) * torch.rand((1, Hkv, cap, 1), generator=g)).to(dtype).to(dev())
    codes, scales = fp8_quantize_rows(x)
    codes[:, :, n:] = 0x7F
    scales[:, :, n:] = float("nan")
    return codes, scales


def _out(Hkv, pages, dtype, guard=GUARD):
    stride = pages * 2 * D + 2 * guard
    return torch.full((Hkv * stride,), 7.0, dtype=dtype, device=dev()), stride


def _run(units, Hkv, dtype, guard=GUARD):
    """units: [(codes, scales, n, buf, stride)]"""
    import retake._native as nv

    arr = (nv.PageSummaryFp8kUnit * len(units))()
    for u, (codes, scales, n, buf, stride) in zip(arr, units):
        u.k8, u.k8_stride_h, u.k_scale, u.scale_stride_h, u.n = codes.data_ptr(), codes.stride(1), scales.data_ptr(), scales.stride(1), n
        u.summ, u.summ_stride_h = buf.data_ptr() + guard * 2, stride
    code = nv.RTK_BF16 if dtype is torch.bfloat16 else nv.RTK_F16
    nv.check(nv.lib.rtk_pivotkv_page_summary_fp8k_batched(arr, len(units), Hkv, D, code, nv.stream()), "summary")
    torch.cuda.synchronize()


def _check(codes, scales, n, buf, stride, dtype, what, guard=GUARD):
    """-> the summaries [Hkv, pages, 2, D]"""
    from retake.native_attention import fp8_dequantize_rows

    Hkv, pages = codes.shape[1], sr.pages_of(n)
    got = buf.view(Hkv, stride)
    assert torch.equal(got[:, :guard], torch.full_like(got[:, :guard], 7.0)), (what, "guard in front")
    assert torch.equal(got[:, guard + pages * 2 * D:], torch.full_like(got[:, guard + pages * 2 * D:], 7.0)), (what, "guard behind")
    got = got[:, guard:guard + pages * 2 * D].reshape(Hkv, pages, 2, D)
    assert not torch.isnan(got.float()).any(), (what, "a row behind n was read")
    K = fp8_dequantize_rows(codes[:, :, :n].contiguous(), scales[:, :, :n].contiguous(), dtype)[0]   # [Hkv, n, D]
    for p in range(pages):
        rows = K[:, PAGE * p:min(PAGE * p + PAGE, n)]
        assert torch.equal(got[:, p, 0].view(torch.int16), rows.amax(dim=1).view(torch.int16)), (what, "max of page", p)
        assert torch.equal(got[:, p, 1].view(torch.int16), rows.amin(dim=1).view(torch.int16)), (what, "min of page", p)
    want = sr.summaries(K, 0, n).to(dev())
    assert torch.equal(got.contiguous().view(torch.int16), want.view(torch.int16)), (what, "against the ordered rule")
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Hkv", [2, 1])
def test_summaries_are_amax_and_amin_of_the_dequantised_rows(dtype, Hkv):
    for i, n in enumerate([1, 31, 32, 33, PAGE * 9, PAGE * 9 + 5]):   # 33: a page of one row
        codes, scales = _archive(10 * Hkv + i, Hkv, n, n + 9, dtype)    # (head strides > the rows)
        buf, stride = _out(Hkv, sr.pages_of(n), dtype)
        _run([(codes, scales, n, buf, stride)], Hkv, dtype)
        _check(codes, scales, n, buf, stride, dtype, (dtype, Hkv, n))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_units_of_different_n_and_an_empty_one_in_one_call(dtype):
    Hkv = 2
    units = []
    for i, n in enumerate([PAGE * 3 + 5, 0, PAGE * 9]):
        codes, scales = _archive(900 + i, Hkv, n, n + 3, dtype)
        buf, stride = _out(Hkv, sr.pages_of(n), dtype)
        units.append((codes, scales, n, buf, stride))
    _run(units, Hkv, dtype)
    for u in units:
        if u[2]:
            _check(*u, dtype, (dtype, u[2]))
        else:
            assert (u[3] == 7.0).all(), "an empty unit was written"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_bits_do_not_depend_on_strides(dtype):
    Hkv, n = 2, PAGE * 3 + 5
    codes, scales = _archive(5, Hkv, n, n + 9, dtype)
    buf, stride = _out(Hkv, sr.pages_of(n), dtype)
    _run([(codes, scales, n, buf, stride)], Hkv, dtype)
    a = _check(codes, scales, n, buf, stride, dtype, "first layout")
    # the same rows in buffers of another capacity (other head strides, another base address), the output without guards
    codes2 = torch.full((1, Hkv, n + 40, D), 0x7F, dtype=torch.uint8, device=dev())
    scales2 = torch.full((1, Hkv, n + 40), float("nan"), dtype=torch.float32, device=dev())
    codes2[:, :, :n], scales2[:, :, :n] = codes[:, :, :n], scales[:, :, :n]
    buf2, stride2 = _out(Hkv, sr.pages_of(n), dtype, guard=0)
    _run([(codes2, scales2, n, buf2, stride2)], Hkv, dtype, guard=0)
    b = _check(codes2, scales2, n, buf2, stride2, dtype, "second layout", guard=0)
    assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_signed_zeros_follow_the_stated_rule(dtype):
    """Code 0x80 (-0) beside 0x00 (+0): the max is +0 and the min -0, whatever their order in the page."""
    n = 4
    codes = torch.zeros((1, 1, n + 2, D), dtype=torch.uint8, device=dev())
    codes[0, 0, 1] = 0x80
    codes[0, 0, 3, :64] = 0x80
    codes[0, 0, n:] = 0x7F
    scales = torch.ones((1, 1, n + 2), dtype=torch.float32, device=dev())
    scales[0, 0, n:] = float("nan")
    buf, stride = _out(1, 1, dtype)
    _run([(codes, scales, n, buf, stride)], 1, dtype)
    bits = buf[GUARD:GUARD + 2 * D].view(torch.int16).view(2, D)
    assert (bits[0] == 0).all() and (bits[1] == -32768).all()
    assert (buf[:GUARD] == 7.0).all() and (buf[GUARD + 2 * D:] == 7.0).all()

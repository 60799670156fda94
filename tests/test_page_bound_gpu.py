"""rtk_attention_page_bound: against float64 under the derived bar of an fp32 sum of 128 exact products,
128 * 2^-24 * sum_d |term_d| per entry (the measured error is printed beside it); the upper-bound property - no float64
logit of a page exceeds ub + bar; bits independent of strides and addresses.  G 1, 2, 7; Lq 1 and 2; pages 1, 9 and 65."""
import pytest
import torch

import sparse_decode_ref as sr

pytestmark = pytest.mark.gpu
D, PAGE = 128, 32


def dev():
    return torch.device("cuda:0")


def _bound(q, summ, pages):
    """q [Hq, Lq, D] and summ [Hkv, pages, 2, D] views, read where they lie -> ub fp32 [Hkv, pages]."""
    import retake._native as nv

    Hq, Lq, _ = q.shape
    Hkv = summ.shape[0]
    ub = torch.full((Hkv * pages + 8,), -7.0, dtype=torch.float32, device=dev())
    code = nv.RTK_BF16 if q.dtype is torch.bfloat16 else nv.RTK_F16
    nv.check(nv.lib.rtk_attention_page_bound(nv.ptr(q), q.stride(0), q.stride(1), nv.ptr(summ), summ.stride(0), Hq, Hkv, Lq, pages,
                                             D, code, nv.ptr(ub), nv.stream()), "rtk_attention_page_bound")
    torch.cuda.synchronize()
    assert (ub[Hkv * pages:] == -7.0).all(), "the kernel wrote behind ub"
    return ub[:Hkv * pages].view(Hkv, pages).clone()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("G", [1, 2, 7])
@pytest.mark.parametrize("Lq", [1, 2])
@pytest.mark.parametrize("pages", [1, 9, 65])
def test_bound_against_float64_and_the_upper_bound_property(dtype, G, Lq, pages):
    Hkv = 2
    Hq, n = G * Hkv, PAGE * pages - 5 if pages > 1 else 7
    g = torch.Generator().manual_seed(1000 * G + 10 * pages + Lq)
    q = (1.7 * torch.randn((Hq, Lq, D), generator=g)).to(dtype).to(dev())
    K = (1.7 * torch.randn((Hkv, n, D), generator=g)).to(dtype).to(dev())
    summ = sr.summaries(K, 0, n).to(dev())
    got = _bound(q, summ, pages)
    want, bar = sr.bound(q, summ)
    err = (got.double().cpu() - want).abs()
    print(f"bound[{dtype}, G {G}, Lq {Lq}, pages {pages}]: max error {err.max().item():.3e}, smallest bar {bar.min().item():.3e}, "
          f"largest error / bar {(err / bar).max().item():.3f}")
    assert (err <= bar).all()
    # every raw float64 logit of every packed row of the group against every key of the page
    logits = torch.einsum("grd,gjd->grj", q.double().cpu().view(Hkv, G * Lq, D), K.double().cpu())   # [Hkv, R, n]
    for p in range(pages):
        top = logits[:, :, PAGE * p:min(PAGE * p + PAGE, n)].amax(dim=(1, 2))
        assert (top <= got[:, p].double().cpu() + bar[:, p]).all(), ("page", p)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bits_do_not_depend_on_strides_or_addresses(dtype):
    Hkv, G, Lq, pages = 2, 7, 2, 9
    Hq = G * Hkv
    g = torch.Generator().manual_seed(5)
    q = (1.7 * torch.randn((Hq, Lq, D), generator=g)).to(dtype).to(dev())
    summ = (1.7 * torch.randn((Hkv, pages, 2, D), generator=g)).to(dtype).to(dev())
    summ = torch.stack([summ.amax(2), summ.amin(2)], 2).contiguous()
    base = _bound(q, summ, pages)
    # q as the transposed view of a [Lq, Hq * D] projection output, with an offset; summ inside a larger, shifted buffer
    proj = torch.zeros((Lq + 1, Hq * D + 64), dtype=dtype, device=dev())
    q2 = proj[1:, 8:8 + Hq * D].view(Lq, Hq, D).transpose(0, 1)
    q2.copy_(q)
    big = torch.zeros((Hkv, pages + 3, 2, D), dtype=dtype, device=dev())
    s2 = big[:, 1:1 + pages]
    s2.copy_(summ)
    assert q2.stride() != q.stride() and s2.stride(0) != summ.stride(0)
    again = _bound(q2, s2, pages)
    assert torch.equal(base.view(torch.int32), again.view(torch.int32))

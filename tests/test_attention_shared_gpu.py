"""rtk_attention_forward_shared / rtk_attention_decode_shared on the GPU: the keys are [archive | shared 16-bit rows of
another buffer | own 16-bit rows].  Every case is compared with the EXISTING entry point on a concatenated copy of
[shared | own] - never with the code under test:
  * Ls a multiple of the key tile (64 chunk kernel, 32 packed decode kernel), any L8: bit for bit;
  * elsewhere the own rows start a new key tile, the fp32 sums are grouped differently, and the bar is the one
    tests/test_attention_gpu.py applies to the 16-bit kernel: within max(2 E, half an ulp of the output dtype at the output's
    magnitude) of float64 on the same inputs - E the eager expression's error, the archive dequantised by fp8_dequantize_rows.
Inputs: tests/synth.py through tests/attention_ref.py."""
import itertools

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

D = 128


def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _segments(seed, Hq, Hkv, Lq, Lk, Ls, L8, dtype):
    """One sequence of L8 + Ls + Lk keys cut three ways.  Returns q, the archive of the first L8 rows (None without one), the
    shared rows as views of a buffer of their own (other strides than the own rows'), the own rows and the concatenated
    [shared | own] rows as views of the sequence, and the dense [dequantised archive | shared | own] rows."""
    import retake.longvideo_cache as lc

    total = L8 + Ls + Lk
    q, k, v = ar.make_inputs("synth", seed, Hq, Hkv, Lq, total, D, dtype, dev())
    archive, dense = None, [k, v]
    if L8:
        ck, sk = lc.fp8_quantize_rows(k[:, :, :L8].contiguous())
        cv, sv = lc.fp8_quantize_rows(v[:, :, :L8].contiguous())
        archive = (ck, cv, sk, sv)
        dense = [torch.cat([lc.fp8_dequantize_rows(c, s, dtype), t[:, :, L8:]], dim=2) for c, s, t in ((ck, sk, k), (cv, sv, v))]
    shared = []
    for t in (k, v):
        buf = torch.full((1, Hkv, Ls + 7, D), float("nan"), dtype=dtype, device=dev())   # rows past Ls must never be read
        buf[:, :, :Ls].copy_(t[:, :, L8:L8 + Ls])
        shared.append(buf[:, :, :Ls])
    own = (k[:, :, L8 + Ls:], v[:, :, L8 + Ls:])
    cat = (k[:, :, L8:], v[:, :, L8:])
    return q, archive, tuple(shared), own, cat, dense


def _check(tag, q, archive, shared, own, cat, dense, tile, packed, offset=None, want_route=None):
    """The call under test against the existing call over the concatenation: bitwise when Ls is a multiple of `tile`,
    else both against float64."""
    import retake.longvideo_cache as lc

    dtype, Ls = q.dtype, shared[0].shape[2]
    route, route_ref = [], []
    got = lc.chunk_attention(q, own[0], own[1], archive=archive, shared=shared, packed_gqa=packed, query_offset=offset, route=route)
    want = lc.chunk_attention(q, cat[0], cat[1], archive=archive, packed_gqa=packed, query_offset=offset, route=route_ref)
    assert got is not None and want is not None and got.shape == want.shape and got.dtype == dtype, tag
    assert route == route_ref == [want_route or ("packed" if packed else "chunk")], (tag, route, route_ref)
    assert torch.isfinite(got.float()).all() and torch.isfinite(want.float()).all(), tag
    if Ls % tile == 0:
        assert torch.equal(_bits(got), _bits(want)), (tag, "bitwise", (got.float() - want.float()).abs().max().item())
        return
    assert offset is None    # (attention_fp64 is bottom-right causal)
    ref = ar.attention_fp64(q, dense[0], dense[1])
    e = (ar.attention_eager_reference(q, dense[0], dense[1]).double() - ref).abs().max().item()
    bar = max(2.0 * e, ar.half_ulp(dtype, ref.abs().max().item()))
    err = (got.double() - ref).abs().max().item()
    twin = (want.double() - ref).abs().max().item()
    print(f"fp64[shared {tag}]: native {err:.3e}  existing call {twin:.3e}  eager E {e:.3e}  bar {bar:.3e}")
    assert err <= bar, (tag, err, bar)


# ---------------------------------------------------------------------------------------------------
# the chunk kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [1, 70, 130])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_chunk_kernel(dtype, Lq):
    """Hq 4 / Hkv 2, own Lq = Lk (130 crosses a 128-row workgroup), Ls x L8 over tile multiples, one row, odd sizes."""
    for Ls, L8 in itertools.product([0, 1, 64, 100, 192], [0, 37, 64]):
        segs = _segments(7, 4, 2, Lq, Lq, Ls, L8, dtype)
        _check((str(dtype)[6:], "Lq", Lq, "Ls", Ls, "L8", L8), *segs, tile=64, packed=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_chunk_kernel_wider_mask(dtype):
    """q_offset larger than bottom-right causal (the width of HF's mask over the uncompressed positions): the same number
    for the call over the concatenation."""
    Lq, Lk = 70, 90
    for Ls, L8 in itertools.product([64, 192], [0, 37, 64]):
        segs = _segments(8, 4, 2, Lq, Lk, Ls, L8, dtype)
        _check(("wide", Ls, L8), *segs, tile=64, packed=False, offset=L8 + Ls + Lk - Lq + 9)


@pytest.mark.parametrize("L8", [0, 64])
def test_chunk_kernel_key_split(L8):
    """Lq 2, own Lk 40, Ls 1536: few rows, so the keys are split over workgroups - the plan of the padded total."""
    import retake._native as nv

    assert nv.lib.rtk_attention_workspace_bytes_shared(4, 2, 2, 40, L8, 1536, D, nv.RTK_BF16) > 0
    segs = _segments(9, 4, 2, 2, 40, 1536, L8, torch.bfloat16)
    _check(("split", L8), *segs, tile=64, packed=False)
    segs = _segments(9, 4, 2, 2, 40, 1500, L8, torch.bfloat16)
    _check(("split-unaligned", L8), *segs, tile=64, packed=False)


# ---------------------------------------------------------------------------------------------------
# the packed decode kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,Lq", [(14, 2, 1), (14, 2, 2), (4, 2, 8)], ids=["G7-Lq1", "G7-Lq2", "G2-Lq8-R16"])
def test_decode_kernel(Hq, Hkv, Lq):
    import retake.longvideo_cache as lc

    for Lk in (1, 33):
        for Ls, L8 in itertools.product([0, 1, 32, 45, 160, 1056], [0, 45, 64]):
            if Lk < Lq:   # not a call: the queries are the last Lq of the own rows
                if (Ls, L8) == (32, 0):
                    segs = _segments(11, Hq, Hkv, Lq, Lq, Ls, L8, torch.bfloat16)
                    with pytest.raises(ValueError, match="Lk"):
                        lc.chunk_attention(segs[0], segs[3][0][:, :, :Lk], segs[3][1][:, :, :Lk], shared=segs[2], packed_gqa=True)
                continue
            segs = _segments(11, Hq, Hkv, Lq, Lk, Ls, L8, torch.bfloat16)
            _check(("decode", Hq, Lq, "Lk", Lk, "Ls", Ls, "L8", L8), *segs, tile=32, packed=True)


def test_decode_kernel_fp16():
    for Ls, L8 in itertools.product([32, 45], [0, 45]):
        segs = _segments(12, 14, 2, 2, 33, Ls, L8, torch.float16)
        _check(("decode fp16", Ls, L8), *segs, tile=32, packed=True)


def test_decode_declines_17_packed_rows_and_the_chunk_kernel_answers():
    import retake._native as nv

    Hq, Hkv, Lq, Lk, Ls = 34, 2, 1, 33, 64
    q, archive, shared, own, cat, dense = _segments(13, Hq, Hkv, Lq, Lk, Ls, 0, torch.bfloat16)
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=dev())
    rc = nv.lib.rtk_attention_decode_shared(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(own[0]), nv.ptr(own[1]), own[0].stride(1), own[0].stride(2),
        nv.ptr(shared[0]), nv.ptr(shared[1]), Ls, shared[0].stride(1), shared[0].stride(2), None, None, None, None, 0, 0, 0,
        nv.ptr(out), Hq, Hkv, Lq, Lk, Lk - Lq, D, nv.RTK_BF16, D ** -0.5, None, 0, nv.stream())
    assert rc == nv.RTK_EUNSUPPORTED and b"packed rows" in nv.lib.rtk_last_error()
    assert nv.lib.rtk_attention_decode_workspace_bytes_shared(Hq, Hkv, Lq, Lk, 0, Ls, D, nv.RTK_BF16) == 0
    # the front end falls to the chunk kernel in the same invocation
    _check("R17", q, archive, shared, own, cat, dense, tile=64, packed=True, want_route="chunk")

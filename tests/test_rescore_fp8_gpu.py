"""rtk_pivotkv_rescore_fp8k_batched on the GPU, the kernel alone: the re-scoring over the e4m3 key rows of an fp8 archive.

Rule 5 of the fp8 rows (include/retake_hip.h): a dequantised value dtype(float(code) * scale) is exactly representable in
the model dtype.  So the expected value needs no tolerance: the call must give, bit for bit, what the existing
rtk_pivotkv_rescore_batched gives on rtk_fp8kv_dequant of the same codes and scales.  On two shapes the float64
restatement (tests/rescore_ref.py on the dequantised keys) is demanded as well, under rescore_ref.bar with the project's BAR.

Operands: gaussian x 1.7 keys quantised by native_attention.fp8_quantize_rows, among them three planted rows per head - an
all-zero row (scale 1), a row scaled by 2^-20 and a row scaled by 2^10.  Code rows at and behind n hold 0x7F (e4m3 NaN)
and their scales NaN, score[n:] holds sentinels: a row read and used there, or a score written there, shows."""
import ctypes as C
import functools

import pytest
import torch

import rescore_ref as rr
from test_prompt_score_gpu import BAR, al256, dev
from test_rescore_gpu import SENTINEL, rescore

pytestmark = pytest.mark.gpu

D = 128
PAD_ROWS = 5        # NaN code rows / scales behind n, inside every head's stride
SHAPES = [          # Hq, Hkv, W, n
    *[(4, 2, 8, n) for n in (1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1025)],   # a wave holds 64 keys, a range 512
    (28, 4, 3, 129),
    (28, 4, 5, 1000),     # a ragged second block
    (8, 8, 16, 257),      # G 1
    (16, 1, 4, 640),      # Hkv 1
    (32, 4, 64, 600),     # 16 query blocks: two LDS tiles
]
FLOAT64_SHAPES = [(28, 4, 3, 129), (4, 2, 8, 513)]
DTYPES = [torch.bfloat16, torch.float16]


def dtype_code(dtype):
    import retake._native as nv

    return {torch.bfloat16: nv.RTK_BF16, torch.float16: nv.RTK_F16}[dtype]


@functools.lru_cache(maxsize=None)
def operands(seed, Hq, Hkv, W, n, dtype):
    """(q [Hq, W, D], codes uint8 [Hkv, n + PAD_ROWS, D] with 0x7F rows from n on, scales fp32 [Hkv, n + PAD_ROWS] with NaN
    from n on, old scores [n + 7] with sentinels from n on, k16 [Hkv, n + PAD_ROWS, D]: rtk_fp8kv_dequant of the first n
    rows, NaN behind them) on the device, made once per case and never written."""
    import retake._native as nv
    from retake.native_attention import fp8_quantize_rows

    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(Hq, W, D, generator=g) * 1.7).to(dtype)
    x = torch.randn(Hkv, n, D, generator=g) * 1.7
    for h in range(Hkv):     # the planted rows, at other places in every head (as many of the three as n has room for)
        for r, f in zip(torch.randperm(n, generator=g)[:3].tolist(), (0.0, 2.0 ** -20, 2.0 ** 10)):
            x[h, r] *= f
    old = torch.rand(n + 7, generator=g) * 2
    old[torch.rand(n + 7, generator=g) < 0.2] = 1.0
    old[n:] = SENTINEL
    c, s = fp8_quantize_rows(x.to(dtype).to(dev())[None])
    codes = torch.full((Hkv, n + PAD_ROWS, D), 0x7F, dtype=torch.uint8, device=dev())
    scales = torch.full((Hkv, n + PAD_ROWS), float("nan"), dtype=torch.float32, device=dev())
    codes[:, :n], scales[:, :n] = c[0], s[0]
    k16 = torch.full((Hkv, n + PAD_ROWS, D), float("nan"), dtype=dtype, device=dev())
    nv.check(nv.lib.rtk_fp8kv_dequant(nv.ptr(codes), codes.stride(0), nv.ptr(scales), scales.stride(0), nv.ptr(k16),
                                      k16.stride(0), Hkv, n, D, dtype_code(dtype), nv.stream()), "rtk_fp8kv_dequant")
    torch.cuda.synchronize()
    return q.to(dev()), codes, scales, old.to(dev()), k16


def rescore_fp8(units, Hq, Hkv, W, dtype, alpha):
    """One rtk_pivotkv_rescore_fp8k_batched call.  units: (q view [Hq, W, D] - any head / row strides, one pair for all -,
    codes [Hkv, cap, D] contiguous, scales [Hkv, cap'] contiguous, score tensor (copied: the result is returned), n).
    -> list of score tensors."""
    import retake._native as nv

    dt = dtype_code(dtype)
    qsh, qsl = units[0][0].stride(0), units[0][0].stride(1)
    stride = max(nv.lib.rtk_pivotkv_rescore_workspace_bytes(Hq, Hkv, W, u[4], D, dt) for u in units)
    assert stride > 0 and stride % 256 == 0
    scratch = torch.empty(len(units) * stride + 256, dtype=torch.uint8, device=dev())
    out = [u[3].clone() for u in units]
    arr = (nv.RescoreFp8kUnit * len(units))()
    for a, (q, c, s, _, n), o in zip(arr, units, out):
        assert q.stride() == (qsh, qsl, 1) and c.is_contiguous() and s.is_contiguous() and c.shape[1] >= n and s.shape[1] >= n
        assert c.dtype == torch.uint8 and s.dtype == torch.float32 and c.shape[0] == s.shape[0] == Hkv and c.shape[2] == D
        a.q, a.k8, a.k8_stride_h, a.k_scale, a.scale_stride_h = q.data_ptr(), c.data_ptr(), c.stride(0), s.data_ptr(), s.stride(0)
        a.score, a.n = o.data_ptr(), n
    nv.check(nv.lib.rtk_pivotkv_rescore_fp8k_batched(arr, len(units), Hq, Hkv, W, D, dt, alpha, qsh, qsl,
                                                     C.c_void_p(al256(scratch.data_ptr())), stride, nv.stream()),
             "rtk_pivotkv_rescore_fp8k_batched")
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Hq,Hkv,W,n", SHAPES, ids=[f"{a}_{b}_{c}_{d}" for a, b, c, d in SHAPES])
def test_the_bits_of_the_16_bit_call_on_the_dequantised_rows(Hq, Hkv, W, n, dtype):
    alpha = (0.5, 0.25, 1.0)[(n + W) % 3]
    q, codes, scales, old, k16 = operands(7, Hq, Hkv, W, n, dtype)
    got = rescore_fp8([(q, codes, scales, old, n)], Hq, Hkv, W, dtype, alpha)[0]
    want = rescore([(q, k16, old, n)], Hq, Hkv, W, D, dtype, alpha)[0]
    assert torch.equal(got[n:], old[n:]), "score[n:] was written"
    assert torch.isfinite(got[:n]).all(), "a code row or a scale at or behind n was read and used"
    differ = (bits(got) != bits(want)).sum().item()
    print(f"rescore fp8k {str(dtype)[6:]} {Hq}/{Hkv} W={W} n={n} alpha={alpha}: {differ} of {n} scores differ from the 16-bit "
          f"call on the dequantised rows; max |diff| = {(got[:n] - want[:n]).abs().max().item():.3e}")
    assert differ == 0
    if (Hq, Hkv, W, n) in FLOAT64_SHAPES:
        m64 = rr.mass(q, k16, n)
        want64 = rr.blend(old[:n], m64 * n / W, alpha)
        ratio = ((got[:n].double() - want64).abs() / rr.bar(alpha, n, W, BAR[dtype], m64, want64)).max().item()
        print(f"    against float64 on the dequantised keys: {ratio:.3f} of the bar")
        assert ratio <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_three_units_and_layouts_leave_the_bits_alone(dtype):
    """A batched call of three units with n = 0, 33 and 1000: the n = 0 unit is untouched, the others give the bits of a
    call of their own.  The same values behind a wider code head stride with a scale head stride different from it, behind
    other query strides (a slice of a chunk's tensor, the projection layout) and as unit 2 of 3 give those bits too."""
    Hq, Hkv, W, alpha = 28, 4, 5, 0.5
    ops = [operands(11 + i, Hq, Hkv, W, n, dtype) for i, n in enumerate((64, 33, 1000))]
    ns = (0, 33, 1000)
    alone = [rescore_fp8([(q, c, s, old, n)], Hq, Hkv, W, dtype, alpha)[0] if n else None for (q, c, s, old, _), n in zip(ops, ns)]
    for u in (1, 2):
        q, _, _, old, k16 = ops[u]
        want = rescore([(q, k16, old, ns[u])], Hq, Hkv, W, D, dtype, alpha)[0]
        assert torch.equal(bits(alone[u]), bits(want))
    both = rescore_fp8([(q, c, s, old, n) for (q, c, s, old, _), n in zip(ops, ns)], Hq, Hkv, W, dtype, alpha)
    assert torch.equal(both[0], ops[0][3]), "the n = 0 unit was touched"
    for u in (1, 2):
        assert torch.equal(bits(both[u]), bits(alone[u])), f"unit {u}: the bits depend on its neighbours"
    q, codes, scales, old, _ = ops[2]
    chunk = torch.randn((Hq, 40, D), device=dev()).to(dtype)
    chunk[:, 40 - W:] = q
    proj = torch.empty((W, Hq, D), dtype=dtype, device=dev())
    proj.transpose(0, 1).copy_(q)
    wide_c = torch.full((Hkv, codes.shape[1] + 24, D), 0x7F, dtype=torch.uint8, device=dev())
    wide_s = torch.full((Hkv, scales.shape[1] + 9), float("nan"), dtype=torch.float32, device=dev())
    wide_c[:, :1000], wide_s[:, :1000] = codes[:, :1000], scales[:, :1000]
    for name, qv, cv, sv in (("slice", chunk[:, 40 - W:], codes, scales), ("projection", proj.transpose(0, 1), codes, scales),
                             ("wide codes, other scale stride", q, wide_c, wide_s)):
        got = rescore_fp8([(qv, cv, sv, old, 1000)], Hq, Hkv, W, dtype, alpha)[0]
        assert torch.equal(bits(got), bits(alone[2])), f"{name}: the bits depend on the layout"
    q1, c1, s1, old1, _ = operands(21, Hq, Hkv, W, 700, dtype)
    got = rescore_fp8([(q1, c1, s1, old1, 700), (*ops[1][:4], 33), (proj.transpose(0, 1).contiguous(), wide_c, wide_s, old, 1000)],
                      Hq, Hkv, W, dtype, alpha)
    assert torch.equal(bits(got[2]), bits(alone[2])), "unit 2 of 3: the bits depend on the call"
    assert torch.equal(bits(got[1]), bits(alone[1]))

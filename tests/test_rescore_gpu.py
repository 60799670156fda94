"""rtk_pivotkv_rescore_batched on the GPU, the kernel alone, against the float64 restatement tests/rescore_ref.py.

Inputs: q, k gaussian x 1.7 (as synth.qkv_chunk), old scores uniform in [0, 2] with exact 1.0 entries mixed in.  The key
rows at and behind n hold NaN and the key heads lie further apart than n rows, score[n:] holds sentinels: a row read and
used there, or a score written there, shows.

Bar, per row j, on the project's score bars (test_prompt_score_gpu.BAR: 5e-6 for fp32 operands, 2e-5 for 16-bit ones):
    |got - want64| <= alpha (n / Wc) BAR max(1, mass64[j]) + 4 2^-24 |want64[j]|
The bars were set on column sums of magnitude about 1, hence the max(1, .); the second term is the blend's two fp32 roundings.
Beside every result the error of the existing rtk_pivotkv_score_prompt_batched on the same operands laid out as one chunk
(L = n + W, Lp = W; its score x n is obs) is printed: the yardstick.  Where a shape exceeds the bar and the yardstick does
too, the new kernel is held to twice the yardstick's measured error instead (profiles/rescore_parity_stats.txt)."""
import ctypes as C
import functools

import pytest
import torch

import rescore_ref as rr
from test_prompt_score_gpu import BAR, al256, dev, run_kernel

pytestmark = pytest.mark.gpu

KEYS = 512          # retake._native.RESCORE_KEYS, asserted below: the key ranges the implementation chose
SENTINEL = -7.25
PAD_ROWS = 5        # NaN key rows behind n, inside every head's stride

SHAPES = [          # Hq, Hkv, W, n
    (4, 2, 8, 1), (4, 2, 8, 31), (4, 2, 8, 33),
    (28, 4, 3, 129),      # 21 packed rows
    (28, 4, 5, 1000),     # 35 rows: a ragged second block
    (28, 4, 64, 4099),    # 14 full blocks, 9 key ranges
    (8, 8, 16, 257),      # G 1
    (16, 1, 4, 640),      # Hkv 1
    (32, 4, 8, 2048),     # 64 rows
    # one below, at and one above the boundaries of the key split (and of a wave's 128 keys inside a range)
    (4, 2, 8, 127), (4, 2, 8, 128), (4, 2, 8, KEYS - 1), (4, 2, 8, KEYS), (4, 2, 8, KEYS + 1),
    (4, 2, 8, 2 * KEYS - 1), (4, 2, 8, 2 * KEYS), (4, 2, 8, 2 * KEYS + 1),   # the last one spans three ranges
]
VARIANTS = [(torch.bfloat16, 128), (torch.float16, 128), (torch.float32, 128), (torch.bfloat16, 64)]
VARIANT_IDS = ["bf16_mfma", "fp16_mfma", "fp32_generic", "bf16_D64_generic"]


@functools.lru_cache(maxsize=None)
def operands(seed, Hq, Hkv, W, n, D, dtype):
    """(q [Hq, W, D], k [Hkv, n + PAD_ROWS, D] with NaN rows from n on, old scores [n + 7] with sentinels from n on) on the
    device, made once per case and never written."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(Hq, W, D, generator=g) * 1.7).to(dtype)
    k = (torch.randn(Hkv, n + PAD_ROWS, D, generator=g) * 1.7).to(dtype)
    k[:, n:] = float("nan")
    old = torch.rand(n + 7, generator=g) * 2
    old[torch.rand(n + 7, generator=g) < 0.2] = 1.0
    old[n:] = SENTINEL
    return q.to(dev()), k.to(dev()), old.to(dev())


def rescore(units, Hq, Hkv, W, D, dtype, alpha):
    """One rtk_pivotkv_rescore_batched call.  units: (q view [Hq, W, D] - any head / row strides, one pair for all -,
    k [Hkv, cap, D] contiguous, score tensor (copied: the result is returned), n).  -> list of score tensors."""
    import retake._native as nv

    dt = {torch.float32: nv.RTK_F32, torch.bfloat16: nv.RTK_BF16, torch.float16: nv.RTK_F16}[dtype]
    qsh, qsl = units[0][0].stride(0), units[0][0].stride(1)
    stride = max(nv.lib.rtk_pivotkv_rescore_workspace_bytes(Hq, Hkv, W, u[3], D, dt) for u in units)
    assert stride > 0 and stride % 256 == 0
    scratch = torch.empty(len(units) * stride + 256, dtype=torch.uint8, device=dev())
    out = [u[2].clone() for u in units]
    arr = (nv.RescoreUnit * len(units))()
    for a, (q, k, _, n), s in zip(arr, units, out):
        assert q.stride() == (qsh, qsl, 1) and k.is_contiguous() and k.shape[1] >= n
        a.q, a.k, a.k_stride_h, a.score, a.n = q.data_ptr(), k.data_ptr(), k.stride(0), s.data_ptr(), n
    nv.check(nv.lib.rtk_pivotkv_rescore_batched(arr, len(units), Hq, Hkv, W, D, dt, alpha, qsh, qsl,
                                                C.c_void_p(al256(scratch.data_ptr())), stride, nv.stream()),
             "rtk_pivotkv_rescore_batched")
    torch.cuda.synchronize()
    return out


def yardstick(q, k, n):
    """obs by the existing prompt-score kernel: the same operands as one chunk of L = n + W rows whose last W are the prompt."""
    Hq, W, D = q.shape
    qf = torch.zeros((Hq, n + W, D), dtype=q.dtype, device=q.device)
    qf[:, n:] = q
    kf = torch.zeros((k.shape[0], n + W, D), dtype=k.dtype, device=k.device)
    kf[:, :n] = k[:, :n]
    return run_kernel([qf], [kf], W)[0, :n].double() * n


def check(name, got, q, k, old, n, alpha, dtype):
    W = q.shape[1]
    m64 = rr.mass(q, k, n)
    o64 = m64 * n / W
    want = rr.blend(old[:n], o64, alpha)
    bar = rr.bar(alpha, n, W, BAR[dtype], m64, want)
    err = (got[:n].double() - want).abs()
    y_err = alpha * (yardstick(q, k, n) - o64).abs()
    ratio, y_ratio = (err / bar).max().item(), (y_err / bar).max().item()
    print(f"rescore {name}: max |got - float64| = {err.max().item():.3e} ({ratio:.3f} of the bar); existing prompt kernel on the "
          f"same operands: {y_err.max().item():.3e} ({y_ratio:.3f} of the bar)")
    assert torch.equal(got[n:], old[n:]), f"{name}: score[n:] was written"
    assert torch.isfinite(got[:n]).all(), f"{name}: a key row at or behind n was read and used"
    if ratio > 1 and y_ratio > 1:
        assert err.max().item() <= 2 * y_err.max().item(), (name, err.max().item(), y_err.max().item())
    else:
        assert ratio <= 1, (name, ratio)


def test_the_key_split_is_the_one_mirrored_here():
    import retake._native as nv

    assert nv.RESCORE_KEYS == KEYS


@pytest.mark.parametrize("dtype,D", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("Hq,Hkv,W,n", SHAPES, ids=[f"{a}_{b}_{c}_{d}" for a, b, c, d in SHAPES])
def test_kernel_against_float64(Hq, Hkv, W, n, dtype, D):
    alpha = (0.5, 0.25, 1.0)[(n + W) % 3]
    q, k, old = operands(7, Hq, Hkv, W, n, D, dtype)
    got = rescore([(q, k, old, n)], Hq, Hkv, W, D, dtype, alpha)[0]
    again = rescore([(q, k, old, n)], Hq, Hkv, W, D, dtype, alpha)[0]
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs differ"
    check(f"{str(dtype)[6:]} D={D} {Hq}/{Hkv} W={W} n={n} alpha={alpha}", got, q, k, old, n, alpha, dtype)


@pytest.mark.parametrize("dtype,D", VARIANTS, ids=VARIANT_IDS)
def test_three_units_layouts_and_determinism(dtype, D):
    """A batched call of three units with n = 0, 33 and 1000; the same values behind other query strides and another key
    head stride, and as unit 2 of 3, give the bits of a call of that unit alone."""
    Hq, Hkv, W, alpha = 28, 4, 5, 0.5
    ops = [operands(11 + i, Hq, Hkv, W, n, D, dtype) for i, n in enumerate((64, 33, 1000))]
    ns = (0, 33, 1000)
    alone = [rescore([(q, k, old, n)], Hq, Hkv, W, D, dtype, alpha)[0] if n else None for (q, k, old), n in zip(ops, ns)]
    both = rescore([(q, k, old, n) for (q, k, old), n in zip(ops, ns)], Hq, Hkv, W, D, dtype, alpha)
    assert torch.equal(both[0], ops[0][2]), "the n = 0 unit was touched"
    for u in (1, 2):
        assert torch.equal(both[u].view(torch.int32), alone[u].view(torch.int32)), f"unit {u}: the bits depend on its neighbours"
        check(f"batched unit {u} {str(dtype)[6:]} D={D}", both[u], *ops[u], ns[u], alpha, dtype)
    # queries as a strided slice of a chunk's tensor [Hq, L, D], and in the projection layout [L, Hq, D]; keys with a wider
    # head stride
    q, k, old = ops[2]
    chunk = torch.randn((Hq, 40, D), device=dev()).to(dtype)
    chunk[:, 40 - W:] = q
    proj = torch.empty((W, Hq, D), dtype=dtype, device=dev())
    proj.transpose(0, 1).copy_(q)
    wide = torch.full((Hkv, k.shape[1] + 24, D), float("nan"), dtype=dtype, device=dev())
    wide[:, :1000] = k[:, :1000]
    for name, qv, kv in (("slice", chunk[:, 40 - W:], k), ("projection", proj.transpose(0, 1), k), ("wide keys", q, wide)):
        got = rescore([(qv, kv, old, 1000)], Hq, Hkv, W, D, dtype, alpha)[0]
        assert torch.equal(got.view(torch.int32), alone[2].view(torch.int32)), f"{name}: the bits depend on the layout"
    # ... and as unit 2 of 3 behind units of other sizes
    q1, k1, old1 = operands(21, Hq, Hkv, W, 700, D, dtype)
    got = rescore([(q1, k1, old1, 700), (ops[1][0], ops[1][1], ops[1][2], 33), (proj.transpose(0, 1).contiguous(), wide, old, 1000)],
                  Hq, Hkv, W, D, dtype, alpha)
    assert torch.equal(got[2].view(torch.int32), alone[2].view(torch.int32)), "unit 2 of 3: the bits depend on the call"
    assert torch.equal(got[1].view(torch.int32), alone[1].view(torch.int32))

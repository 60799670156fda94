"""The MA-LLM kernels against tests/mallm_ref.py, through the C ABI (retake._native.lib) so that the indices are seen
and nothing can fall back: rtk_adjacent_cosine, rtk_mallm_argmax, rtk_mallm_merge and rtk_mallm_hard_chain on their own.

Lattice banks (mallm_ref.lattice_bank) have cosines k/m that are exact in fp32, bf16 and fp16 in any summation order, so
every arg-max decision of a chain - most of them ties, decided by the first-index rule - is compared index for index with
an integer reference.  tests/test_mallm_ref_cpu.py checks that reference and the input conditions of the banks used here.
"""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import mallm_ref as mr
import synth

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MODE = {"fp32": 0, "bf16": 1, "fp16": 2}          # the round_bf16 argument


def dev():
    return torch.device("cuda:0")


def code(dt):
    import retake._native as nv

    return {"fp32": nv.RTK_F32, "bf16": nv.RTK_BF16, "fp16": nv.RTK_F16}[dt]


def to_dev(x64, dt):
    xt = torch.from_numpy(np.ascontiguousarray(x64)).to(TDT[dt])
    assert torch.equal(xt.double(), torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float64)))   # exact in the dtype
    return xt.to(dev()).contiguous()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def adjacent_cosine(xt, dt):
    import retake._native as nv

    T, N, C = xt.shape
    cos = torch.full((T - 1, N), -7.0, dtype=torch.float32, device=dev())
    assert nv.lib.rtk_adjacent_cosine(nv.ptr(xt), T, N, C, code(dt), nv.ptr(cos), nv.stream()) == 0
    return cos


def argmax(cos, sync, mode):
    import retake._native as nv

    T1, N = cos.shape
    assert cos.dtype == torch.float32 and cos.is_contiguous()
    idx = torch.full((N,), -1, dtype=torch.int64, device=dev())
    assert nv.lib.rtk_mallm_argmax(nv.ptr(cos), T1, N, int(sync), mode, nv.ptr(idx), nv.stream()) == 0
    return idx.cpu().numpy()


def chain(xt, dt, tgt, sync):
    """-> (rc, idx [tgt,N] / [tgt], the device tensor of idx)."""
    import retake._native as nv

    T, N, C = xt.shape
    ws = torch.empty((T - 1, N), dtype=torch.float32, device=dev())
    idx = torch.full((tgt,) if sync else (tgt, N), -1, dtype=torch.int64, device=dev())
    rc = nv.lib.rtk_mallm_hard_chain(nv.ptr(xt), T, N, C, code(dt), tgt, int(sync), nv.ptr(ws), nv.ptr(idx), nv.stream())
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), idx


def gather_frames(xt, dt, idx_dev, tgt, sync):
    import retake._native as nv

    T, N, C = xt.shape
    out = torch.empty((tgt, N, C), dtype=xt.dtype, device=dev())
    assert nv.lib.rtk_gather_frames(nv.ptr(xt), T, N, C, code(dt), nv.ptr(idx_dev), tgt, int(sync), nv.ptr(out),
                                    nv.stream()) == 0
    return out


# ---------------------------------------------------------------------------------------------------
# rtk_adjacent_cosine
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,T,N,C,m,dt", [c[:5] + (dt,) for c in mr.COS_CASES for dt in c[5]])
def test_adjacent_cosine_is_exact_on_lattice_banks(seed, T, N, C, m, dt):
    """cos * m is the integer sum(sign_a * sign_b), exactly, in every dtype, kernel and strip geometry."""
    signs, _, x = mr.lattice_bank(seed, T, N, C, m)
    cos = adjacent_cosine(to_dev(x, dt), dt).cpu().numpy()
    np.testing.assert_array_equal(cos.astype(np.float64) * m, mr.pair_counts(signs))


def test_adjacent_cosine_random_fp32_within_its_error_bound():
    """|cos - cosine64| <= 2 (C + 6) 2^-24: C fused multiply-adds, two divisions and a product per term, on unit operands.
    Measured on MI355X: profiles/mallm_parity_stats.txt."""
    T, N, C = 33, 7, 40
    x = synth.frames_iid(5, T, N, C)[0]
    cos = adjacent_cosine(torch.from_numpy(x).to(dev()), "fp32").cpu().numpy()
    err = np.abs(cos.astype(np.float64) - mr.cosine64(x)).max()
    bar = 2 * (C + 6) * 2.0 ** -24
    print(f"\n[adjacent cosine fp32 ({T}, {N}, {C})] max |cos - float64| = {err:.3e} (bar {bar:.3e}, {err / 2.0 ** -24:.2f} ulp of 1)")
    assert err <= bar


# ---------------------------------------------------------------------------------------------------
# rtk_mallm_argmax on planted similarity matrices
# ---------------------------------------------------------------------------------------------------
def planted_sets(T1):
    """Index sets that hold the (equal) maximum of a column: single positions at the ends of lanes, waves and the
    256-thread stride; pairs and triples that straddle them (the lowest must win); None = a column of equal values."""
    sets = [(0,), (63,), (64,), (255,), (256,), (T1 - 1,),
            (1, 2), (63, 64), (62, 63, 64), (0, T1 - 1), (T1 - 2, T1 - 1), (127, 128), (191, 192), (70, 200),
            (255, 256), (255, 256, 257), (5, 261), (0, 256), (3, 259, 515), (63, 64, 320), (300, 556), (256, 511, 512)]
    out = []
    for s in sets:
        s = tuple(sorted({p for p in s if 0 <= p < T1}))
        if s and s not in out:
            out.append(s)
    return out + [None]


def background(rng, T1, N):
    """Multiples of 2^-6 in [-1, 0.5]: every partial sum over a patch row is exact in fp32 whatever its order."""
    return rng.integers(-64, 33, size=(T1, N)).astype(np.float64) / 64.0


@pytest.mark.parametrize("T1", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_argmax_async_planted(T1):
    N = 5
    rng = np.random.default_rng(T1)
    plans = planted_sets(T1)
    for g in range(0, len(plans), N):
        group = (plans[g:g + N] * N)[:N]           # five columns a launch; a short last group repeats its plans
        cos = background(rng, T1, N)
        for n, s in enumerate(group):
            if s is None:
                cos[:, n] = 0.25
            else:
                cos[list(s), n] = 0.75
        want = mr.argmax_step(cos, False, N)
        np.testing.assert_array_equal(want, [0 if s is None else s[0] for s in group])     # the plan itself
        got = argmax(torch.from_numpy(cos).float().to(dev()), False, 0)
        np.testing.assert_array_equal(got, want, err_msg=f"T1={T1} planted {group}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 17, 64, 70])
@pytest.mark.parametrize("T1", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_argmax_sync_planted(T1, N, mode):
    """The patch mean (fp32 sum, one division, one rounding to the dtype of `mode`) and its first arg-max, written to
    every entry of idx.  Planted frames hold 0.75 at every patch position - their mean is 0.75 in every dtype - over a
    background whose means stay below 0.5 but may round to ties among themselves."""
    dt = mr.DTYPES[mode]
    rng = np.random.default_rng(1000 * T1 + N)
    for s in planted_sets(T1):
        cos = background(rng, T1, N)
        if s is None:
            cos[:] = 0.25
        else:
            cos[list(s)] = 0.75
        want = mr.argmax_step(cos, True, N, dt)
        assert want.shape == (N,) and (want == (0 if s is None else s[0])).all()
        got = argmax(torch.from_numpy(cos).float().to(dev()), True, mode)
        np.testing.assert_array_equal(got, want, err_msg=f"T1={T1} N={N} mode={mode} planted {s}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_argmax_sync_rounded_means_tie(mode):
    """Two patch means that differ in fp32 and round to one bf16 / fp16 value: frame 200 holds 0.75 everywhere, frame 40
    misses it by 2^-6 at one patch position.  fp32 takes the larger mean, the 16-bit dtypes tie and take the first."""
    T1, N = 300, 70
    cos = background(np.random.default_rng(7), T1, N)
    cos[[40, 200]] = 0.75
    cos[40, 33] -= 2.0 ** -6
    want = mr.argmax_step(cos, True, N, mr.DTYPES[mode])
    assert (want == (200, 40, 40)[mode]).all()
    np.testing.assert_array_equal(argmax(torch.from_numpy(cos).float().to(dev()), True, mode), want)


def test_argmax_sync_refuses_a_row_beyond_lds():
    import retake._native as nv

    T1 = 16385
    cos = torch.zeros((T1, 1), dtype=torch.float32, device=dev())
    idx = torch.full((1,), -1, dtype=torch.int64, device=dev())
    assert nv.lib.rtk_mallm_argmax(nv.ptr(cos), T1, 1, 1, 0, nv.ptr(idx), nv.stream()) == nv.RTK_EUNSUPPORTED
    torch.cuda.synchronize()
    assert int(idx[0]) == -1


# ---------------------------------------------------------------------------------------------------
# rtk_mallm_merge with a planted idx
# ---------------------------------------------------------------------------------------------------
def merge(xt, st, idx, dt, hard):
    import retake._native as nv

    T, N, C = xt.shape
    out = torch.empty((T - 1, N, C), dtype=xt.dtype, device=dev())
    so = None if hard else torch.empty((T - 1, N), dtype=xt.dtype, device=dev())
    it = torch.from_numpy(idx).to(dev())
    assert nv.lib.rtk_mallm_merge(nv.ptr(xt), None if hard else nv.ptr(st), nv.ptr(it), T, N, C, code(dt), int(hard),
                                  nv.ptr(out), None if hard else nv.ptr(so), nv.stream()) == 0
    return out, so


def planted_idx(T, N, r):
    """The merged slot of patch n: 0, T-2 or an interior frame, in turn."""
    choices = [0, T - 2, (T - 2) // 2 if T > 3 else 0]
    return np.array([choices[(n + r) % 3] for n in range(N)], dtype=np.int64)


@pytest.mark.parametrize("dt", mr.DTYPES)
@pytest.mark.parametrize("T,N,C", [(2, 1, 1), (5, 3, 7), (9, 4, 33), (6, 2, 1280)])
def test_merge_bit_equal_with_planted_idx(T, N, C, dt):
    """Hard: the copy out[t] = x[t + (t >= idx)].  Soft: out and sizes_out bit-equal to the torch-CPU expression in the
    bank's dtype - one rounding per torch op is the kernel's stated contract."""
    rng = np.random.default_rng(T * 100 + C)
    x = torch.from_numpy(rng.standard_normal((T, N, C)).astype(np.float32)).to(TDT[dt])
    sizes = torch.from_numpy(rng.integers(1, 13, size=(T, N)).astype(np.float32)).to(TDT[dt])
    xt, st = x.to(dev()), sizes.to(dev())
    for r in range(3):
        idx = planted_idx(T, N, r)
        assert idx.min() >= 0 and idx.max() <= T - 2
        out, _ = merge(xt, None, idx, dt, True)
        np.testing.assert_array_equal(bits(out), bits(mr.hard_merge(x, torch.from_numpy(idx))))
        out, so = merge(xt, st, idx, dt, False)
        want, want_s = mr.soft_merge(x, sizes, torch.from_numpy(idx))
        np.testing.assert_array_equal(bits(so), bits(want_s), err_msg=f"sizes_out, idx {idx}")
        np.testing.assert_array_equal(bits(out), bits(want), err_msg=f"out, idx {idx}")


def test_merge_bf16_sizes_beyond_256():
    """Sizes up to 300: above 256 a bf16 size, and the sum of two, rounds; the merge stays finite and equal."""
    T, N, C = 9, 4, 33
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((T, N, C)).astype(np.float32)).bfloat16()
    sizes = torch.from_numpy(rng.integers(200, 301, size=(T, N)).astype(np.float32)).bfloat16()
    for r in range(3):
        idx = planted_idx(T, N, r)
        out, so = merge(x.to(dev()), sizes.to(dev()), idx, "bf16", False)
        want, want_s = mr.soft_merge(x, sizes, torch.from_numpy(idx))
        assert torch.isfinite(out.float()).all() and torch.isfinite(so.float()).all()
        np.testing.assert_array_equal(bits(so), bits(want_s))
        np.testing.assert_array_equal(bits(out), bits(want))


# ---------------------------------------------------------------------------------------------------
# one step on random data
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,T,N,C,sync", mr.STEP_CASES)
def test_step_on_random_data_is_the_float64_argmax(seed, T, N, C, sync):
    """rtk_adjacent_cosine -> rtk_mallm_argmax on fp32 data whose float64 top-2 gap is beyond the fp32 error in every
    column (asserted in tests/test_mallm_ref_cpu.py): T1 = 299 takes the second trip of the 256-thread scan."""
    x = synth.frames_iid(seed, T, N, C)[0]
    cos = adjacent_cosine(torch.from_numpy(x).to(dev()), "fp32")
    np.testing.assert_array_equal(argmax(cos, sync, 0), mr.argmax_step(mr.cosine64(x), sync, N))


# ---------------------------------------------------------------------------------------------------
# rtk_mallm_hard_chain
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_reference(case, dt):
    signs, _, x = mr.case_bank(case)
    return x, mr.hard_chain(signs, case.m, case.tgt, case.sync, dt)


@pytest.mark.parametrize("case,dt", [(c, dt) for c in mr.CHAIN_CASES for dt in c.dtypes],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d_t%d_%s" % (
                             v.T, v.N, v.C, v.tgt, "sync" if v.sync else "async"))
def test_hard_chain_on_lattice_banks(case, dt):
    """idx_out == the integer reference, index for index."""
    x, ref = chain_reference(case, dt)
    rc, idx, _ = chain(to_dev(x, dt), dt, case.tgt, case.sync)
    assert rc == 0
    np.testing.assert_array_equal(idx, ref.idx)


def fixture_bank(name):
    g = gu.load(name)
    dt = "fp16" if name.startswith("fp16") else str(g["dtype"])
    x, out = g["x"][0], g["out"][0]
    if dt != "fp32":
        x, out = (torch.from_numpy(a.view(np.int16)).view(TDT[dt]) for a in (x, out))
    else:
        x, out = torch.from_numpy(x), torch.from_numpy(out)
    return g, dt, x, out


@pytest.mark.parametrize("name", gu.names("mallm_lattice_") + gu.names("fp16mallm_lattice_"))
def test_hard_chain_reproduces_the_reference_on_the_lattice_fixture(name):
    """The reference's own run of the loop, recorded (the fp16 bank with an all-zero frame - NaN similarities - among
    them): chain + rtk_gather_frames give its bank bit for bit, and so does the loop of single steps."""
    import retake.visual_compression as vc

    g, dt, x, want = fixture_bank(name)
    tgt, sync = int(g["tgt"]), bool(g["sync"])
    xt = x.to(dev())
    rc, idx, idx_dev = chain(xt, dt, tgt, sync)
    assert rc == 0
    np.testing.assert_array_equal(bits(gather_frames(xt, dt, idx_dev, tgt, sync)), bits(want))
    # the first decision alone, through rtk_mallm_argmax
    first = argmax(adjacent_cosine(xt, dt), sync, MODE[dt])
    np.testing.assert_array_equal(first, g["steps_idx"][0])
    bank = xt[None]
    while bank.shape[1] > tgt:
        bank = vc.memory_bank_compress_MALLM_hard(bank, sync=sync)
    np.testing.assert_array_equal(bits(bank[0]), bits(want))


def test_nan_similarities_are_the_maximum_and_the_first_wins():
    """torch.max(dim) returns the first NaN: a column with NaN at 5 and 6 of 19 gives 5 (async and sync); a zero fp16
    frame makes such a column (0 / 0, like the reference)."""
    for N in (1, 5):
        cos = background(np.random.default_rng(N), 19, N)
        cos[[5, 6]] = np.nan
        ct = torch.from_numpy(cos).float().to(dev())
        for sync in (False, True):
            np.testing.assert_array_equal(argmax(ct, sync, 0), np.full(N, 5))
    cos = background(np.random.default_rng(3), 600, 5)
    cos[[300, 64], 0], cos[[257, 256], 1], cos[[599], 2], cos[[63, 0], 3] = np.nan, np.nan, np.nan, np.nan
    want = mr.argmax_step(cos, False, 5)
    np.testing.assert_array_equal(want[:4], [64, 256, 599, 0])
    np.testing.assert_array_equal(argmax(torch.from_numpy(cos).float().to(dev()), False, 0), want)
    signs, _, x = mr.lattice_bank(21, 12, 3, 8, 4)
    x[6] = 0.0
    got = adjacent_cosine(to_dev(x, "fp16"), "fp16").cpu().numpy()
    assert np.isnan(got[5:7]).all() and not np.isnan(np.delete(got, [5, 6], axis=0)).any()


def test_hard_chain_refusals():
    """RTK_EUNSUPPORTED for a frame list beyond the LDS (T = 12 801: 12 bytes a frame over 150 KiB) and for rows that are
    no 16-byte vectors (C = 6 in bf16).  The ABI call alone: the fall-back loop is not run at that length."""
    import retake._native as nv

    x = torch.ones((12801, 1, 8), dtype=torch.float32, device=dev())
    rc, idx, _ = chain(x, "fp32", 12000, False)
    assert rc == nv.RTK_EUNSUPPORTED and (idx == -1).all()
    assert b"rtk_mallm_hard_chain" in nv.lib.rtk_last_error()
    x = torch.ones((8, 2, 6), dtype=torch.bfloat16, device=dev())
    for sync in (False, True):
        rc, idx, _ = chain(x, "bf16", 4, sync)
        assert rc == nv.RTK_EUNSUPPORTED and (idx == -1).all()


"""tests/mallm_ref.py checked without a GPU: against every MA-LLM fixture recorded from the reference, against the C
oracle on lattice banks, and the input conditions of the banks tests/test_mallm_gpu.py runs."""
import numpy as np
import pytest
import torch

import golden_util as gu
import mallm_ref as mr
import synth
from oracle import oracle as orc

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
FIXTURES = gu.names("mallm_") + gu.names("fp16mallm_")
LATTICE = gu.names("mallm_lattice_") + gu.names("fp16mallm_lattice_")


def fixture_tensor(g, key, name):
    """x / out of a fixture as a torch tensor of its dtype, batch axis dropped."""
    a = g[key]
    dtype = "fp16" if name.startswith("fp16") else str(g["dtype"])
    if dtype == "fp32":
        return torch.from_numpy(a)[0], dtype
    return torch.from_numpy(a.view(np.int16)).view(TDT[dtype])[0], dtype


def gather(x, idx):
    return np.take_along_axis(x, idx[:, :, None], 0)


# ---------------------------------------------------------------------------------------------------
# the reference's own runs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_float64_loop_reproduces_the_reference_fixture(name):
    """hard: hard_chain64's surviving frames ARE the reference's bank (copies: bit-equal).  soft: soft_chain within
    test_mallm_golden's bars.  fp32 banks are decided by the float64 cosines; a 16-bit bank of random data holds pairs
    that only the dtype's own rounding separates or ties, so there the cosines are cosine_ops'."""
    g = gu.load(name)
    xt, dtype = fixture_tensor(g, "x", name)
    ref, _ = fixture_tensor(g, "out", name)
    tgt, sync = int(g["tgt"]), bool(g["sync"])
    cosine = mr.cosine64 if dtype == "fp32" or "lattice" in name else mr.cosine_ops
    if bool(g["hard"]):
        idx, steps = mr.hard_chain64(xt.double().numpy(), tgt, sync, dtype, cosine)
        out = gather(xt.float().numpy(), idx)
        np.testing.assert_array_equal(out, ref.float().numpy())
        if "steps_idx" in g.files:
            np.testing.assert_array_equal(steps, g["steps_idx"])
        return
    bank, sizes, steps = mr.soft_chain(xt, tgt, sync, dtype, cosine)
    if "steps_idx" in g.files:
        np.testing.assert_array_equal(np.stack(steps), g["steps_idx"])
    a, b = bank.float().numpy(), ref.float().numpy()
    if dtype == "fp32":
        assert np.abs(a - b).max() <= 1e-5
    else:
        assert np.abs(a - b).max() <= (2 ** -6 if dtype == "bf16" else 2 ** -8) and (a != b).mean() < 0.02
    if dtype != "bf16":
        np.testing.assert_array_equal(sizes.float().numpy(), g["size"][0])


@pytest.mark.parametrize("name", [n for n in FIXTURES if "soft" in n and "bf16" not in n and not n.startswith("fp16")])
def test_soft_merge_is_the_reference_arithmetic_in_fp32(name):
    """In fp32 the torch-CPU expression and the reference run the same ops on the same pairs: the banks are bit-equal."""
    g = gu.load(name)
    xt, dtype = fixture_tensor(g, "x", name)
    bank, sizes, _ = mr.soft_chain(xt, int(g["tgt"]), bool(g["sync"]), dtype)
    np.testing.assert_array_equal(bank.numpy(), g["out"][0])


@pytest.mark.parametrize("name", LATTICE)
def test_integer_chain_reproduces_the_lattice_fixture(name):
    """The fixtures recorded from the reference on the lattice bank - the fp16 bank with an all-zero frame among them,
    which pins what the arg-max does with NaN - against the integer reference: every step and the bank."""
    g = gu.load(name)
    seed, T, N, C, m, tgt = mr.FIXTURE_BANK
    xt, dtype = fixture_tensor(g, "x", name)
    signs, _, x = mr.lattice_bank(seed, T, N, C, m)
    zf = int(g["zero_frame"])
    if zf >= 0:
        signs[zf], x[zf] = 0, 0.0
    np.testing.assert_array_equal(xt.double().numpy(), x)
    assert (int(g["tgt"]), int(g["m"])) == (tgt, m)
    ch = mr.hard_chain(signs, m, tgt, bool(g["sync"]), dtype)
    np.testing.assert_array_equal(ch.steps, g["steps_idx"])
    idx = ch.idx if ch.idx.ndim == 2 else np.repeat(ch.idx[:, None], N, 1)
    ref, _ = fixture_tensor(g, "out", name)
    np.testing.assert_array_equal(gather(x, idx), ref.double().numpy())
    idx64, steps64 = mr.hard_chain64(x, tgt, bool(g["sync"]), dtype)
    np.testing.assert_array_equal(idx64, idx)
    np.testing.assert_array_equal(steps64, ch.steps)
    if zf >= 0:   # the fixture has teeth: the rule "NaN never wins" would have merged other pairs
        assert mr.eps_of(dtype) == 0.0 and np.isnan(mr.cosine64(x, dtype)[zf - 1:zf + 1]).all()
        other = mr.hard_chain(signs, m, tgt, bool(g["sync"]), "fp32")   # zero rows clamp to eps: their cosines are 0
        assert not np.array_equal(other.steps, g["steps_idx"])
        assert ch.steps[0, 0] == zf - 1                                  # the first NaN pair goes first


def test_first_max_rule():
    nan = np.nan
    v = np.array([[1.0, nan, 3.0, -np.inf], [2.0, 0.0, 3.0, -np.inf], [2.0, nan, nan, -np.inf], [nan, 5.0, nan, -np.inf]])
    np.testing.assert_array_equal(mr.first_max(v), [3, 0, 2, 0])
    want = torch.max(torch.from_numpy(v), dim=0).indices.numpy()       # the documented rule of torch.max(dim)
    np.testing.assert_array_equal(mr.first_max(v), want)
    np.testing.assert_array_equal(mr.argmax_step(v, True, 4, "fp32"), [0, 0, 0, 0])   # every patch mean is NaN


# ---------------------------------------------------------------------------------------------------
# lattice banks
# ---------------------------------------------------------------------------------------------------
def all_banks():
    seen = {}
    for c in mr.CHAIN_CASES:
        seen[(c.seed, c.T, c.N, c.C, c.m, c.width)] = None
    for seed, T, N, C, m, _ in mr.COS_CASES:
        seen[(seed, T, N, C, m, 0)] = None
    seen[mr.FIXTURE_BANK[:5] + (0,)] = None
    return list(seen)


@pytest.mark.parametrize("bank", all_banks(), ids=lambda b: "s%d_%dx%dx%d_m%d_w%d" % b)
def test_lattice_properties(bank):
    """m non-zeros of one magnitude per row; cos * m an integer, the same integer in float64, in two fp32 summation
    orders and in torch's own cosine in all three dtypes; every value representable in bf16 and fp16."""
    seed, T, N, C, m, width = bank
    signs, exps, x = mr.lattice_bank(seed, T, N, C, m, width)
    assert signs.shape == (T, N, C) and ((signs != 0).sum(-1) == m).all()
    assert exps.min() >= -3 and exps.max() <= 3
    np.testing.assert_array_equal(np.abs(x), (signs != 0) * np.exp2(exps.astype(np.float64))[:, :, None])
    for dt in ("bf16", "fp16"):
        np.testing.assert_array_equal(mr.round_dtype(x, dt).astype(np.float64), x)
    k = mr.pair_counts(signs)
    np.testing.assert_array_equal(mr.cosine64(x) * m, k)
    if N > 100:          # the fp32 orders and torch below on a slice of a very wide bank
        signs, x, k = signs[:, :64], x[:, :64], k[:, :64]
    x32 = x.astype(np.float32)
    for order in (slice(None), slice(None, None, -1)):
        xs = x32[:, :, order]
        ss = np.add.accumulate(xs * xs, axis=-1, dtype=np.float32)[..., -1]
        xn = xs / np.maximum(np.sqrt(ss), np.float32(1e-8))[..., None]
        cos = np.add.accumulate(xn[:-1] * xn[1:], axis=-1, dtype=np.float32)[..., -1]
        assert cos.dtype == np.float32
        np.testing.assert_array_equal(cos.astype(np.float64) * m, k)
    for dt in mr.DTYPES:
        xt = torch.from_numpy(x).to(TDT[dt])
        cos = torch.nn.functional.cosine_similarity(xt[:-1], xt[1:], dim=-1)
        assert cos.dtype == TDT[dt]
        np.testing.assert_array_equal(cos.double().numpy() * m, k)


def test_tiled_bank_has_distinct_rows_with_equal_cosines():
    signs, exps, x = mr.lattice_bank(3, 70, 70, 64, 64, 5)
    k = mr.pair_counts(signs)
    np.testing.assert_array_equal(k[:, :5], k[:, 65:])
    assert not np.array_equal(x[:, :5], x[:, 65:])


def bf16_bits(x):
    return torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("case", [c for c in mr.CHAIN_CASES if c.T <= 1100], ids=lambda c: "%dx%dx%d_t%d_%s" % (
    c.T, c.N, c.C, c.tgt, "sync" if c.sync else "async"))
def test_integer_chain_equals_the_c_oracle(case):
    """orc.mallm_compress (the C restatement of the reference's loop, fp32 and bf16 bits) on the lattice banks: the
    per-step pairs and the final bank bit-equal to the integer chain's."""
    signs, _, x = mr.case_bank(case)
    for dt in [d for d in case.dtypes if d != "fp16"]:
        ch = mr.hard_chain(signs, case.m, case.tgt, case.sync, dt)
        xin = x.astype(np.float32) if dt == "fp32" else bf16_bits(x)
        bank, _, steps = orc.mallm_compress(xin, case.tgt, case.sync, True)
        np.testing.assert_array_equal(steps, ch.steps)
        idx = ch.idx if ch.idx.ndim == 2 else np.repeat(ch.idx[:, None], case.N, 1)
        np.testing.assert_array_equal(bank, gather(xin, idx))


# ---------------------------------------------------------------------------------------------------
# input conditions of the GPU tests
# ---------------------------------------------------------------------------------------------------
def test_chain_banks_tie_and_reach_head_and_tail():
    """Every run of tests/test_mallm_gpu.py on a lattice bank: at least half of its decisions fall to the first-index
    rule (a single pair, T = 2, cannot tie); every bank drops its head frame and chooses its last pair at least once."""
    heads, tails = {}, {}
    for c in mr.CHAIN_CASES:
        signs, _, _ = mr.case_bank(c)
        bank = (c.seed, c.T, c.N, c.C, c.m, c.width)
        for dt in c.dtypes:
            ch = mr.hard_chain(signs, c.m, c.tgt, c.sync, dt)
            assert ch.idx.shape == ((c.tgt,) if c.sync else (c.tgt, c.N)) and (np.diff(ch.idx, axis=0) > 0).all()
            if c.T > 2:
                assert ch.tie_share >= 0.5, (c, dt, ch.tie_share)
            heads[bank] = heads.get(bank, 0) + ch.head_drops
            tails[bank] = tails.get(bank, 0) + ch.tail_drops
    for bank in heads:
        assert heads[bank] >= 1 and tails[bank] >= 1, (bank, heads[bank], tails[bank])
    seed, T, N, C, m, tgt = mr.FIXTURE_BANK
    signs, _, _ = mr.lattice_bank(seed, T, N, C, m)
    for sync in (False, True):
        for dt in mr.DTYPES:
            ch = mr.hard_chain(signs, m, tgt, sync, dt)
            assert ch.tie_share >= 0.5 and ch.head_drops >= 1 and ch.tail_drops >= 1, (sync, dt, ch)


@pytest.mark.parametrize("seed,T,N,C,sync", mr.STEP_CASES)
def test_random_step_banks_have_a_safe_top2_gap(seed, T, N, C, sync):
    x = synth.frames_iid(seed, T, N, C)[0].astype(np.float64)
    sim = mr.cosine64(x)
    if sync:
        sim = sim.mean(1, keepdims=True)
    assert mr.top2_gap(sim).min() >= mr.step_gap_bar(N, C, sync)

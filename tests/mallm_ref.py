"""Plain reference of the MA-LLM / MA-LLM-hard merges (include/retake_hip.h §C), for tests.

    rtk_adjacent_cosine   cosine64            cos(x[t], x[t+1]) per patch position, float64
    rtk_mallm_argmax      argmax_step         first arg-max per patch position (of the patch mean when sync)
    rtk_mallm_merge       soft_merge, hard_merge   torch-CPU expressions in the bank's dtype, one rounding per op
    rtk_mallm_hard_chain  hard_chain (lattice banks, integer-only) and hard_chain64 (any bank, float64)

The arg-max rule everywhere: the maximum wins, NaN counts as the maximum, and among equals (several NaNs included) the
lowest index wins - what torch.max(dim) does.

Lattice banks make the arg-max decisions exact.  A row has exactly m non-zero entries, each +-2^e with one e per row, so
||x|| = 2^e sqrt(m), every normalised entry is +-1/sqrt(m), every product is +-1/m and the cosine is k/m for the integer
k = sum(sign_a * sign_b) - in fp32, bf16 and fp16 alike and whatever the summation order (m in {4, 16, 64}: sqrt(m) is
a power of two).  hard_chain works on k alone.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

DTYPES = ("fp32", "bf16", "fp16")
NAN_K = np.iinfo(np.int64).max   # "this pair's cosine is NaN" among the integer similarities: above every number


def round_dtype(a, dtype: str) -> np.ndarray:
    """fp32 values -> the nearest value of `dtype` (ties to even), returned as fp32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "fp32":
        return a
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    assert dtype == "bf16", dtype
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), a, r)


def eps_of(dtype: str) -> float:
    """F.cosine_similarity's eps = 1e-8 as the tensor dtype holds it: fp16 has no such number (0)."""
    return float(round_dtype(np.full(1, 1e-8, np.float32), dtype)[0])


# ---------------------------------------------------------------------------------------------------
# lattice banks
# ---------------------------------------------------------------------------------------------------
def lattice_bank(seed: int, T: int, N: int, C: int, m: int, width: int = 0):
    """A walk per patch position: every frame is a duplicate of the previous one (p = 0.15), a cut to a fresh row
    (p = 0.08), or the previous row with 1-3 signs flipped (and a fresh exponent).  width > 0: the walk is drawn for
    `width` patch positions and tiled along N, every copy with its channels rolled and its exponents shifted - rows
    that differ while their cosines agree, so that the patch mean of a wide bank still ties.
    Returns (signs [T,N,C] int8 in {-1, 0, 1} with m non-zeros per row, exps [T,N] in [-3, 3], x [T,N,C] float64)."""
    assert m in (4, 16, 64) and m <= C
    if 0 < width < N:
        s, e, _ = lattice_bank(seed, T, width, C, m)
        signs = np.stack([np.roll(s[:, n % width], n // width, axis=-1) for n in range(N)], axis=1)
        exps = np.stack([(e[:, n % width] + 3 + n // width) % 7 - 3 for n in range(N)], axis=1)
        return signs, exps, signs.astype(np.float64) * np.exp2(exps.astype(np.float64))[:, :, None]
    rng = np.random.default_rng(seed)
    rows = np.arange(N)

    def fresh(count):
        s = np.zeros((count, C), dtype=np.int8)
        support = np.argsort(rng.random((count, C)), axis=1)[:, :m]
        s[np.arange(count)[:, None], support] = rng.integers(0, 2, size=(count, m), dtype=np.int8) * 2 - 1
        return s

    signs = np.empty((T, N, C), dtype=np.int8)
    exps = np.empty((T, N), dtype=np.int64)
    signs[0], exps[0] = fresh(N), rng.integers(-3, 4, size=N)
    for t in range(1, T):
        u = rng.random(N)
        dup, cut = u < 0.15, (u >= 0.15) & (u < 0.23)
        prev = signs[t - 1]
        # flip the `nflip` non-zero entries with the smallest random keys
        keys = np.where(prev != 0, rng.random((N, C), dtype=np.float32), np.float32(2.0))
        nflip = rng.integers(1, 4, size=N)
        row = np.where(keys <= np.partition(keys, 2, axis=1)[rows, nflip - 1][:, None], -prev, prev)
        row[cut] = fresh(int(cut.sum()))
        e = rng.integers(-3, 4, size=N)
        signs[t] = np.where(dup[:, None], prev, row)
        exps[t] = np.where(dup, exps[t - 1], e)
    x = signs.astype(np.float64) * np.exp2(exps.astype(np.float64))[:, :, None]
    return signs, exps, x


def pair_counts(signs: np.ndarray, dtype: str = "fp32") -> np.ndarray:
    """m * cos of every adjacent pair of a lattice bank, as integers [T-1,N].  A pair with an all-zero row: 0 where the
    dtype clamps the norm to eps > 0, NAN_K in fp16 (0 / 0)."""
    s = signs.astype(np.int32)
    k = (s[:-1] * s[1:]).sum(-1).astype(np.int64)
    if eps_of(dtype) == 0.0:
        zero = ~signs.any(-1)
        k[zero[:-1] | zero[1:]] = NAN_K
    return k


# ---------------------------------------------------------------------------------------------------
# the single step
# ---------------------------------------------------------------------------------------------------
def cosine64(x: np.ndarray, dtype: str = "fp32") -> np.ndarray:
    """x [T,N,C] -> cos [T-1,N] in float64: sum_c (a_c / max(||a||, eps)) (b_c / max(||b||, eps)), eps as `dtype` has it."""
    x = np.asarray(x, dtype=np.float64)
    nrm = np.maximum(np.sqrt((x * x).sum(-1)), eps_of(dtype))
    with np.errstate(divide="ignore", invalid="ignore"):
        xn = x / nrm[..., None]
    return (xn[:-1] * xn[1:]).sum(-1)


def cosine_ops(x: np.ndarray, dtype: str = "fp32") -> np.ndarray:
    """The same cosines as a chain of torch-CPU ops on a tensor of `dtype`, each op rounding once to it - norm,
    clamp_min(eps), quotient, product, sum: what a 16-bit bank's near-ties are decided by.  x holds values of `dtype`."""
    import torch

    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).to({"fp32": torch.float32, "bf16": torch.bfloat16,
                                                                "fp16": torch.float16}[dtype])
    xn = xt / torch.linalg.vector_norm(xt, dim=-1, keepdim=True).clamp_min(1e-8)
    return (xn[:-1] * xn[1:]).sum(-1).double().numpy()


def first_max(v: np.ndarray) -> np.ndarray:
    """Index of the first maximum along axis 0, NaN counting as the maximum."""
    v = np.asarray(v)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        finite_best = np.where(nan, -np.inf, v).argmax(0)   # numpy's argmax: first occurrence
    return np.where(nan.any(0), nan.argmax(0), finite_best).astype(np.int64)


def patch_mean(row_sum, N: int, dtype: str) -> np.ndarray:
    """similarity_matrix.mean(-1) from the exact per-frame sum: one fp32 division by N, one rounding to the dtype."""
    with np.errstate(invalid="ignore"):
        return round_dtype(np.asarray(row_sum, dtype=np.float64).astype(np.float32) / np.float32(N), dtype)


def argmax_step(sim: np.ndarray, sync: bool, N: int, dtype: str = "fp32") -> np.ndarray:
    """sim [T1,N] -> idx [N] int64: the first arg-max per patch position, of the patch-mean row when sync."""
    sim = np.asarray(sim, dtype=np.float64)
    assert sim.shape[1] == N
    if not sync:
        return first_max(sim)
    sums = np.array([math.fsum(r) if not np.isnan(r).any() else np.nan for r in sim])
    return np.full(N, first_max(patch_mean(sums, N, dtype)), dtype=np.int64)


def hard_merge(x, idx):
    """torch x [T,N,C], idx [N] -> out[t] = x[t + (t >= idx)]: the first frame of the pair leaves."""
    import torch

    T, N, C = x.shape
    t = torch.arange(T - 1)[:, None]
    d = t + (t >= idx[None]).long()
    return x.gather(0, d[:, :, None].expand(-1, -1, C))


def soft_merge(x, sizes, idx):
    """torch x [T,N,C], sizes [T,N] (dtype of x), idx [N] -> (out [T-1,N,C], sizes_out [T-1,N]), every torch op rounding
    once to the dtype, in rtk_mallm_merge's order: out[t] = (x[d] * s[d]) / s[d] with d = t + (t > idx), and at t = idx
    ((x[i] * s[i]) + (x[i+1] * s[i+1])) / (s[i] + s[i+1])."""
    import torch

    T, N, C = x.shape
    cols = torch.arange(N)
    t = torch.arange(T - 1)[:, None]
    d = t + (t > idx[None]).long()
    den = sizes.gather(0, d)
    num = x.gather(0, d[:, :, None].expand(-1, -1, C)) * den[:, :, None]
    src = x[idx + 1, cols] * sizes[idx + 1, cols][:, None]
    num[idx, cols] = num[idx, cols] + src
    den[idx, cols] = den[idx, cols] + sizes[idx + 1, cols]
    return num / den[:, :, None], den


# ---------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------
Chain = namedtuple("Chain", "idx steps tie_share head_drops tail_drops")
Chain.__doc__ = """idx: the surviving frames, ascending ([tgt,N], or [tgt] when sync); steps [T-tgt,N]: the merged pair of
every step as an index into the bank of that step; tie_share: the share of decisions in which the maximum occurred more
than once; head_drops / tail_drops: decisions that dropped the first surviving frame / chose the last pair."""


def hard_chain(signs: np.ndarray, m: int, tgt: int, sync: bool, dtype: str = "fp32") -> Chain:
    """MA-LLM-hard looped down to tgt frames on a lattice bank, on the integers k = m * cos alone.  sync compares the
    patch means as the dtype holds them (patch_mean of the exact sum: in 16 bits distinct sums can round to a tie)."""
    T, N, C = signs.shape
    s = signs.astype(np.int32)
    zero_nan = (~signs.any(-1)) if eps_of(dtype) == 0.0 else np.zeros((T, N), dtype=bool)
    k0 = pair_counts(signs, dtype)

    def pair(a, b, n):   # k of frames a, b at patch positions n (an index or a slice)
        k = (s[a, n] * s[b, n]).sum(-1).astype(np.int64)
        return np.where(zero_nan[a, n] | zero_nan[b, n], NAN_K, k)

    def key_of(k):       # [.., N] integers -> what the sync arg-max compares
        nan = (k == NAN_K).any(-1)
        mean = patch_mean(np.where(k == NAN_K, 0, k).sum(-1) / m, N, dtype).astype(np.float64)
        return np.where(nan, np.inf, mean.reshape(nan.shape))

    ties = heads = tails = decisions = 0
    out, steps = [], []
    for n in ([slice(None)] if sync else range(N)):
        alive = np.arange(T)
        ks = k0.copy() if sync else k0[:, n].copy()
        keys = key_of(ks) if sync else ks
        col_steps = []
        while len(alive) > tgt:
            j = int(keys.argmax())           # first occurrence of the maximum; NaN stands above every number
            ties += int((keys == keys[j]).sum() > 1)
            heads += j == 0
            tails += j == len(keys) - 1
            decisions += 1
            col_steps.append(j)
            alive = np.delete(alive, j)      # the pair's first frame leaves; alive[j] is now its second
            if j > 0:
                ks[j - 1] = pair(alive[j - 1], alive[j], n)
                keys[j - 1] = key_of(ks[j - 1]) if sync else ks[j - 1]
            ks, keys = np.delete(ks, j, axis=0), np.delete(keys, j)
        out.append(alive)
        steps.append(col_steps)
    idx = out[0] if sync else np.stack(out, axis=1)
    st = np.asarray(steps, dtype=np.int64).T.reshape(T - tgt, 1 if sync else N)
    st = np.repeat(st, N, axis=1) if sync else st
    return Chain(idx.astype(np.int64), st, ties / max(decisions, 1), int(heads), int(tails))


def hard_chain64(x: np.ndarray, tgt: int, sync: bool, dtype: str = "fp32", cosine=cosine64):
    """The same loop on any bank, every step from the float64 cosines of the current bank (or cosine_ops').
    Returns (idx [tgt,N] - every column alike when sync -, steps [T-tgt,N])."""
    x = np.asarray(x, dtype=np.float64)
    T, N, C = x.shape
    alive = np.tile(np.arange(T)[:, None], (1, N))
    steps = []
    while alive.shape[0] > tgt:
        bank = np.take_along_axis(x, alive[:, :, None], 0)
        idx = argmax_step(cosine(bank, dtype), sync, N, dtype)
        t = np.arange(alive.shape[0] - 1)[:, None]
        alive = np.take_along_axis(alive, t + (t >= idx[None]), 0)
        steps.append(idx)
    return alive, (np.stack(steps) if steps else np.zeros((0, N), np.int64))


def soft_chain(xt, tgt: int, sync: bool, dtype: str = "fp32", cosine=cosine64):
    """MA-LLM (soft) looped down to tgt frames: float64 cosines of the current bank choose the pair, soft_merge merges.
    torch xt [T,N,C] -> (bank [tgt,N,C], sizes [tgt,N], steps)."""
    import torch

    bank, sizes, steps = xt, torch.ones_like(xt[:, :, 0]), []
    while bank.shape[0] > tgt:
        idx = argmax_step(cosine(bank.double().numpy(), dtype), sync, bank.shape[1], dtype)
        bank, sizes = soft_merge(bank, sizes, torch.from_numpy(idx))
        steps.append(idx)
    return bank, sizes, steps


def top2_gap(sim: np.ndarray) -> np.ndarray:
    """Per column: the largest value minus the second largest (inf for a single row)."""
    if sim.shape[0] < 2:
        return np.full(sim.shape[1:], np.inf)
    s = np.sort(sim, axis=0)
    return s[-1] - s[-2]


# ---------------------------------------------------------------------------------------------------
# The lattice banks of tests/test_mallm_gpu.py.  tests/test_mallm_ref_cpu.py asserts their input conditions: in every
# run at least half of the decisions fall to the first-index rule, and every bank drops a head frame and a tail pair.
# ---------------------------------------------------------------------------------------------------
LatticeCase = namedtuple("LatticeCase", "seed T N C m width tgt sync dtypes")
_ALL, _F32 = DTYPES, ("fp32",)
CHAIN_CASES = [
    LatticeCase(3, 2, 3, 8, 4, 0, 1, False, _ALL), LatticeCase(3, 2, 3, 8, 4, 0, 1, True, _ALL),       # a single step
    LatticeCase(14, 3, 2, 8, 4, 0, 1, False, _ALL), LatticeCase(14, 3, 2, 8, 4, 0, 1, True, _ALL),
    LatticeCase(1, 130, 3, 8, 4, 0, 1, False, _ALL),        # every unlink, repeated head drops (frame T-1 is left)
    LatticeCase(1, 130, 3, 8, 4, 0, 129, False, _ALL),      # one drop
    LatticeCase(1, 130, 3, 8, 4, 0, 30, False, _ALL),       # ... and a target at which the survivors tell the order
    LatticeCase(1, 70, 5, 64, 64, 0, 9, False, _ALL),
    LatticeCase(1, 70, 17, 64, 64, 2, 9, True, _ALL),       # the sync kernel's second wave trip over patches
    LatticeCase(3, 70, 70, 64, 64, 5, 9, True, _ALL),       # second lane trip in the patch mean; N no power of two
    LatticeCase(1, 1100, 2, 8, 4, 0, 3, False, _ALL),
    LatticeCase(1, 1100, 2, 8, 4, 0, 500, True, _ALL),      # T beyond the sync kernel's workgroup
    LatticeCase(1, 4200, 2, 8, 4, 0, 4100, False, _ALL), LatticeCase(1, 4200, 2, 8, 4, 0, 4100, True, _ALL),  # LDS opt-in
    LatticeCase(1, 4200, 2, 8, 4, 0, 2000, False, _F32),    # ... and deep enough to reach the bank's head and tail
    LatticeCase(2, 20, 2, 1540, 64, 0, 5, False, _F32), LatticeCase(2, 20, 2, 1540, 64, 0, 5, True, _F32),   # vpl 7 -> 8
]

FIXTURE_BANK = (7, 40, 6, 8, 4, 11)   # seed, T, N, C, m, tgt of tests/golden/*mallm_lattice_*.npz (gen_golden.py)


def case_bank(c: LatticeCase):
    return lattice_bank(c.seed, c.T, c.N, c.C, c.m, c.width)

# rtk_adjacent_cosine on lattice banks: (seed, T, N, C, m, dtypes)
COS_CASES = [
    (11, 2, 1, 8, 4, _ALL), (12, 9, 3, 8, 4, _ALL), (13, 70, 5, 64, 64, _ALL),
    (14, 20, 2, 7, 4, _ALL),                   # odd C: the generic kernel in cosine mode
    (15, 20, 2, 260, 64, _F32),                # 2 vectors per lane, ragged tail
    (16, 20, 2, 1540, 64, _F32),               # 7 vectors per lane, served by the instantiation for 8
    (17, 20, 2, 4104, 64, ("bf16",)),          # 9 vectors per lane, served by the instantiation for 10
    (18, 130, 9000, 8, 4, ("fp32", "bf16")),   # more patch positions than resident waves: 64-row strips and their halos
]
# one step on random fp32 data (synth.frames_iid): (seed, T, N, C, sync).  The float64 arg-max is the truth where the
# float64 top-2 gap of every column is at least step_gap_bar: twice the error bound of an fp32 cosine (C fused
# multiply-adds, two divisions and a product per term, the norms: (C + 8) 2^-24 on unit operands) plus, for the patch
# mean, N fp32 additions - and that twice over.
STEP_CASES = [(1, 300, 8, 8, False), (1, 300, 70, 8, True)]


def step_gap_bar(N: int, C: int, sync: bool) -> float:
    return 4.0 * (C + 8 + (N if sync else 0)) * 2.0 ** -24

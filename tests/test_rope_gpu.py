"""Every entry point of csrc/rope.hip against tests/rope_ref.py (the host restatement of its arithmetic) and against float64:
rtk_rope_rotate_rows, rtk_rope_shift, rtk_rope_shift_segments, rtk_position_shift, rtk_rope_merge - at their own edges
(one-row tails, the smallest head_dim of each vector width, padded strides, the 8192-id sweep of the id shift), not through
whole-cache fixtures.  Each test prints its worst error as a fraction of its derived bound (profiles/rope_parity_stats.txt).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rope_ref as rr
import synth

pytestmark = pytest.mark.gpu

YARN = synth.YARN_FACTOR4_ATTENTION_SCALING
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def dev():
    return torch.device("cuda:0")


def _note(line: str):
    """Print a measured figure; also append it to $RETAKE_ROPE_STATS when set (profiles/rope_parity_stats.txt)."""
    print(line, flush=True)
    path = os.environ.get("RETAKE_ROPE_STATS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _name(dtype):
    return str(dtype)[6:]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(INT_VIEW[t.dtype]) if t.dtype in INT_VIEW else t


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _sections(sec):
    return ((C.c_int * len(sec))(*sec), len(sec)) if sec else (None, 0)


def _values(seed, shape, dtype):
    """1.7 * N(0, 1) rounded to `dtype`, on the host."""
    return torch.from_numpy((1.7 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)).to(dtype)


def _mixed_ids(rng, n):
    """ids mixing 0 ... 2500 and video-scale values up to 300 000, in no order"""
    small = rng.integers(0, 2501, n)
    large = rng.integers(2500, 300001, n)
    return np.where(rng.uniform(size=n) < 0.5, small, large).astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# rtk_rope_rotate_rows
# ---------------------------------------------------------------------------------------------------
ROTATE_CASES = [(torch.float32, 128, 3, [16, 24, 24]), (torch.bfloat16, 128, 3, [16, 24, 24]), (torch.float16, 128, 1, None),
                (torch.bfloat16, 128, 1, None), (torch.bfloat16, 64, 3, [8, 12, 12]), (torch.float32, 16, 3, [2, 3, 3]),
                (torch.bfloat16, 16, 1, None), (torch.float32, 8, 1, None), (torch.bfloat16, 256, 1, None)]


def _rotate_rows(k, rows, ids, inv, scaling, sec, dtype):
    import retake._native as nv

    layers, H, cap, D = k.shape
    _, P, ld = ids.shape
    secp, nsec = _sections(sec)
    rc = nv.lib.rtk_rope_rotate_rows(nv.ptr(k), k.stride(0), k.stride(1), layers, H, rows, D, nv.dtype_code(k), nv.ptr(ids),
                                     P * ld, ld, P, nv.ptr(inv), scaling, secp, nsec, nv.round_mode(dtype), nv.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype,D,P,sec", ROTATE_CASES, ids=[f"{_name(c[0])}-D{c[1]}-P{c[2]}" for c in ROTATE_CASES])
def test_rotate_rows_equals_host_restatement_and_float64(dtype, D, P, sec):
    """rtk_rope_rotate_rows over a [layers, H, cap, D] buffer with its real strides, padded ids [layers, P, ld]: (a) bit
    equality with rope_ref (tables and one rounding per op), (b) the derived float64 bound on its own, (c) the NaN rows
    behind `rows` and the ids bitwise untouched, (d) rows = 0 writes nothing - at 1 row, and at 33 / 257 rows (a one-row
    tail behind whole workgroups of 32 rows at D 128 in 16 bit), scaling 1 and YaRN."""
    import retake._native as nv

    layers, H = 3, 4
    inv_np = synth.inv_freq(D)
    inv = torch.from_numpy(inv_np).to(dev())
    worst = 0.0
    for rows in (1, 33, 257):
        cap, ld = rows + 5, rows + 3
        rng = np.random.default_rng(1000 * D + 10 * rows + P)
        x = _values(rows + D, (layers, H, cap, D), dtype)
        x[:, :, rows:] = float("nan")
        ids = torch.full((layers, P, ld), -123456789, dtype=torch.int64)
        for l in range(layers):
            for p in range(P):
                ids[l, p, :rows] = torch.from_numpy(_mixed_ids(rng, rows))
        if rows > 1:
            ids[0, 0, 0], ids[1, 0, 1] = 0, 300000
        for scaling in (1.0, YARN):
            k = x.clone().to(dev())
            ids_d = ids.clone().to(dev())
            assert _rotate_rows(k, rows, ids_d, inv, scaling, sec, dtype) == 0, nv.lib.rtk_last_error()
            got = k.cpu()
            assert _same_bits(ids_d, ids)                                               # (c)
            assert _same_bits(got[:, :, rows:], x[:, :, rows:])                         # (c): the NaN rows, bit for bit
            for l in range(layers):
                idl = ids[l, :, :rows].numpy()
                cos, sin = rr.tables(idl, inv_np, D, scaling, rr.round_mode(dtype), sec)
                want = rr.rotate(x[l, :, :rows], cos, sin)
                truth, mag = rr.rotate_truth(x[l, :, :rows], rr.angles(idl, inv_np, D, sec), scaling)
                frac = np.abs(got[l, :, :rows].double().numpy() - truth) / rr.rotate_bound(dtype, mag)
                worst = max(worst, float(frac.max()))
                assert frac.max() <= 1.0, (rows, scaling, l, float(frac.max()))         # (b)
                if not _same_bits(got[l, :, :rows], want):                              # (a)
                    bad = (_bits(got[l, :, :rows]) != _bits(want)).nonzero()
                    h, r, d = bad[0].tolist()
                    raise AssertionError(f"rows {rows} scaling {scaling} layer {l}: {bad.shape[0]} elements differ from rope_ref; "
                                         f"first at head {h} row {r} channel {d}: {float(got[l, h, r, d])!r} vs "
                                         f"{float(want[h, r, d])!r} (id rows {idl[:, r].tolist()})")
        k = x.clone().to(dev())                                                         # (d)
        assert _rotate_rows(k, 0, ids.to(dev()), inv, YARN, sec, dtype) == 0
        assert _same_bits(k.cpu(), x)
    _note(f"rotate_rows[{_name(dtype)} D{D} P{P}]: bit-equal to rope_ref at rows 1/33/257, scaling 1 and YaRN; worst error vs "
          f"float64 {worst:.3f} of the bound ({6 if dtype == torch.float32 else 4} u (|x1 cos| + |x2 sin|))")


# ---------------------------------------------------------------------------------------------------
# rtk_rope_shift / rtk_rope_shift_segments
# ---------------------------------------------------------------------------------------------------
def _shift(k, n, delta_dev, inv, P, sec):
    """rtk_rope_shift on k [H, cap, D] (rows [0, n) of every head)."""
    import retake._native as nv

    H, cap, D = k.shape
    secp, nsec = _sections(sec)
    return nv.lib.rtk_rope_shift(nv.ptr(k), k.stride(0), H, n, D, nv.dtype_code(k), nv.ptr(delta_dev), nv.ptr(inv), P, secp, nsec,
                                 nv.stream())


@pytest.mark.parametrize("D,P,sec", [(128, 1, None), (128, 3, [16, 24, 24]), (16, 1, None)], ids=["D128-P1", "D128-P3", "D16-P1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
def test_shift_against_float64(dtype, D, P, sec):
    """rtk_rope_shift in place on [3, n + 4, D] (padded stride_h, NaN tail), delta read from the device: the derived bound
    against the float64 value of the expression; delta 0 is the identity bit for bit; with M-RoPE the channels of the height
    / width rows and - always - the padding rows keep their bits; n = 0 touches nothing."""
    import retake._native as nv

    H = 3
    inv_np = synth.inv_freq(D)
    inv = torch.from_numpy(inv_np).to(dev())
    worst = 0.0
    for n in (1, 700):
        cap = n + 4
        x = _values(n + D + P, (H, cap, D), dtype)
        x[:, n:] = float("nan")
        for delta in (0, 1, -5, 4097, 250000):
            k = x.clone().to(dev())
            dl = torch.tensor([delta], dtype=torch.int64, device=dev())
            assert _shift(k, n, dl, inv, P, sec) == 0, nv.lib.rtk_last_error()
            torch.cuda.synchronize()
            got = k.cpu()
            assert _same_bits(got[:, n:], x[:, n:])
            want, mag = rr.shift(x[:, :n], delta, inv_np, P, sec)
            frac = np.abs(got[:, :n].double().numpy() - want) / rr.shift_bound(dtype, mag)
            worst = max(worst, float(frac.max()))
            assert frac.max() <= 1.0, (n, delta, float(frac.max()))
            if delta == 0:
                assert _same_bits(got, x)
            if P == 3:
                off = torch.from_numpy(np.concatenate([rr.rowsel(D, P, sec)[:D // 2] != 0] * 2))
                assert off.nonzero().flatten().tolist() == list(range(16, 64)) + list(range(80, 128))
                assert _same_bits(got[:, :n][..., off], x[:, :n][..., off])
    k = x.clone().to(dev())
    assert _shift(k, 0, torch.tensor([9], dtype=torch.int64, device=dev()), inv, P, sec) == 0
    torch.cuda.synchronize()
    assert _same_bits(k.cpu(), x)
    _note(f"shift[{_name(dtype)} D{D} P{P}]: worst error vs float64 {worst:.3f} of the bound ((u + 2^-21) (|x1 c| + |x2 s|)) over "
          f"n 1/700, delta 0/1/-5/4097/250000")


@pytest.mark.parametrize("P,sec", [(1, None), (3, [16, 24, 24])], ids=["P1", "P3"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_name)
def test_shift_segments_equals_one_shift_per_segment(dtype, P, sec):
    """rtk_rope_shift_segments over [2, 2, 3 * seg, D] with a [world, layers] table of positive, zero and negative steps ==
    world x layers calls of rtk_rope_shift on the segments of a copy, bit for bit; seg = 0 touches nothing."""
    import retake._native as nv

    layers, H, world, seg, D = 2, 2, 3, 5, 128
    inv = torch.from_numpy(synth.inv_freq(D)).to(dev())
    table = torch.tensor([[3, -2], [0, 70001], [-11, 0]], dtype=torch.int64, device=dev())
    x = _values(77 + P, (layers, H, world * seg, D), dtype)
    secp, nsec = _sections(sec)

    def segments(k, seg_):
        return nv.lib.rtk_rope_shift_segments(nv.ptr(k), k.stride(0), k.stride(1), layers, H, world, seg_, D, nv.dtype_code(k),
                                              nv.ptr(table), nv.ptr(inv), P, secp, nsec, nv.stream())

    a = x.clone().to(dev())
    assert segments(a, seg) == 0, nv.lib.rtk_last_error()
    b = x.clone().to(dev())
    es = b.element_size()
    for r in range(world):
        for l in range(layers):
            part = C.c_void_p(b.data_ptr() + (l * b.stride(0) + r * seg * D) * es)
            dl = C.c_void_p(table.data_ptr() + (r * layers + l) * 8)
            assert nv.lib.rtk_rope_shift(part, b.stride(1), H, seg, D, nv.dtype_code(b), dl, nv.ptr(inv), P, secp, nsec,
                                         nv.stream()) == 0, nv.lib.rtk_last_error()
    torch.cuda.synchronize()
    assert _same_bits(a.cpu(), b.cpu())
    assert not _same_bits(a.cpu()[1, :, seg:2 * seg], x[1, :, seg:2 * seg])    # table[1, 1] == 70001: rotated
    assert _same_bits(a.cpu()[0, :, seg:2 * seg], x[0, :, seg:2 * seg])        # table[1, 0] == 0: the identity
    c = x.clone().to(dev())
    assert segments(c, 0) == 0
    torch.cuda.synchronize()
    assert _same_bits(c.cpu(), x)
    _note(f"shift_segments[{_name(dtype)} P{P}]: bit-equal to {world * layers} rtk_rope_shift calls on the segments; seg 0 is a no-op")


# ---------------------------------------------------------------------------------------------------
# rtk_position_shift
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 20000])
def test_position_shift_across_block_and_sweep_boundaries(n):
    """rtk_position_shift on row 0 of a [3, 1, n] tensor, n around one workgroup (1024 ids) and one sweep (8192 ids): the
    row moves so that its first id is prev + 1 (0 without a previous id), rows 1 and 2 keep their bits, a row that already
    continues prev is left alone.  Expected values: int64 torch arithmetic."""
    import retake._native as nv

    rng = np.random.default_rng(n)
    ids = torch.from_numpy(rng.integers(-5000, 300000, (3, 1, n)).astype(np.int64))
    ids[0, 0, 0] = -17
    prev = torch.tensor([41], dtype=torch.int64, device=dev())
    cont = ids.clone()
    cont[0, 0] += 42 - cont[0, 0, 0]
    for src, pv, first in ((ids, None, 0), (ids, prev, 42), (cont, prev, 42)):
        t = src.clone().to(dev())
        assert nv.lib.rtk_position_shift(nv.ptr(t), n, nv.ptr(pv), nv.stream()) == 0, nv.lib.rtk_last_error()
        torch.cuda.synchronize()
        want = src.clone()
        want[0, 0] += first - src[0, 0, 0]
        assert torch.equal(t.cpu(), want)
        assert int(t[0, 0, 0]) == first and torch.equal(t.cpu()[1:], src[1:])
        if src is cont:
            assert torch.equal(t.cpu(), src)
    assert int(prev[0]) == 41
    _note(f"position_shift[n {n}]: exact (no prev -> 0, prev 41 -> 42, already continuous: untouched; rows 1, 2 untouched)")


# ---------------------------------------------------------------------------------------------------
# rtk_rope_merge
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 777])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
def test_merge_selects_the_section_rows_exactly(dtype, L):
    """rtk_rope_merge: out[l, d] == float(in[row[d], l, d]) exactly, M-RoPE sections [16, 24, 24] and plain RoPE."""
    import retake._native as nv

    D = 128
    for P, sec in ((3, [16, 24, 24]), (1, None)):
        cin, sin_ = _values(L + P, (P, L, D), dtype), _values(L + P + 50, (P, L, D), dtype)
        secp, nsec = _sections(sec)
        out_c = torch.full((L, D), float("nan"), dtype=torch.float32, device=dev())
        out_s = torch.full_like(out_c, float("nan"))
        cin_d, sin_d = cin.to(dev()), sin_.to(dev())
        assert nv.lib.rtk_rope_merge(nv.ptr(cin_d), nv.ptr(sin_d), P, L, D, nv.dtype_code(cin), secp, nsec,
                                     nv.ptr(out_c), nv.ptr(out_s), nv.stream()) == 0, nv.lib.rtk_last_error()
        torch.cuda.synchronize()
        row = torch.from_numpy(rr.rowsel(D, P, sec))
        d = torch.arange(D)
        for got, src in ((out_c, cin), (out_s, sin_)):
            want = src.float()[row[None, :], torch.arange(L)[:, None], d[None, :]]
            assert _same_bits(got.cpu(), want)
    _note(f"merge[{_name(dtype)} L{L}]: exact for P 3 [16, 24, 24] and P 1")

"""rtk_pivotkv_renumber_batched alone, on the GPU, against tests/renumber_ref.py (the rule restated: the per-row deltas in
integers, the rotation rebase_ref's float64 one at the kernel's fp32 angles).  The rule is this project's own; the reference
has no counterpart and answer quality is not evaluated.

The frame is test_rebase_gpu.py's: H = 2 heads (test_head_batches: 4, 5, 9) and a guard head of [cap, D] rows, head stride
cap * D with cap = first + rows + 3 guard rows, ids [P, cap], first in {0, 5}, several layers in one call with distinct slots
and a pre-filled offset array.  The limit is first + 2.  The five layers of a call, over a ramp of 16 rows an id:
  0  holes of random size - 1000 and 100 000 among them - in front of random rows;
  1  every gap <= G and the region right behind the pinned rows: total 0, everything stays bit-equal;
  2  only the gap behind the pinned rows open (37): ids, K and offset must equal, BIT FOR BIT, what
     rtk_pivotkv_rebase_batched leaves on a copy of the same tensors;
  3  a non-monotone id row (negative steps between holes; they stay as they are);
  4  holes, but the last id below the limit: untouched.
Rows: {1, 63, 257} on every geometry, and {T - 1, T, T + 1, 3 T + 5} for the scan tile T = RTK_RENUMBER_TILE on D128_plain
bf16 (the scan's carry across tiles and its ragged last tile; the apply's contiguous row blocks).  G in {1, 4}.

Pass criteria: ids (all rows, guard included), `delta` and the offset array exact against the ref; rows with d = 0, rows
below `first`, guard rows, the guard head and non-temporal channels bit-equal to the snapshot; every rotated element within
rebase_ref.bar = half_ulp(dtype, |ref|) + 6 * 2^-24 (|x1| + |x2|) of rebase_ref.rotate(snapshot row, d of the row) - the
re-base's bar, derived in DESIGN.md §5: the arithmetic per row is the re-base's, so no new constant."""
import ctypes as C

import numpy as np
import pytest
import torch

import rebase_ref as rr
import renumber_ref as nr
import synth

pytestmark = pytest.mark.gpu

H, GUARD = 2, 3
SLOTS = (4, 0, 2, 1, 5)                # the layers' slots in the offset array
OFFSETS0 = (100, 0, 7, 0, 0, -1, 9)    # what the array holds before the call
FIRST_GAP = 37                         # layer 2's only open gap

GEOMETRIES = {   # name: (D, P, sections, dtypes)
    "D128_plain": (128, 1, None, ("bfloat16", "float16", "float32")),
    "D128_mrope": (128, 3, [16, 24, 24], ("bfloat16", "float16", "float32")),
    "D64_mrope_mixed_chunk": (64, 3, [4, 14, 14], ("bfloat16", "float16")),   # chunk 0 holds temporal AND h channels
    "D32_plain": (32, 1, None, ("float32",)),
    "D32_mrope": (32, 3, [4, 6, 6], ()),   # (test_head_batches' alone)
}
CASES = [(g, dt) for g, (_, _, _, dts) in GEOMETRIES.items() for dt in dts]


def dev():
    return torch.device("cuda:0")


def _tile():
    import retake._native as nv

    return nv.RENUMBER_TILE


def _layer_ids(kind, rng, first, rows, limit, P, cap):
    """ids [P, cap] of one layer: pinned ids 0 .. first - 1, the region as `kind` says, guard ids behind it."""
    t = np.arange(cap, dtype=np.int64)
    ramp = np.arange(rows) // 16
    if kind == 1:
        region = first + ramp
    elif kind == 2:
        region = first + FIRST_GAP + ramp
    else:
        k = min(rows, 6)
        at = np.sort(rng.choice(rows, size=k, replace=False))
        size = np.array([1000, 100_000] + list(rng.integers(2, 60, size=4)))[:k]
        step = np.zeros(rows, dtype=np.int64)
        step[at] = rng.permutation(size)
        if kind == 3 and rows > 2:      # negative steps, one of them right behind a hole where there is room
            back = rng.choice(np.arange(1, rows), size=min(rows - 1, 3), replace=False)
            step[back] -= rng.integers(1, 20, size=len(back))
        region = first + 1 + ramp + np.cumsum(step)
        if kind == 4:
            region[-1] = limit - 1      # (a negative step at the end, or for one row a gap of 1)
    t[first:first + rows] = region
    t[first + rows:] = 7_000_000 + np.arange(cap - first - rows)      # guard ids
    return np.stack([t + 100_000 * p for p in range(P)])


def _sec(sections):
    return (C.c_int * len(sections))(*sections) if sections else None


def _call(units, D, dtype, P, inv, sections, limit, gap, offsets, delta):
    import retake._native as nv

    arr = (nv.RenumberUnit * len(units))(*units)
    rc = nv.lib.rtk_pivotkv_renumber_batched(arr, len(units), D, nv.dtype_code(torch.empty(0, dtype=dtype)), P, inv.data_ptr(),
                                             _sec(sections), len(sections) if sections else 0, limit, gap, offsets.data_ptr(),
                                             delta.data_ptr(), nv.stream())
    nv.check(rc, "rtk_pivotkv_renumber_batched")
    torch.cuda.synchronize()


def _call_rebase(units, D, dtype, P, inv, sections, limit, offsets, delta):
    import retake._native as nv

    arr = (nv.RebaseUnit * len(units))(*units)
    rc = nv.lib.rtk_pivotkv_rebase_batched(arr, len(units), D, nv.dtype_code(torch.empty(0, dtype=dtype)), P, inv.data_ptr(),
                                           _sec(sections), len(sections) if sections else 0, limit, offsets.data_ptr(),
                                           delta.data_ptr(), nv.stream())
    nv.check(rc, "rtk_pivotkv_rebase_batched")
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check_layer(name, dtype_name, k_before, k_after, ids_before, ids_after, first, end, rows, limit, gap, inv, sections):
    """-> (total, worst error / bar).  Everything the pass criteria name, for one layer."""
    P, D = ids_before.shape[0], k_before.shape[-1]
    ref_ids, ref_k, d, total = nr.renumber(ids_before.numpy(), k_before.double().numpy(), first, end, rows, limit, gap, inv, sections)
    assert np.array_equal(ids_after.numpy(), ref_ids), (name, "ids")
    if total == 0:
        assert torch.equal(_bits(k_after), _bits(k_before)), (name, "an untriggered layer changed")
        return 0, 0.0
    on = torch.from_numpy(np.concatenate([rr.temporal_pairs(D, P, sections)] * 2))
    moved = torch.zeros(k_before.shape[1], dtype=torch.bool)
    moved[first:first + rows] = torch.from_numpy(d[:rows] > 0)
    same = torch.ones_like(k_before, dtype=torch.bool)
    same[:, moved.nonzero().flatten()[:, None], on.nonzero().flatten()[None, :]] = False
    assert torch.equal(_bits(k_after)[same], _bits(k_before)[same]), (name, "rows with d = 0 / below first / guard rows / other channels")
    rot = moved.numpy()
    got, want, x = k_after.double().numpy()[:, rot], ref_k[:, rot], k_before.double().numpy()[:, rot]
    err, bound = np.abs(got - want), rr.bar(dtype_name, want, x)
    worst = float((err / bound)[..., on.numpy()].max()) if rot.any() else 0.0
    assert np.all(err <= bound), (name, "worst error / bar", worst)
    return total, worst


def _one_call(geometry, dtype_name, first, rows, gap, H=H):
    """The five layers at one (first, rows, G), every pass criterion checked -> worst error / bar.  Every K tensor has a guard
    head behind the H the calls are told of: it keeps its bits."""
    import retake._native as nv

    D, P, sections, _ = GEOMETRIES[geometry]
    dtype = getattr(torch, dtype_name)
    inv = synth.inv_freq(D)
    inv_d = torch.from_numpy(inv).to(dev())
    limit = first + 2
    cap = first + rows + GUARD
    rng = np.random.default_rng(100_000 * gap + 1000 * first + rows)
    guard_rng = np.random.default_rng(77)
    ks, idss, units = [], [], []
    scratch = torch.full((5, rows + 1), -7, dtype=torch.int64, device=dev())     # one guard word behind each row of scratch
    for l in range(5):
        k = np.concatenate([rng.standard_normal((H, cap, D)), guard_rng.standard_normal((1, cap, D))])
        k = torch.from_numpy(1.7 * k.astype(np.float32)).to(dtype).to(dev())
        ids = torch.from_numpy(_layer_ids(l, rng, first, rows, limit, P, cap)).to(dev())
        ks.append(k)
        idss.append(ids)
        units.append(nv.RenumberUnit(k.data_ptr(), cap * D * k.element_size(), first, rows, ids.data_ptr(), cap, first + rows, H,
                                     SLOTS[l], scratch[l].data_ptr()))
    k0 = [k.cpu() for k in ks]
    ids0 = [i.cpu() for i in idss]
    # layer 2 through the re-base, on a copy of the same tensors
    k2, ids2 = ks[2].clone(), idss[2].clone()
    off2 = torch.tensor(OFFSETS0, dtype=torch.int64, device=dev())
    d2 = torch.full((1,), -5, dtype=torch.int64, device=dev())
    _call_rebase([nv.RebaseUnit(k2.data_ptr(), cap * D * k2.element_size(), first, rows, ids2.data_ptr(), cap, first + rows, H, SLOTS[2])],
                 D, dtype, P, inv_d, sections, limit, off2, d2)
    offsets = torch.tensor(OFFSETS0, dtype=torch.int64, device=dev())
    delta = torch.full((5,), -5, dtype=torch.int64, device=dev())
    _call(units, D, dtype, P, inv_d, sections, limit, gap, offsets, delta)
    what = (geometry, dtype_name, first, rows, gap, H)
    assert scratch[:, rows].tolist() == [-7] * 5, (what, "the scan wrote behind its end - first scratch entries")
    expect, worst, totals = list(OFFSETS0), 0.0, []
    for l in range(5):
        ka = ks[l].cpu()
        assert torch.equal(_bits(ka[H]), _bits(k0[l][H])), (what, l, "the head behind the last")
        total, w = _check_layer(what + (l,), dtype_name, k0[l][:H], ka[:H], ids0[l], idss[l].cpu(), first, first + rows, rows, limit,
                                gap, inv, sections)
        expect[SLOTS[l]] += total
        totals.append(total)
        worst = max(worst, w)
    assert delta.tolist() == totals and offsets.tolist() == expect, what
    assert totals[0] > 0 and totals[1] == 0 and totals[2] == FIRST_GAP == int(d2[0]) and totals[3] > 0 and totals[4] == 0, (what, totals)
    assert torch.equal(idss[2], ids2) and torch.equal(_bits(ks[2]), _bits(k2)), (what, "not the re-base's bits")
    assert int(offsets[SLOTS[2]]) == int(off2[SLOTS[2]]), what
    return worst


@pytest.mark.parametrize("gap", [1, 4])
@pytest.mark.parametrize("geometry,dtype_name", CASES, ids=[f"{g}-{d}" for g, d in CASES])
def test_five_layers_in_one_call(geometry, dtype_name, gap):
    worst = 0.0
    for first in (0, 5):
        for rows in (1, 63, 257):
            worst = max(worst, _one_call(geometry, dtype_name, first, rows, gap))
    print(f"renumber[{geometry} {dtype_name} G={gap}]: worst error / bar {worst:.3f}")


HEAD_CASES = [("D128_plain", "bfloat16", 33), ("D32_mrope", "float32", 9)]


@pytest.mark.parametrize("heads", [4, 5, 9])
@pytest.mark.parametrize("geometry,dtype_name,rows", HEAD_CASES, ids=[f"{g}-{d}" for g, d, _ in HEAD_CASES])
def test_head_batches(geometry, dtype_name, rows, heads):
    """The rotation walks a row's heads in batches of 4: one full batch, a full batch and a ragged one of 1 (its loads are
    clamped to the last head, its stores stop there), two full batches and 1.  33 rows at D = 128: one workgroup step of 32
    and a ragged one.  The pass criteria are the file's - the guard head's bits and layer 2's bit-for-bit agreement with
    rtk_pivotkv_rebase_batched among them."""
    worst = max(_one_call(geometry, dtype_name, 5, rows, gap, heads) for gap in (1, 4))
    print(f"renumber[{geometry} {dtype_name} H={heads}]: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("gap", [1, 4])
@pytest.mark.parametrize("rows", ["T-1", "T", "T+1", "3T+5"])
def test_rows_around_the_scan_tile(rows, gap):
    T = _tile()
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[rows]
    for first in (0, 5):
        _one_call("D128_plain", "bfloat16", first, n, gap)


def test_holes_at_every_tile_and_wave_boundary():
    """The scan alone (K rows: 0): a hole in front of every id whose index is a multiple of 64 +- 1 or of the tile +- 1 -
    where a wave's sum, the waves' sums through LDS and the carry across tiles enter."""
    import retake._native as nv

    T = _tile()
    first, n, D = 5, 2 * T + 70, 32
    t = np.arange(first + n + GUARD, dtype=np.int64)
    at = np.array(sorted({i + o for i in list(range(0, n, 64)) + [T, 2 * T] for o in (-1, 0, 1) if 0 <= i + o < n}))
    step = np.zeros(n, dtype=np.int64)
    step[at] = 3 + (at % 11)
    t[first:first + n] = first + np.arange(n) // 16 + np.cumsum(step)
    ids = torch.from_numpy(t[None].copy()).to(dev())
    k = torch.ones((H, 8, D), dtype=torch.float32, device=dev())
    scratch = torch.zeros(n, dtype=torch.int64, device=dev())
    offsets = torch.zeros(1, dtype=torch.int64, device=dev())
    delta = torch.full((1,), -1, dtype=torch.int64, device=dev())
    inv_d = torch.from_numpy(synth.inv_freq(D)).to(dev())
    _call([nv.RenumberUnit(k.data_ptr(), 8 * D * 4, first, 0, ids.data_ptr(), len(t), first + n, H, 0, scratch.data_ptr())], D,
          torch.float32, 1, inv_d, None, 0, 2, offsets, delta)
    d, total = nr.decide(t, first, first + n, 0, 2)
    assert total > 0 and delta.tolist() == [total] and offsets.tolist() == [total]
    assert np.array_equal(scratch.cpu().numpy(), d)
    want = t.copy()
    want[first:first + n] -= d
    assert np.array_equal(ids.cpu().numpy()[0], want)
    assert torch.equal(k, torch.ones_like(k))


def test_more_units_than_one_launch_takes():
    """70 layers (RTK_REBASE_MAX_UNITS = 64: two pairs of launches, the second pair reads its own deltas and scratch), every
    third one untriggered.  `rows` < end - first: the K rows stop 2 short of the ids - the ids beyond them are renumbered
    (a hole lies among them) and no K row beyond `rows` is touched."""
    import retake._native as nv

    assert nv.REBASE_MAX_UNITS == 64
    D, first, n_ids, rows, cap, n, gap = 16, 2, 9, 7, 12, 70, 2
    inv = synth.inv_freq(D)
    inv_d = torch.from_numpy(inv).to(dev())
    rng = np.random.default_rng(3)
    k = torch.from_numpy(rng.standard_normal((n, H, cap, D)).astype(np.float32)).to(torch.bfloat16).to(dev())
    ids = torch.arange(cap, dtype=torch.int64).repeat(n, 1, 1)           # [n, 1, cap]: dense - total 0
    for l in range(n):
        if l % 3:
            ids[l, 0, first + 1 + l % 5:] += 5 + l                       # a hole among the K rows
            ids[l, 0, first + 8:] += 40                                  # ... and one among the ids beyond them
    ids = ids.to(dev())
    k0, ids0 = k.cpu(), ids.cpu()
    scratch = torch.zeros((n, n_ids), dtype=torch.int64, device=dev())
    units = [nv.RenumberUnit(k[l].data_ptr(), cap * D * 2, first, rows, ids[l].data_ptr(), cap, first + n_ids, H, l,
                             scratch[l].data_ptr()) for l in range(n)]
    offsets = torch.zeros(n, dtype=torch.int64, device=dev())
    delta = torch.full((n,), -1, dtype=torch.int64, device=dev())
    _call(units, D, torch.bfloat16, 1, inv_d, None, 0, gap, offsets, delta)
    want = [5 + l - gap + 1 + 40 - gap + 1 if l % 3 else 0 for l in range(n)]      # (a step of 1 + hole closes to gap)
    assert delta.tolist() == want and offsets.tolist() == want
    ka, ia = k.cpu(), ids.cpu()
    for l in range(n):
        total, _ = _check_layer(("unit", l), "bfloat16", k0[l], ka[l], ids0[l], ia[l], first, first + n_ids, rows, 0, gap, inv, None)
        assert total == want[l], l
        assert torch.equal(_bits(ka[l][:, first + rows:]), _bits(k0[l][:, first + rows:])), l
        if want[l]:
            assert int(ia[l][0, first + n_ids - 1]) == int(ids0[l][0, first + n_ids - 1]) - want[l], l


def test_an_empty_region_and_no_units_launch_nothing_harmful():
    import retake._native as nv

    D, cap = 128, 8
    k = torch.ones((H, cap, D), dtype=torch.bfloat16, device=dev())
    ids = (torch.arange(cap, dtype=torch.int64, device=dev()) * 10).view(1, cap).contiguous()
    k0, ids0 = k.clone(), ids.clone()
    inv_d = torch.from_numpy(synth.inv_freq(D)).to(dev())
    offsets = torch.zeros(1, dtype=torch.int64, device=dev())
    delta = torch.full((1,), -1, dtype=torch.int64, device=dev())
    scratch = torch.full((4,), -7, dtype=torch.int64, device=dev())
    _call([nv.RenumberUnit(k.data_ptr(), cap * D * 2, 5, 0, ids.data_ptr(), cap, 5, H, 0, scratch.data_ptr())], D, torch.bfloat16, 1,
          inv_d, None, 0, 4, offsets, delta)
    assert delta.tolist() == [0] and offsets.tolist() == [0] and scratch.tolist() == [-7] * 4
    assert torch.equal(k, k0) and torch.equal(ids, ids0)
    assert nv.lib.rtk_pivotkv_renumber_batched(None, 0, D, nv.RTK_BF16, 1, inv_d.data_ptr(), None, 0, 0, 4, offsets.data_ptr(),
                                               delta.data_ptr(), nv.stream()) == 0

"""rtk_pivotkv_rebase_batched alone, on the GPU, against tests/rebase_ref.py (the rule restated: the decision in integers, the
rotation in float64 at the kernel's fp32 angles).  The rule is this project's own; the reference has no counterpart.

One call carries four layers: one triggered with delta 37, one triggered with delta 1000, one whose last id is below the
limit (delta 11, not applied) and one with delta 0.  Every layer: H = 2 heads (test_head_batches: 4, 5, 9) and a guard head
of [cap, D] rows, head stride cap * D with cap = first + rows + 3 guard rows, ids [P, cap].  first in {0, 5}, rows in
{1, 63, 257}: one row, less than one workgroup step at D = 128 (32 rows), and several steps with a ragged end.

Pass criteria: ids (all rows, guard included) and the offset array exact; untriggered layers bit-equal everywhere; in
triggered layers rows below `first`, guard rows, the guard head and non-temporal channels bit-equal to the snapshot; every
rotated element within rebase_ref.bar = half_ulp(dtype, |ref|) + 6 * 2^-24 (|x1| + |x2|) of the float64 rotation of the
snapshot (the constant is derived in DESIGN.md §5, restated in rebase_ref's docstring; it does not come from a run)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rebase_ref as rr
import synth

pytestmark = pytest.mark.gpu

H, GUARD = 2, 3
DELTAS = (37, 1000, 11, 0)          # layer 2's is not applied: its last id stays below the limit
SLOTS = (4, 0, 2, 1)                # the layers' slots in the offset array
OFFSETS0 = (100, 0, 7, 0, 0, -1)    # what the array holds before the call

GEOMETRIES = {   # name: (D, P, sections, dtypes)
    "D128_plain": (128, 1, None, ("bfloat16", "float16", "float32")),
    "D128_mrope": (128, 3, [16, 24, 24], ("bfloat16", "float16", "float32")),
    "D64_plain": (64, 1, None, ("bfloat16",)),
    "D64_mrope_mixed_chunk": (64, 3, [4, 14, 14], ("bfloat16", "float16")),   # chunk 0 holds temporal AND h channels
    "D32_plain": (32, 1, None, ("float32",)),
    "D32_mrope": (32, 3, [4, 6, 6], ("float32",)),
}
CASES = [(g, dt) for g, (_, _, _, dts) in GEOMETRIES.items() for dt in dts]


def dev():
    return torch.device("cuda:0")


def _layer_ids(first, rows, delta, limit, P, cap, reach):
    """ids [P, cap]: pinned ids 0 .. first - 1, the region from first + delta on (non-decreasing, 16 rows an id); `reach`:
    the last region id is pushed to the limit and beyond, else every region id stays below it."""
    t = np.arange(cap, dtype=np.int64)
    t[first:first + rows] = first + delta + np.arange(rows) // 16
    if reach:
        t[first + rows - 1] = max(t[first + rows - 1], limit + 3)
    else:
        t[first:first + rows] = np.minimum(t[first:first + rows], limit - 1)
    t[first + rows:] = 7_000_000 + np.arange(cap - first - rows)      # guard ids
    ids = np.stack([t + 100_000 * p for p in range(P)])
    return ids


def _call(units, D, dtype, P, inv, sections, limit, offsets, delta):
    import retake._native as nv

    arr = (nv.RebaseUnit * len(units))(*units)
    sec = (C.c_int * len(sections))(*sections) if sections else None
    rc = nv.lib.rtk_pivotkv_rebase_batched(arr, len(units), D, nv.dtype_code(torch.empty(0, dtype=dtype)), P, inv.data_ptr(), sec,
                                           len(sections) if sections else 0, limit, offsets.data_ptr(), delta.data_ptr(),
                                           nv.stream())
    nv.check(rc, "rtk_pivotkv_rebase_batched")
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check_layer(name, dtype_name, k_before, k_after, ids_before, ids_after, first, rows, limit, inv, sections, want_delta):
    P, D = ids_before.shape[0], k_before.shape[-1]
    end = first + rows
    ref_ids, ref_k, delta = rr.rebase(ids_before.numpy(), k_before.double().numpy(), first, end, end, limit, inv, sections)
    assert delta == want_delta, (name, delta, want_delta)
    assert np.array_equal(ids_after.numpy(), ref_ids), (name, "ids")
    if delta == 0:
        assert torch.equal(_bits(k_after), _bits(k_before)), (name, "an untriggered layer changed")
        return 0.0
    same = torch.ones_like(k_before, dtype=torch.bool)
    on = torch.from_numpy(np.concatenate([rr.temporal_pairs(D, P, sections)] * 2))
    same[:, first:end, on] = False
    assert torch.equal(_bits(k_after)[same], _bits(k_before)[same]), (name, "rows below first / guard rows / other channels")
    got = k_after.double().numpy()[:, first:end]
    want = ref_k[:, first:end]
    err = np.abs(got - want)
    bound = rr.bar(dtype_name, want, k_before.double().numpy()[:, first:end])
    worst = float((err / bound)[..., on.numpy()].max())
    assert np.all(err <= bound), (name, "worst error / bar", worst)
    return worst


def _one_call(geometry, dtype_name, first, rows, H=H):
    """The four layers at one (first, rows), every pass criterion checked -> worst error / bar.  Every K tensor has a guard
    head behind the H the call is told of: it keeps its bits."""
    import retake._native as nv

    D, P, sections, _ = GEOMETRIES[geometry]
    dtype = getattr(torch, dtype_name)
    inv = synth.inv_freq(D)
    inv_d = torch.from_numpy(inv).to(dev())
    limit = first + 30
    cap = first + rows + GUARD
    rng = np.random.default_rng(1000 * first + rows)
    guard_rng = np.random.default_rng(77)
    ks, idss, units = [], [], []
    want = [DELTAS[0], DELTAS[1], 0, 0]
    for l in range(4):
        k = np.concatenate([rng.standard_normal((H, cap, D)), guard_rng.standard_normal((1, cap, D))])
        k = torch.from_numpy(1.7 * k.astype(np.float32)).to(dtype).to(dev())
        # (the delta-0 layer reaches the limit too, where it has a second row to do it with)
        reach = l != 2 and not (l == 3 and rows == 1)
        ids = torch.from_numpy(_layer_ids(first, rows, DELTAS[l], limit, P, cap, reach)).to(dev())
        ks.append(k)
        idss.append(ids)
        units.append(nv.RebaseUnit(k.data_ptr(), cap * D * k.element_size(), first, rows, ids.data_ptr(), cap,
                                   first + rows, H, SLOTS[l]))
    k0 = [k.cpu() for k in ks]
    ids0 = [i.cpu() for i in idss]
    offsets = torch.tensor(OFFSETS0, dtype=torch.int64, device=dev())
    delta = torch.full((4,), -5, dtype=torch.int64, device=dev())
    _call(units, D, dtype, P, inv_d, sections, limit, offsets, delta)
    assert delta.tolist() == want, (first, rows)
    expect = list(OFFSETS0)
    for l in range(4):
        expect[SLOTS[l]] += want[l]
    assert offsets.tolist() == expect, (first, rows)
    worst = 0.0
    for l in range(4):
        ka = ks[l].cpu()
        assert torch.equal(_bits(ka[H]), _bits(k0[l][H])), (geometry, dtype_name, first, rows, H, l, "the head behind the last")
        w = _check_layer((geometry, dtype_name, first, rows, H, l), dtype_name, k0[l][:H], ka[:H], ids0[l], idss[l].cpu(),
                         first, rows, limit, inv, sections, want[l])
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("geometry,dtype_name", CASES, ids=[f"{g}-{d}" for g, d in CASES])
def test_four_layers_in_one_call(geometry, dtype_name):
    worst = 0.0
    for first in (0, 5):
        for rows in (1, 63, 257):
            worst = max(worst, _one_call(geometry, dtype_name, first, rows))
    print(f"rebase[{geometry} {dtype_name}]: worst error / bar {worst:.3f}")


HEAD_CASES = [("D128_plain", "bfloat16", 33), ("D32_mrope", "float32", 9)]


@pytest.mark.parametrize("heads", [4, 5, 9])
@pytest.mark.parametrize("geometry,dtype_name,rows", HEAD_CASES, ids=[f"{g}-{d}" for g, d, _ in HEAD_CASES])
def test_head_batches(geometry, dtype_name, rows, heads):
    """The rotation walks a row's heads in batches of 4: one full batch, a full batch and a ragged one of 1 (its loads are
    clamped to the last head, its stores stop there), two full batches and 1.  33 rows at D = 128: one workgroup step of 32
    and a ragged one.  The pass criteria are the file's, the guard head's bits among them."""
    worst = _one_call(geometry, dtype_name, 5, rows, heads)
    print(f"rebase[{geometry} {dtype_name} H={heads}]: worst error / bar {worst:.3f}")


def test_more_units_than_one_launch_takes():
    """70 layers (RTK_REBASE_MAX_UNITS = 64: two pairs of launches, the second pair reads its own deltas), every third one
    untriggered.  `rows` and `end` are independent: here the K rows stop 2 short of the ids, and the K rows beyond `rows`
    stay as they are."""
    import retake._native as nv

    assert nv.REBASE_MAX_UNITS == 64
    D, first, n_ids, rows, cap, n = 16, 2, 9, 7, 12, 70
    inv = synth.inv_freq(D)
    inv_d = torch.from_numpy(inv).to(dev())
    rng = np.random.default_rng(3)
    k = torch.from_numpy(rng.standard_normal((n, H, cap, D)).astype(np.float32)).to(torch.bfloat16).to(dev())
    ids = torch.arange(cap, dtype=torch.int64).repeat(n, 1, 1)           # [n, 1, cap]: dense - delta 0
    for l in range(n):
        if l % 3:
            ids[l, 0, first:] += 5 + l
    ids = ids.to(dev())
    k0, ids0 = k.cpu(), ids.cpu()
    units = [nv.RebaseUnit(k[l].data_ptr(), cap * D * 2, first, rows, ids[l].data_ptr(), cap, first + n_ids, H, l) for l in range(n)]
    offsets = torch.zeros(n, dtype=torch.int64, device=dev())
    delta = torch.full((n,), -1, dtype=torch.int64, device=dev())
    _call(units, D, torch.bfloat16, 1, inv_d, None, 0, offsets, delta)
    want = [5 + l if l % 3 else 0 for l in range(n)]
    assert delta.tolist() == want and offsets.tolist() == want
    ka, ia = k.cpu(), ids.cpu()
    for l in range(n):
        ref_ids, ref_k, d = rr.rebase(ids0[l].numpy(), k0[l].double().numpy(), first, first + n_ids, first + rows, 0, inv)
        assert d == want[l] and np.array_equal(ia[l].numpy(), ref_ids), l
        assert torch.equal(_bits(ka[l][:, first + rows:]), _bits(k0[l][:, first + rows:])), l
        assert torch.equal(_bits(ka[l][:, :first]), _bits(k0[l][:, :first])), l
        got, ref = ka[l].double().numpy()[:, first:first + rows], ref_k[:, first:first + rows]
        assert np.all(np.abs(got - ref) <= rr.bar("bfloat16", ref, k0[l].double().numpy()[:, first:first + rows])), l
        if not d:
            assert torch.equal(_bits(ka[l]), _bits(k0[l])), l


def test_an_empty_region_and_no_units_launch_nothing_harmful():
    import retake._native as nv

    D, cap = 128, 8
    k = torch.ones((H, cap, D), dtype=torch.bfloat16, device=dev())
    ids = (torch.arange(cap, dtype=torch.int64, device=dev()) * 10).view(1, cap).contiguous()
    k0, ids0 = k.clone(), ids.clone()
    inv_d = torch.from_numpy(synth.inv_freq(D)).to(dev())
    offsets = torch.zeros(1, dtype=torch.int64, device=dev())
    delta = torch.full((1,), -1, dtype=torch.int64, device=dev())
    _call([nv.RebaseUnit(k.data_ptr(), cap * D * 2, 5, 0, ids.data_ptr(), cap, 5, H, 0)], D, torch.bfloat16, 1, inv_d, None, 0,
          offsets, delta)
    assert delta.tolist() == [0] and offsets.tolist() == [0]
    assert torch.equal(k, k0) and torch.equal(ids, ids0)

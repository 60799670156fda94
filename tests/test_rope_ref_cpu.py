"""tests/rope_ref.py on its own, against float64 truth: the bounds tests/test_rope_gpu.py holds the kernels to are bounds the
host restatement itself keeps, in every dtype, head_dim, id layout and scaling - shown without a GPU."""
import numpy as np
import pytest
import torch

import rope_ref as rr
import synth

SECTIONS = {8: [1, 1, 2], 16: [2, 3, 3], 64: [8, 12, 12], 128: [16, 24, 24], 256: [32, 48, 48]}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _ids(seed, P, n):
    rng = np.random.default_rng(seed)
    rows = []
    for p in range(P):
        a = np.concatenate([rng.integers(0, 2501, n - n // 2), rng.integers(2500, 300001, n // 2)])
        rng.shuffle(a)
        rows.append(a)
    ids = np.stack(rows).astype(np.int64)
    ids[0, 0], ids[-1, -1] = 0, 300000
    return ids


@pytest.mark.parametrize("scaling", [1.0, synth.YARN_FACTOR4_ATTENTION_SCALING])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("D", [8, 16, 64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_forward_rotation_keeps_its_bound(dtype, D, P, scaling):
    n, H = 300, 2
    sec = SECTIONS[D] if P == 3 else None
    ids = _ids(D + P, P, n)
    inv = synth.inv_freq(D)
    x = torch.from_numpy(synth.qkv_chunk(11 + D, 1, H, n, D)[1][0]).to(dtype)
    cos, sin = rr.tables(ids, inv, D, scaling, rr.round_mode(dtype), sec)
    out = rr.rotate(x, cos, sin)
    assert out.dtype == dtype and out.shape == x.shape
    truth, mag = rr.rotate_truth(x, rr.angles(ids, inv, D, sec), scaling)
    frac = np.abs(out.double().numpy() - truth) / rr.rotate_bound(dtype, mag)
    print(f"rope_ref rotate[{str(dtype)[6:]} D{D} P{P} a={scaling:.4f}]: worst error {frac.max():.3f} of the bound")
    assert frac.max() <= 1.0


@pytest.mark.parametrize("delta", [0, 1, -5, 4097, 250000])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_shift_rounded_to_the_dtype_keeps_its_bound(dtype, delta):
    """The float64 shift rounded once to the tensor dtype lies inside the shift bound; untouched channels are the input."""
    D, n = 128, 50
    x = torch.from_numpy(synth.qkv_chunk(5, 1, 3, n, D)[1][0]).to(dtype)
    for P, sec in ((1, None), (3, SECTIONS[D])):
        want, mag = rr.shift(x, delta, synth.inv_freq(D), P, sec)
        got = torch.from_numpy(want).to(dtype).double().numpy()
        assert (np.abs(got - want) <= rr.shift_bound(dtype, mag)).all()
        off = np.concatenate([rr.rowsel(D, P, sec)[:D // 2] != 0] * 2)
        assert np.array_equal(want[..., off], x.double().numpy()[..., off]) and off.sum() == (96 if P == 3 else 0)
        if delta == 0:
            assert np.array_equal(want, x.double().numpy())
    # R(a) R(b) = R(a + b) at small angles: the composition the chunk-sharded prefill once relied on
    a, _ = rr.shift(x, 3, synth.inv_freq(D))
    b, _ = rr.shift(torch.from_numpy(a), 4, synth.inv_freq(D))
    c, _ = rr.shift(x, 7, synth.inv_freq(D))
    assert np.abs(b - c).max() <= 1e-5 * np.abs(c).max()


def test_row_selection_tables_and_reforged_ids():
    assert rr.rowsel(128, 3, [16, 24, 24]).tolist() == ([0] * 16 + [1] * 24 + [2] * 24) * 2
    assert rr.rowsel(16, 1).tolist() == [0] * 16
    # tables: the bf16 / fp16 ones are the fp32 ones rounded once; id 0 gives cos = scaling, sin = 0
    ids = _ids(1, 3, 64)
    inv = synth.inv_freq(128)
    a = synth.YARN_FACTOR4_ATTENTION_SCALING
    c0, s0 = rr.tables(ids, inv, 128, a, 0, [16, 24, 24])
    for mode, dt in ((1, torch.bfloat16), (2, torch.float16)):
        c, s = rr.tables(ids, inv, 128, a, mode, [16, 24, 24])
        assert np.array_equal(c, torch.from_numpy(c0).to(dt).float().numpy())
        assert np.array_equal(s, torch.from_numpy(s0).to(dt).float().numpy())
    assert c0[0, 0] == np.float32(a) and s0[0, 0] == 0.0 and c0[0, 64] == np.float32(a)
    assert c0[0, 16] == np.float32(np.float32(np.cos(np.float64(np.float32(ids[1, 0]) * inv[16]))) * np.float32(a))
    # reforged ids: 640 consecutive ids from 19, every 10th-ish kept, ratio 63 / 640 truncates
    kept = torch.arange(19, 19 + 640)[torch.arange(63) * 10 + 3]
    got = rr.reforge_ids(kept, 63, 640)
    want = [22 + int(np.float32(10 * i) * np.float32(63 / 640)) for i in range(63)]
    assert got.tolist() == want and got.dtype == torch.int64

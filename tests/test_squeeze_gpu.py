"""rtk_pivotkv_squeeze_batched alone, straight through the C ABI: rows of several byte streams gathered down in place,
row[first + r] = row[first + idx[r]], against torch.index_select from a snapshot, bit for bit.  Every buffer is a flat byte
tensor [streams, rows, row_bytes] of random bytes whose stream stride reaches beyond the moved rows, and it is compared
WHOLE: a byte written before `first`, past `rows_out` or between the streams shows up.

The kernel moves 1024 vectors per workgroup and step over a 128-byte column slice: R = 128 rows a step for rows of 256 and
128 bytes (16-byte accesses), 512 for 8-byte rows and 1024 for 4-byte rows (4-byte accesses).  rows_out lies on both sides
of R, at several steps plus a remainder, and at 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP = {256: 128, 128: 128, 8: 512, 4: 1024}     # R of the kernel per row size
FIRST, GUARD = 5, 9                               # an odd first row; untouched rows behind the region
KINDS = ("identity", "drop_row0", "drop_leading", "every_other", "random", "last_only")


def dev():
    return torch.device("cuda:0")


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _buffer(streams, rows, row_bytes, seed):
    return torch.randint(0, 256, (streams, rows, row_bytes), dtype=torch.uint8, generator=_gen(seed)).to(dev())


def _index_list(kind, m, seed):
    """(idx [rows_out] int64 on the CPU, rows_in) of a list with about m destination rows."""
    if kind == "identity":
        return torch.arange(m), m + 3
    if kind == "drop_row0":                          # a shift by one: maximal overlap
        return torch.arange(1, m + 1), m + 1
    if kind == "drop_leading":                       # a constant shift: what rtk_pivotkv_slide_batched does
        return torch.arange(37, m + 37), m + 37
    if kind == "every_other":
        return torch.arange(m) * 2 + 1, 2 * m
    if kind == "random":                             # 1.5 % of the rows dropped, anywhere
        n = m + max(1, (m * 15 + 999) // 1000)
        keep = torch.randperm(n, generator=_gen(seed))[:m].sort().values
        return keep, n
    assert kind == "last_only"
    return torch.tensor([m - 1] if m else [], dtype=torch.int64), m


def _unit(t, first, idx_dev, rows_out, rows_in, byte_offset=0):
    import retake._native as nv

    streams, rows, row_bytes = t.shape
    return nv.SqueezeUnit(t.data_ptr() + byte_offset, rows * row_bytes, streams, row_bytes, first, rows_out, rows_in,
                          idx_dev.data_ptr() if idx_dev.numel() else None)


def _expected(t, first, idx, rows_out):
    want = t.clone()
    if rows_out:
        want[:, first:first + rows_out] = t.index_select(1, first + idx.to(t.device))
    return want


def _launch(units):
    import retake._native as nv

    arr = (nv.SqueezeUnit * max(1, len(units)))(*units)
    rc = nv.lib.rtk_pivotkv_squeeze_batched(arr, len(units), nv.stream())
    torch.cuda.synchronize()
    return rc


def _ok(rc):
    import retake._native as nv

    nv.check(rc, "rtk_pivotkv_squeeze_batched")


def _launches(fn, name="squeeze_units"):
    import retake._native as nv

    kid = nv.profile_kernel_ids()[name]
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable_mask(1 << kid)
    try:
        fn()
        return nv.profile_read().get(name, (0, 0.0))[0]
    finally:
        nv.lib.rtk_profile_enable(0)
        nv.lib.rtk_profile_reset()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row_bytes", [256, 128, 8, 4])
def test_one_unit(row_bytes, kind):
    """Streams 1, 3, 4 x rows_out around the kernel's step, each its own launch on its own buffer."""
    R = STEP[row_bytes]
    for streams in (1, 3, 4):
        for m in (0, R - 1, R, R + 1, 3 * R + 17):
            idx, rows_in = _index_list(kind, m, 1000 * row_bytes + m)
            rows_out = idx.numel()
            t = _buffer(streams, FIRST + rows_in + GUARD, row_bytes, 7 * row_bytes + streams + m)
            want = _expected(t, FIRST, idx, rows_out)
            idx_dev = idx.to(torch.int32).to(dev())
            n = _launches(lambda: _ok(_launch([_unit(t, FIRST, idx_dev, rows_out, rows_in)])))
            assert torch.equal(t, want), (row_bytes, kind, streams, m)
            assert n == (1 if rows_out else 0)       # a unit that moves nothing launches nothing


@pytest.mark.parametrize("row_bytes", [256, 8])
def test_a_leading_block_equals_the_slide(row_bytes):
    """Dropping a leading block is a constant shift: the same bytes as rtk_pivotkv_slide_batched leaves on a copy."""
    import retake._native as nv

    m, d = 3 * STEP[row_bytes] + 17, 37
    t = _buffer(3, FIRST + m + d + GUARD, row_bytes, 11)
    twin = t.clone()
    idx_dev = torch.arange(d, m + d, dtype=torch.int32, device=dev())
    _ok(_launch([_unit(t, FIRST, idx_dev, m, m + d)]))
    su = nv.SlideUnit(twin.data_ptr(), twin.shape[1] * row_bytes, 3, row_bytes, FIRST, d, m)
    nv.check(nv.lib.rtk_pivotkv_slide_batched(C_byref(su), 1, nv.stream()), "rtk_pivotkv_slide_batched")
    torch.cuda.synchronize()
    assert torch.equal(t, twin)


def C_byref(x):
    import ctypes

    return ctypes.byref(x)


def test_many_steps_per_stream():
    """6000 rows of 256 bytes in 2 streams (3 MB), 1.5 % dropped at random: 47 steps per workgroup, two slices per stream."""
    idx, rows_in = _index_list("random", 6000, 5)
    t = _buffer(2, 13 + rows_in + GUARD, 256, 6)
    want = _expected(t, 13, idx, idx.numel())
    _ok(_launch([_unit(t, 13, idx.to(torch.int32).to(dev()), idx.numel(), rows_in)]))
    assert torch.equal(t, want)


@pytest.mark.parametrize("row_bytes", [128, 256])
def test_base_offset_by_four_bytes(row_bytes):
    """A unit whose base lies 4 bytes into the buffer: rows of 128 / 256 bytes on the 4-byte path."""
    idx, rows_in = _index_list("random", 700, 8)
    t = _buffer(2, FIRST + rows_in + GUARD, row_bytes, 9)
    flat = t.clone().view(2, -1)
    want = flat.clone()
    lo = 4 + FIRST * row_bytes
    src = flat[:, 4 + FIRST * row_bytes:4 + (FIRST + rows_in) * row_bytes].reshape(2, rows_in, row_bytes)
    want[:, lo:lo + idx.numel() * row_bytes] = src.index_select(1, idx.to(dev())).reshape(2, -1)
    _ok(_launch([_unit(t, FIRST, idx.to(torch.int32).to(dev()), idx.numel(), rows_in, byte_offset=4)]))
    assert torch.equal(t.view(2, -1), want)


def test_one_launch_with_mixed_units():
    """3 layers x (K, V of 256-byte rows, ids of 8, scores of 4), each layer with its own list: one launch."""
    bufs, units, wants, keep = [], [], [], []
    for l, kind in enumerate(("random", "identity", "every_other")):
        idx, rows_in = _index_list(kind, 600, 20 + l)
        idx_dev = idx.to(torch.int32).to(dev())
        keep.append(idx_dev)
        for streams, row_bytes in ((2, 256), (2, 256), (3, 8), (1, 4)):
            t = _buffer(streams, FIRST + rows_in + GUARD, row_bytes, 100 * l + len(bufs))
            bufs.append(t)
            wants.append(_expected(t, FIRST, idx, idx.numel()))
            units.append(_unit(t, FIRST, idx_dev, idx.numel(), rows_in))
    assert _launches(lambda: _ok(_launch(units))) == 1
    for i, (t, w) in enumerate(zip(bufs, wants)):
        assert torch.equal(t, w), i
    assert _launch([]) == 0                          # n_units == 0: success


def test_more_units_than_one_launch_holds():
    """100 moving units in one call: two kernel launches; a bad unit at the very end stops the call before the first."""
    import retake._native as nv

    idx, rows_in = _index_list("random", 70, 3)
    idx_dev = idx.to(torch.int32).to(dev())
    big = _buffer(100, 3 + rows_in + GUARD, 64, 4)
    before = big.clone()
    units = [_unit(big[i:i + 1], 3, idx_dev, idx.numel(), rows_in) for i in range(100)]
    bad = _unit(big[:1], 3, idx_dev, idx.numel(), rows_in)
    bad.row_bytes = 6
    assert _launches(lambda: _expect(_launch(units + [bad]), nv.RTK_EINVAL)) == 0
    assert nv.lib.rtk_last_error().startswith(b"rtk_pivotkv_squeeze_batched")
    assert torch.equal(big, before)
    assert _launches(lambda: _ok(_launch(units))) == -(-100 // nv.SQUEEZE_MAX_UNITS) == 2
    assert torch.equal(big, _expected(before, 3, idx, idx.numel()))


def _expect(rc, code):
    assert rc == code, rc


@pytest.mark.parametrize("row_bytes", [256, 4])
def test_a_bad_list_is_clamped(row_bytes):
    """The kernel clamps idx[r] into [r, rows_in - 1]: a list that descends, repeats, or names rows just outside the region
    moves exactly the clamped rows and writes nothing outside [first, first + rows_out).  (The entries stay within 3 rows of
    the region and the buffer has 9 guard rows on either side: nothing here can leave the allocation.)"""
    rows_in, first = 2 * STEP[row_bytes] + 50, GUARD
    m = rows_in - 20
    idx = torch.randint(-3, rows_in + 3, (m,), generator=_gen(12))
    clamped = torch.minimum(torch.maximum(idx, torch.arange(m)), torch.tensor(rows_in - 1))
    t = _buffer(2, first + rows_in + GUARD, row_bytes, 13)
    want = _expected(t, first, clamped, m)
    _ok(_launch([_unit(t, first, idx.to(torch.int32).to(dev()), m, rows_in)]))
    assert torch.equal(t, want)

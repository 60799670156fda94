"""rtk_pivotkv_slide_batched alone, straight through the C ABI: rows of several byte streams moved down in place in one
launch, against torch's `dst.copy_(src.clone())` on a twin tensor.  Every buffer is filled with values derived from
`arange` (distinct bit patterns row by row, so a misplaced row cannot pass for a correct one) and compared WHOLE, bit
for bit, so that a write outside the destination range shows up.  The kernel moves 16 KB (16-byte accesses) or 4 KB
(4-byte accesses) per workgroup and step: the cases lie on both sides of that, and of "one workgroup per stream"."""

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(5, 1, 690),      # maximal overlap
         (0, 3, 600),
         (5, 64, 600),     # bf16 rows of 256 bytes: the drop is exactly one 16 KB tile
         (7, 300, 300),    # ranges just disjoint
         (5, 400, 200),    # disjoint with a gap
         (5, 0, 600),      # no-ops
         (5, 10, 0),
         (3, 1, 1)]
SHAPES = {"bf16": ((1, 2, 700, 128), torch.bfloat16), "fp32": ((1, 2, 700, 64), torch.float32),
          "codes": ((1, 2, 700, 128), torch.uint8), "scales": ((1, 2, 700), torch.float32), "ids": ((3, 700), torch.int64)}


def dev():
    return torch.device("cuda:0")


def _filled(shape, dtype, salt=0):
    """A tensor whose element i holds a bit pattern mixed from arange: i + salt through two multiply / xor-shift rounds
    (int64 arithmetic wraps), cut to the element's width - rows differ from each other at any distance."""
    n = 1
    for s in shape:
        n *= s
    x = torch.arange(n, dtype=torch.int64, device=dev()) + (salt + 1)
    for mul in (0x2545F4914F6CDD1D, 0x1B873593CC9E2D51):
        x = x * mul
        x = x ^ (x >> 29)
    if dtype == torch.int64:
        return x.view(shape)
    if dtype == torch.uint8:
        return (x & 0xFF).to(torch.uint8).view(shape)
    if dtype == torch.float32:
        return (x & 0x7FFFFFFF).to(torch.int32).view(torch.float32).view(shape)
    return ((x & 0xFFFF) - 0x8000).to(torch.int16).view(dtype).view(shape)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _rows_dim(t):
    return {4: 2, 3: 2, 2: 1}[t.ndim]


def _unit(t, first, drop, rows, byte_offset=0):
    """The rtk_slide_unit of a contiguous [1, H, R, D] / [1, H, R] / [P, R] tensor: one stream per head / id plane."""
    import retake._native as nv

    rd = _rows_dim(t)
    row_bytes = t.element_size() * (t.shape[3] if t.ndim == 4 else 1)
    return nv.SlideUnit(t.data_ptr() + byte_offset, t.shape[rd] * row_bytes, t.shape[rd - 1], row_bytes, first, drop, rows)


def _expected(t, first, drop, rows):
    out = t.clone()
    if drop and rows:
        rd = _rows_dim(t)
        out.narrow(rd, first, rows).copy_(out.narrow(rd, first + drop, rows).clone())
    return out


def _launch(units):
    import retake._native as nv

    arr = (nv.SlideUnit * max(1, len(units)))(*units)
    rc = nv.lib.rtk_pivotkv_slide_batched(arr, len(units), nv.stream())
    torch.cuda.synchronize()
    return rc


def _launches(fn):
    """How many slide launches fn() makes (rtk_profile_read of the kernel's id)."""
    import retake._native as nv

    kid = nv.profile_kernel_ids()["slide_units"]
    nv.lib.rtk_profile_reset()
    nv.lib.rtk_profile_enable_mask(1 << kid)
    try:
        fn()
        return nv.profile_read().get("slide_units", (0, 0.0))[0]
    finally:
        nv.lib.rtk_profile_enable(0)
        nv.lib.rtk_profile_reset()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "f%d_d%d_r%d" % c)
@pytest.mark.parametrize("kind", list(SHAPES))
def test_one_unit(kind, case):
    shape, dtype = SHAPES[kind]
    t = _filled(shape, dtype)
    want = _expected(t, *case)
    n = _launches(lambda: _check_ok(_launch([_unit(t, *case)])))
    assert torch.equal(_bits(t), _bits(want)), (kind, case)
    assert n == (1 if case[1] and case[2] else 0)       # a no-op unit launches nothing


def _check_ok(rc):
    import retake._native as nv

    nv.check(rc, "rtk_pivotkv_slide_batched")


def test_many_tiles_and_slices_per_stream():
    """40 000 rows of 256 bytes per stream, moved by 1568 rows: 25 workgroups per stream, 25 steps each."""
    t = _filled((1, 4, 40000, 128), torch.bfloat16)
    want = _expected(t, 13, 1568, 38000)
    _check_ok(_launch([_unit(t, 13, 1568, 38000)]))
    assert torch.equal(_bits(t), _bits(want))
    # and one workgroup per stream walking many tiles (a drop below a tile)
    t = _filled((1, 4, 40000, 128), torch.bfloat16, salt=3)
    want = _expected(t, 13, 7, 39000)
    _check_ok(_launch([_unit(t, 13, 7, 39000)]))
    assert torch.equal(_bits(t), _bits(want))


def test_one_launch_with_mixed_units():
    """3 layers x (K, V, ids), the drop differing per layer, one of them 0: one launch, every buffer right."""
    drops = (7, 0, 64)
    bufs, units, wants = [], [], []
    for l, d in enumerate(drops):
        for shape, dtype in (((1, 2, 700, 128), torch.bfloat16), ((1, 2, 700, 128), torch.bfloat16), ((3, 700), torch.int64)):
            t = _filled(shape, dtype, salt=1000 * l + len(bufs))
            bufs.append(t)
            wants.append(_expected(t, 5, d, 600))
            units.append(_unit(t, 5, d, 600))
    assert _launches(lambda: _check_ok(_launch(units))) == 1
    for i, (t, w) in enumerate(zip(bufs, wants)):
        assert torch.equal(_bits(t), _bits(w)), i
    assert _launch([]) == 0                                  # n_units == 0: success


def test_more_units_than_one_launch_holds():
    """100 moving units in one call: two kernel launches (96 units travel per launch), every buffer right; and a bad unit at
    the very end still stops the call before the first launch."""
    import retake._native as nv

    big = _filled((100, 2, 90, 16), torch.float32)
    bufs = [big[i:i + 1] for i in range(100)]
    wants = [_expected(t, 3, 1 + i % 5, 80) for i, t in enumerate(bufs)]
    units = [_unit(t, 3, 1 + i % 5, 80) for i, t in enumerate(bufs)]
    before = big.clone()
    bad = _unit(bufs[0], 3, 1, 80)
    bad.row_bytes = 6
    assert _launches(lambda: _expect(_launch(units + [bad]), nv.RTK_EINVAL, "bad last unit")) == 0
    assert torch.equal(_bits(big), _bits(before))
    assert _launches(lambda: _check_ok(_launch(units))) == -(-100 // nv.SLIDE_MAX_UNITS) == 2
    for i, (t, w) in enumerate(zip(bufs, wants)):
        assert torch.equal(_bits(t), _bits(w)), i


@pytest.mark.parametrize("kind,drop", [("scales", 3), ("scales", 1100), ("codes", 3), ("codes", 40)])
def test_base_offset_by_four_bytes(kind, drop):
    """A unit whose base is 4 bytes into the buffer (scales that start at an odd row; codes at byte 4): the 4-byte path,
    narrow and wide drops.  The twin is the same move on the flat buffer."""
    shape, dtype = ((1, 2, 1400), torch.float32) if kind == "scales" else ((1, 2, 700, 128), torch.uint8)
    t = _filled(shape, dtype)
    H, per_head = 2, t.numel() // 2
    row = t.element_size() * (128 if kind == "codes" else 1)
    rows = per_head * t.element_size() // row - drop - 2
    flat = t.clone().view(H, -1).view(torch.uint8)            # [H, bytes per head]
    want = flat.clone()
    a = 4 + row
    want[:, a:a + rows * row] = flat[:, a + drop * row:a + (drop + rows) * row]
    u = _unit(t, 1, drop, rows, byte_offset=4)
    _check_ok(_launch([u]))
    assert torch.equal(t.view(H, -1).view(torch.uint8), want)


def test_errors_come_before_any_launch():
    import retake._native as nv

    k = _filled((1, 2, 700, 128), torch.bfloat16)
    ids = _filled((3, 700), torch.int64)
    k0, ids0 = k.clone(), ids.clone()
    good = lambda: _unit(k, 5, 7, 600)   # noqa: E731

    def bad(**kw):
        u = _unit(ids, 5, 7, 600)
        for name, value in kw.items():
            setattr(u, name, value)
        return u

    cases = {"NULL base": bad(base=None), "negative first": bad(first=-1), "negative drop": bad(drop=-1),
             "negative rows": bad(rows=-1), "no streams": bad(streams=0), "row_bytes 6": bad(row_bytes=6),
             "row_bytes 0": bad(row_bytes=0), "base + 2": bad(base=ids.data_ptr() + 2),
             "stride + 2": bad(stream_stride=700 * 8 + 2)}
    for what, u in cases.items():
        n = _launches(lambda: _expect(_launch([good(), u]), nv.RTK_EINVAL, what))   # the valid unit in front moves nothing either
        assert n == 0, what
        assert torch.equal(_bits(k), _bits(k0)) and torch.equal(ids, ids0), what
        assert nv.lib.rtk_last_error().startswith(b"rtk_pivotkv_slide_batched"), what
    assert nv.lib.rtk_pivotkv_slide_batched(None, 1, nv.stream()) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_slide_batched(None, -1, nv.stream()) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_slide_batched(None, 0, nv.stream()) == 0


def _expect(rc, code, what):
    assert rc == code, (what, rc)

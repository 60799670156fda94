"""rtk_pivotkv_focus_gather_batched alone, straight through the C ABI: rows of several byte streams gathered OUT OF PLACE,
destination = [src rows [0, head) | src rows first + clamp(idx) | src rows [tail_src, tail_src + tail)], against torch.cat /
index_select from a snapshot, bit for bit.

Every destination is a flat byte tensor [streams, GUARD + rows + GUARD, row_bytes] of sentinel bytes whose unit begins at row
GUARD, compared WHOLE: a byte written in front of a stream, behind its last row or between the streams shows up.  Every
source holds PAD sentinel rows on both sides of the region (the `head` rows in front of it are followed by PAD rows, the
tail lies PAD rows behind it): an index that was not clamped would read a sentinel row - a wrong byte in the comparison -,
never unmapped memory.  The kernel gives a workgroup 64 destination rows, a wave 16, 8 in flight per thread: the row counts
lie on both sides of 8, 16 and 64."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 700                   # region rows
GUARD, PAD = 3, 9         # destination guard rows; source sentinel rows around the region
DST_FILL, SRC_FILL = 0xA5, 0x5A
HEADS, TAILS, KEEPS = (0, 5), (0, 13), (1, 37, 512, N)


def dev():
    return torch.device("cuda:0")


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


class _Case:
    """One unit: source [streams, src_rows, row_bytes] laid out [head | PAD sentinels | region n | PAD sentinels | tail | PAD]
    with stream stride src_rows * row_bytes, destination [streams, GUARD + total + GUARD + extra, row_bytes] - unequal
    strides on the two sides.  offset: both bases lie `offset` bytes into their allocations (4: the 4-byte path)."""

    def __init__(self, streams, row_bytes, head, keep, tail, idx, seed, n=N, offset=0, extra=2):
        self.streams, self.row_bytes, self.head, self.keep, self.tail, self.n, self.offset = streams, row_bytes, head, keep, tail, n, offset
        self.first, self.tail_src = head + PAD, head + PAD + n + PAD
        src_rows = self.tail_src + tail + PAD
        src = torch.randint(0, 256, (streams, src_rows, row_bytes), dtype=torch.uint8, generator=_gen(seed))
        src[:, head:self.first] = SRC_FILL
        src[:, self.first + n:self.tail_src] = SRC_FILL
        src[:, self.tail_src + tail:] = SRC_FILL
        self.total = head + keep + tail
        self.dst_rows = GUARD + self.total + GUARD + extra
        # both units begin 16 + offset bytes into their allocations (which are 256-byte aligned)
        self.src_at = self.dst_at = 16 + offset
        self.src_raw = torch.cat([torch.full((self.src_at,), SRC_FILL, dtype=torch.uint8), src.flatten()]).to(dev())
        self.dst_raw = torch.full((self.dst_at + streams * self.dst_rows * row_bytes,), DST_FILL, dtype=torch.uint8, device=dev())
        self.src = src.to(dev())
        self.src_rows = src_rows
        self.idx = idx.to(torch.int32).to(dev()) if idx is not None else None
        self.idx_cpu = idx

    def unit(self):
        import retake._native as nv

        rb = self.row_bytes
        return nv.FocusUnit(self.src_raw.data_ptr() + self.src_at, self.dst_raw.data_ptr() + self.dst_at + GUARD * rb,
                            self.src_rows * rb, self.dst_rows * rb, self.streams, rb, self.head, self.first, self.n, self.keep,
                            self.tail_src, self.tail, self.idx.data_ptr() if self.keep else None)

    def dst(self):
        n = self.streams * self.dst_rows * self.row_bytes
        return self.dst_raw[self.dst_at:self.dst_at + n].view(self.streams, self.dst_rows, self.row_bytes)

    def want(self):
        w = torch.full((self.streams, self.dst_rows, self.row_bytes), DST_FILL, dtype=torch.uint8, device=dev())
        parts = [self.src[:, :self.head]]
        if self.keep:
            clamped = self.idx_cpu.clamp(0, self.n - 1).to(dev())
            parts.append(self.src.index_select(1, self.first + clamped))
        parts.append(self.src[:, self.tail_src:self.tail_src + self.tail])
        w[:, GUARD:GUARD + self.total] = torch.cat(parts, dim=1)
        return w

    def check(self, what):
        got, want = self.dst(), self.want()
        assert torch.equal(got, want), (what, "first differing row", int((got != want).any(dim=2).any(dim=0).nonzero()[0]))
        assert bool((self.dst_raw[:self.dst_at] == DST_FILL).all()), (what, "bytes in front of the destination")

    def untouched(self):
        return bool((self.dst_raw == DST_FILL).all())


def _launch(cases, expect=0):
    import retake._native as nv

    units = [c.unit() if isinstance(c, _Case) else c for c in cases]
    arr = (nv.FocusUnit * max(1, len(units)))(*units)
    rc = nv.lib.rtk_pivotkv_focus_gather_batched(arr, len(units), nv.stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, nv.lib.rtk_last_error())
    return rc


def _list(kind, keep, seed, n=N):
    if kind == "isolated":      # rows scattered over the region
        return torch.randperm(n, generator=_gen(seed))[:keep].sort().values
    if kind == "runs":          # long runs: a block at either end and one in the middle
        a = keep // 3
        b = keep - 2 * a
        return torch.cat([torch.arange(a), torch.arange(n // 2 - b // 2, n // 2 - b // 2 + b), torch.arange(n - a, n)])
    assert kind == "last"
    return torch.tensor([n - 1])


# (streams, row_bytes): D 128 bf16, D 64, fp32 rows, the 4-byte path, ids x 1 and x 3
SHAPES = [(4, 256), (1, 256), (4, 128), (4, 512), (1, 12), (4, 12), (1, 8), (3, 8)]


@pytest.mark.parametrize("streams,row_bytes", SHAPES)
def test_one_unit(streams, row_bytes):
    """head x tail x keep x list kind, each its own launch on its own buffers."""
    seed = 0
    for head in HEADS:
        for tail in TAILS:
            for keep in KEEPS:
                kinds = ("last",) if keep == 1 else (("identity",) if keep == N else ("isolated", "runs"))
                for kind in kinds:
                    seed += 1
                    idx = torch.arange(N) if kind == "identity" else _list(kind, keep, seed)
                    c = _Case(streams, row_bytes, head, keep, tail, idx, 100 * row_bytes + seed)
                    _launch([c])
                    c.check((streams, row_bytes, head, tail, keep, kind))


@pytest.mark.parametrize("row_bytes", [256, 128, 8])
def test_base_offset_by_four_bytes(row_bytes):
    """Bases 4 bytes behind a 16-byte boundary: rows of 256 / 128 / 8 bytes on the 4-byte path, the same bytes."""
    c = _Case(2, row_bytes, 5, 37, 13, _list("isolated", 37, 3), 7, offset=4)
    assert (c.src_raw.data_ptr() + c.src_at) % 16 == 4 and (c.dst_raw.data_ptr() + c.dst_at) % 16 == 4
    _launch([c])
    c.check(("offset 4", row_bytes))


@pytest.mark.parametrize("row_bytes", [256, 12])
def test_a_bad_list_is_clamped(row_bytes):
    """A list holding -5 and n + 7 gives what the clamped list gives: rows 0 and n - 1 of the region, no sentinel row."""
    idx = _list("isolated", 37, 5)
    idx[3], idx[20] = -5, N + 7
    c = _Case(4, row_bytes, 5, 37, 13, idx, 11)
    _launch([c])
    c.check(("clamped", row_bytes))
    got = c.dst()
    assert torch.equal(got[:, GUARD + 5 + 3], c.src[:, c.first]) and torch.equal(got[:, GUARD + 5 + 20], c.src[:, c.first + N - 1])


def _batch(seed):
    return [_Case(4, 256, 5, 512, 13, _list("isolated", 512, seed), seed),
            _Case(3, 8, 5, 512, 13, _list("isolated", 512, seed), seed + 1),
            _Case(2, 12, 0, 37, 0, _list("runs", 37, seed + 2), seed + 2)]


def test_units_of_different_shapes_in_one_call():
    """Three units of different shapes in one call; each alone gives the same bytes; a zero-row unit between them."""
    together = _batch(40)
    empty = _Case(2, 256, 0, 0, 0, None, 50)
    _launch(together[:1] + [empty] + together[1:])
    assert empty.untouched()
    for i, c in enumerate(together):
        c.check(("batched", i))
    for i, c in enumerate(_batch(40)):
        _launch([c])
        c.check(("alone", i))
        assert torch.equal(c.dst_raw, together[i].dst_raw), ("alone == batched", i)
    assert _launch([]) == 0                       # n_units == 0: success
    assert _launch([empty]) == 0 and empty.untouched()


def test_more_units_than_one_launch_holds():
    import retake._native as nv

    n = nv.FOCUS_MAX_UNITS + 1
    idx = _list("isolated", 37, 9)
    cases = [_Case(1 + i % 2, (256, 8, 12)[i % 3], i % 3, 37, i % 5, idx, 60 + i, extra=i % 4) for i in range(n)]
    _launch(cases)
    for i, c in enumerate(cases):
        c.check(("many units", i))


def test_every_refusal_leaves_the_destination_unwritten():
    import retake._native as nv

    idx = _list("isolated", 37, 2)
    good = _Case(2, 256, 5, 37, 13, idx, 70)
    bad = _Case(2, 256, 5, 37, 13, idx, 71)

    def refused(word=None, **change):
        u = bad.unit()
        for k, v in change.items():
            setattr(u, k, v)
        _launch([good, u], nv.RTK_EINVAL)         # a bad unit behind a good one stops the call before the first launch
        msg = nv.lib.rtk_last_error()
        assert msg.startswith(b"rtk_pivotkv_focus_gather_batched"), msg
        assert word is None or word in msg, (word, msg)
        assert good.untouched() and bad.untouched(), change

    u0 = bad.unit()
    refused(b"NULL", src=None)
    refused(b"NULL", dst=None)
    refused(b"NULL idx", idx=None)
    for name in ("head", "first", "n", "keep", "tail_src", "tail"):
        refused(b"negative", **{name: -1})
    refused(b"exceeds", keep=N + 1)
    refused(b"streams", streams=0)
    refused(b"row_bytes", row_bytes=0)
    refused(b"row_bytes", row_bytes=6)
    refused(b"aligned", src=u0.src + 2)
    refused(b"aligned", dst=u0.dst + 2)
    refused(b"aligned", src_stride=u0.src_stride + 2)
    refused(b"aligned", dst_stride=u0.dst_stride + 2)
    refused(b"negative", src_stride=-u0.src_stride)
    refused(b"dst_stride", dst_stride=256)
    refused(b"int32", n=1 << 40)
    # source and destination ranges that overlap: the destination inside the source, and the source's last row in the destination
    refused(b"overlap", dst=u0.src + 256)
    refused(b"overlap", src=u0.dst - (bad.tail_src + bad.tail - 1) * 256, src_stride=0)
    arr = (nv.FocusUnit * 1)(good.unit())
    assert nv.lib.rtk_pivotkv_focus_gather_batched(arr, -1, nv.stream()) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_focus_gather_batched(None, 1, nv.stream()) == nv.RTK_EINVAL
    assert good.untouched()
    _launch([good])
    good.check("the good unit afterwards")


def test_abi():
    import retake._native as nv

    assert "rtk_pivotkv_focus_gather_batched" in nv.EXPORTS and nv.lib.rtk_version() == nv.ABI_VERSION
    assert C.sizeof(nv.FocusUnit) == 96 and nv.FOCUS_MAX_UNITS == 48

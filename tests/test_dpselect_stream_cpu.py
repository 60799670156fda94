"""DPSelect on a stream (retake/dpselect_stream.py), the parts that need no GPU: what the constructor, from_config and the
two C entry points refuse - every refusal comes before any launch - and the host-side plan of pieces and emissions, checked
against a brute-force walk frame by frame."""
import ctypes
import types

import numpy as np
import pytest
import torch


def _stream(*a, **kw):
    from retake.dpselect_stream import DPSelectStream

    return DPSelectStream(*a, **kw)


@pytest.mark.parametrize("args, kw", [
    ((1,), dict(ratio=0.5, window_size=1)),          # S < 2
    ((4,), dict(ratio=0.5, window_size=5)),          # S < w
    ((8,), dict(ratio=0.5, window_size=0)),          # w < 1
    ((8,), dict()),                                  # neither ratio nor keep
    ((8,), dict(ratio=0.5, keep=2)),                 # both
    ((8,), dict(ratio=0.0)),
    ((8,), dict(ratio=1.5)),
    ((8,), dict(ratio=-0.25)),
    ((8,), dict(keep=0)),
    ((8,), dict(keep=9)),
])
def test_constructor_refusals(args, kw):
    with pytest.raises(ValueError, match="DPSelectStream"):
        _stream(*args, **kw)


def test_constructor_accepts_the_edges():
    import retake.visual_compression as vc
    from retake.dpselect_stream import DPSelectStream

    assert vc.DPSelectStream is DPSelectStream and "DPSelectStream" in vc.__all__
    s = _stream(2, ratio=1.0, window_size=2)
    assert (s.segment_frames, s.window_size, s.sync, s.frames_seen, s.segments_emitted) == (2, 2, True, 0, 0)
    assert s.memory_footprint() == 0                 # nothing is allocated before the first push
    assert _stream(5, keep=5, window_size=5, sync=False).keep == 5
    assert s.finish() == []                          # an empty stream emits nothing ...
    with pytest.raises(RuntimeError, match="finish"):
        s.push(torch.zeros(1, 4, 8))                 # ... and is closed all the same
    s.reset()
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # open again; a push needs a device
        s.push(torch.zeros(1, 4, 8))


def test_push_refusals_before_any_launch():
    s = _stream(8, ratio=0.5)
    for bad in (torch.zeros(4, 8), torch.zeros(2, 3, 4, 8), torch.zeros(1, 1, 3, 4, 8)):
        with pytest.raises(ValueError, match="frames must be"):
            s.push(bad)
    with pytest.raises(IndexError):                  # the reference's failure, same class
        _stream(8, ratio=0.5, sync=False).push(torch.zeros(3, 1, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.push(torch.zeros(3, 4, 8))
    assert s.frames_seen == 0 and s.memory_footprint() == 0


def test_from_config():
    from retake.dpselect_stream import DPSelectStream

    def cfg(**ck):
        return types.SimpleNamespace(longvideo_kwargs={"visual_compression_kwargs": ck})

    s = DPSelectStream.from_config(cfg(compression_ratio=0.25, compression_method="Keyframe", patch_sync=False), 16)
    assert (s.segment_frames, s.ratio, s.keep, s.sync, s.window_size) == (16, 0.25, None, False, 3)
    assert DPSelectStream.from_config(cfg(compression_ratio=1.0, compression_method="Keyframe", patch_sync=True), 4).sync
    for bad in (cfg(compression_ratio=0.5, compression_method="MALLM", patch_sync=True), cfg(compression_ratio=0.5),
                types.SimpleNamespace(), types.SimpleNamespace(longvideo_kwargs={})):
        with pytest.raises(ValueError, match="Keyframe"):
            DPSelectStream.from_config(bad, 16)
    with pytest.raises(ValueError):                  # the constructor's own checks still apply
        DPSelectStream.from_config(cfg(compression_ratio=2.0, compression_method="Keyframe"), 16)
    with pytest.raises(ValueError):
        DPSelectStream.from_config(cfg(compression_method="Keyframe"), 16)   # no ratio


def _refused(rc, code, *words):
    import retake._native as nv

    msg = nv.lib.rtk_last_error()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_ingest_refuses_bad_arguments_before_any_launch():
    import retake._native as nv

    lib, E, name = nv.lib, nv.RTK_EINVAL, b"rtk_dpselect_ingest"
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    t, N, C = 2, 4, 8                                 # bf16: 64 bytes a frame row block, 128 bytes a piece
    x, out, dis = p, p + 1024, p + 2048
    _refused(lib.rtk_dpselect_ingest(None, None, t, N, C, nv.RTK_BF16, out, dis, None), E, name, b"NULL")
    _refused(lib.rtk_dpselect_ingest(x, None, t, N, C, nv.RTK_BF16, None, dis, None), E, name, b"NULL")
    _refused(lib.rtk_dpselect_ingest(x, None, t, N, C, nv.RTK_BF16, out, None, None), E, name, b"NULL")
    for shape in ((0, N, C), (t, 0, C), (t, N, 0), (-1, N, C)):
        _refused(lib.rtk_dpselect_ingest(x, None, *shape, nv.RTK_BF16, out, dis, None), E, name, b"shape")
    for code in (nv.RTK_BF16_REFROUND, nv.RTK_BF16_FAST, nv.RTK_F16_REFROUND, 17, -1):
        _refused(lib.rtk_dpselect_ingest(x, None, t, N, C, code, out, dis, None), E, name, b"dtype")
    for o in (x, x + 64, x + 127, x - 127):           # any byte in common
        _refused(lib.rtk_dpselect_ingest(x, None, t, N, C, nv.RTK_BF16, o, dis, None), E, name, b"overlaps")
    for prev in (out, out + 64, out + 127, out - 63):  # the halo row would be overwritten while it is read
        _refused(lib.rtk_dpselect_ingest(x, prev, t, N, C, nv.RTK_BF16, out, dis, None), E, name, b"prev")


def test_select_ring_refuses_bad_arguments_before_any_launch():
    import retake._native as nv

    lib, E, name = nv.lib, nv.RTK_EINVAL, b"rtk_dpselect_select_ring"
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)

    def call(R=16, N=4, r0=8, length=8, left=1, right=1, keep=4, window=3, sync=1, dis=p, idx=p, mask=p, keys=p):
        return lib.rtk_dpselect_select_ring(dis, R, N, r0, length, left, right, keep, window, sync, idx, mask, keys, None)

    for null in ("dis", "idx", "mask", "keys"):
        _refused(call(**{null: None}), E, name, b"NULL")
    for bad in (dict(R=0), dict(N=0), dict(window=0)):
        _refused(call(**bad), E, name, b"shape")
    for bad in (dict(r0=-1), dict(r0=16), dict(length=0)):
        _refused(call(**bad), E, name, b"segment")
    for bad in (dict(left=-1), dict(left=2), dict(right=-1), dict(right=2), dict(window=4, left=3), dict(window=4, right=2)):
        _refused(call(**bad), E, name, b"halo")
    _refused(call(length=15, keep=1), E, name, b"exceed")          # 15 + 1 + 1 > 16
    _refused(call(R=8, r0=0, length=8, left=0, right=1), E, name, b"exceed")
    for bad in (dict(keep=0), dict(keep=9), dict(keep=-3)):
        _refused(call(**bad), E, name, b"keep")
    _refused(call(N=1, sync=0), nv.RTK_EREFCRASH, name, b"IndexError")
    assert nv.lib.rtk_version() == 18                               # additions only


# ---- the schedule -------------------------------------------------------------------------------------------------------
def _brute(S, w, pushes):
    """Frame by frame: which ring row every frame goes to, and after which frame every segment leaves."""
    la = w - 1 - w // 2
    events, g, k = [], 0, 0
    for p, t in enumerate(pushes):
        for _ in range(t):
            events.append(("frame", p, g, g % (2 * S)))
            if g == (k + 1) * S - 1 + la:
                events.append(("emit", p, k))
                k += 1
            g += 1
    return events


@pytest.mark.parametrize("S, w, pushes", [
    (16, 3, [53]), (16, 3, [1] * 53), (16, 3, [5, 1, 47]), (16, 3, [15, 1, 1, 1, 14, 40, 0, 3]), (80, 3, [7, 200, 1, 37]),
    (4, 4, [1, 2, 3, 4, 5, 6, 7]), (5, 5, [13, 2, 2, 30]), (2, 1, [1, 1, 1, 4]), (2, 2, [9]), (6, 4, [6, 6, 6, 1, 23]),
    (3, 3, [100]),
])
def test_the_plan_is_the_brute_force_walk(S, w, pushes):
    from retake.dpselect_stream import plan_finish, plan_push, segment_geometry

    lb, la = w // 2, w - 1 - w // 2
    R = 2 * S
    want = _brute(S, w, pushes)
    got, seen, emitted, written_at = [], 0, 0, {}
    for p, t in enumerate(pushes):
        ops = plan_push(S, w, seen, t)
        covered = 0
        for op in ops:
            if op[0] == "ingest":
                _, off, cnt, g = op
                assert off == covered and g == seen and cnt >= 1
                assert g // R == (g + cnt - 1) // R, "a piece is one contiguous run of ring rows"
                assert cnt <= (S + la if g == 0 else S)   # between two emissions lie S frames; before the first, S + la
                # the row in front of the piece (the carry frame) is not among the rows the piece writes
                assert g == 0 or (g - 1) % R not in {(g + i) % R for i in range(cnt)}
                for i in range(cnt):
                    got.append(("frame", p, g + i, (g + i) % R))
                    written_at[(g + i) % R] = g + i
                covered += cnt
                seen += cnt
            else:
                k = op[1]
                assert k == emitted
                first, length, left, right = segment_geometry(S, w, k, seen)
                assert (first, length, right) == (k * S, S, la) and left == min(lb, first)
                # every row the selection and the gather read still holds the frame it should
                for g in range(first - left, first + length + right):
                    assert written_at[g % R] == g, (k, g)
                got.append(("emit", p, k))
                emitted += 1
        assert covered == t
    assert got == want
    # finish: every segment that has a frame and has not left, windows clipped at the last frame
    T = sum(pushes)
    for _, k in plan_finish(S, T, emitted):
        assert k == emitted
        first, length, left, right = segment_geometry(S, w, k, T)
        assert first == k * S and length == min(S, T - first) >= 1
        assert left == min(lb, first) and right == min(la, T - first - length)
        for g in range(first - left, first + length + right):
            assert written_at[g % R] == g, (k, g)
        emitted += 1
    assert emitted == -(-T // S)


def test_keep_counts():
    s = _stream(16, ratio=0.3)
    assert [s._keep_of(n) for n in (16, 5, 1, 2)] == [max(1, round(0.3 * n)) for n in (16, 5, 1, 2)] == [5, 2, 1, 1]
    assert _stream(10, ratio=0.25)._keep_of(10) == 2            # python's round: 2.5 -> 2, as the whole-video path
    s = _stream(16, keep=6)
    assert [s._keep_of(n) for n in (16, 6, 5, 1)] == [6, 6, 5, 1]


def test_the_restatement_on_a_hand_made_row():
    import dpselect_stream_ref as ref

    for kw in (dict(ratio=0.3), dict(ratio=0.25), dict(ratio=1.0), dict(keep=6)):   # the two sides count alike
        s = _stream(16, **kw)
        assert [s._keep_of(n) for n in range(1, 17)] == [ref.keep_count(n, **kw) for n in range(1, 17)]
    r = np.array([1.0, 0.2, 0.2, 0.5, 0.5, 0.1, 0.3, 0.3], dtype=np.float32)
    assert ref.peaks(r, 3).tolist() == [True, False, False, True, False, False, True, False]   # the first of a plateau
    # one patch position, sync: the mean of one value is the value
    segs = ref.select_stream(r[:, None], 4, 3, True, keep=2)
    assert [s[0].tolist() for s in segs] == [[0, 3], [4, 6]] and [s[1][:, 0].tolist() for s in segs] == [[True, True], [False, True]]
    # exact ties among non-peaks go to the lowest index: segment [1, 2] of S = 2 keeps frame ... the first
    segs = ref.select_stream(r[:, None], 2, 3, True, keep=1)
    assert [s[0].tolist() for s in segs] == [[0], [3], [4], [6]]
    d = np.random.default_rng(0).uniform(size=(5, 70)).astype(np.float32)
    assert np.allclose(ref.patch_mean(d), d.mean(1), rtol=1e-6)

"""DPSelect on a stream (retake/dpselect_stream.py) on the GPU.  Three yardsticks, none of them the code under test:
  * one segment closed by finish() must be `vc.dpselect_stages` on the same tensor, bit for bit - that call is pinned to the
    reference by the goldens;
  * the distance rows of many segments, concatenated, must be `dpselect_stages(...)[3]` of the whole video, bit for bit;
  * what is kept must be tests/dpselect_stream_ref.py (the rule restated in numpy) applied to the device's own distances, and
    the emitted frames must be torch's gather of the input at those indices.
Shapes are small: N 5..16, C 64 / 256 (16-byte vector rows) and 30 / 37 (the generic path), T <= 300."""
import functools

import numpy as np
import pytest
import torch

import dpselect_stream_ref as ref
import synth

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _video(seed, T, N, C, dtype, kind="video"):
    """[T, N, C] on the device; made once, shared, never written."""
    return torch.from_numpy(synth.make_frames(kind, seed, T, N, C)[0]).to(dev()).to(dtype).contiguous()


@functools.lru_cache(maxsize=None)
def _whole(seed, T, N, C, dtype, window):
    """The whole-video distance rows [T, N] of _video(...) (tgt = T: only the distances are used)."""
    import retake.visual_compression as vc

    return vc.dpselect_stages(_video(seed, T, N, C, dtype)[None], T, window, False)[3]


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(_bits(a), _bits(b)), what


def _run(x, cuts, S, **kw):
    """Push x [T, N, C] in pieces of the given sizes, finish; returns (segments, the push index each was emitted by)."""
    from retake.dpselect_stream import DPSelectStream

    assert sum(cuts) == x.shape[0]
    st = DPSelectStream(S, **kw)
    segs, at, o = [], [], 0
    for p, t in enumerate(cuts):
        got = st.push(x[o:o + t])
        segs += got
        at += [p] * len(got)
        o += t
    got = st.finish()
    return segs + got, at + ["finish"] * len(got), st


def _same_segments(a, b, what):
    assert len(a) == len(b), what
    for k, (s, t) in enumerate(zip(a, b)):
        assert (s.first_frame, s.num_frames) == (t.first_frame, t.num_frames), (what, k)
        for f in ("frames", "keypatches_mask", "idx", "dis"):
            _same(getattr(s, f), getattr(t, f), (what, k, f))


def _check_against_ref(x, segs, S, window, sync, ratio=None, keep=None):
    """Selection = the numpy restatement on the device's own distances; frames = torch's gather of the input."""
    T, N, C = x.shape
    dis = torch.cat([s.dis for s in segs])
    assert dis.shape == (T, N)
    want = ref.select_stream(dis.cpu().numpy(), S, window, sync, ratio=ratio, keep=keep)
    assert len(want) == len(segs) == -(-T // S)
    for k, (s, (idx, mask)) in enumerate(zip(segs, want)):
        assert (s.first_frame, s.num_frames) == (k * S, min(S, T - k * S)), k
        assert s.idx.dtype == torch.int64 and s.keypatches_mask.dtype == torch.bool
        assert np.array_equal(s.idx.cpu().numpy(), idx), (k, s.idx.cpu().numpy().T, idx.T)
        assert np.array_equal(s.keypatches_mask.cpu().numpy(), mask.reshape(-1)), k
        g = s.idx
        frames = x[g] if sync else x.gather(0, g[:, :, None].expand(-1, -1, C))
        _same(s.frames, frames[None], (k, "frames"))


# ---------------------------------------------------------------------------------------------------
# 1. one segment is the whole-video call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [3, 5])
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("dt, C", [("fp32", 64), ("bf16", 256), ("fp16", 64), ("bf16", 30), ("fp32", 37)])
def test_one_segment_is_the_whole_video_call(dt, C, sync, window):
    import retake.visual_compression as vc

    T, N, tgt = 41, 7, 13
    x = _video(3, T, N, C, DTYPES[dt])
    out, mask, idx, dis, _ = vc.dpselect_stages(x[None], tgt, window, sync)
    for cuts in ([T], [1] * T, [5, 1, T - 6]):
        segs, at, _ = _run(x, cuts, T, keep=tgt, window_size=window, sync=sync)
        assert len(segs) == 1 and at == ["finish"], cuts
        s = segs[0]
        assert (s.first_frame, s.num_frames) == (0, T)
        _same(s.frames, out, (cuts, "frames"))
        _same(s.keypatches_mask, mask.flatten(), (cuts, "mask"))
        _same(s.idx, idx, (cuts, "idx"))
        _same(s.dis, dis, (cuts, "dis"))


# ---------------------------------------------------------------------------------------------------
# 2. distances across seams
# ---------------------------------------------------------------------------------------------------
def _seam_cuts(S):
    """T = 3 S + 5 in pushes of which one is longer than the ring (2 S), one piece crosses the ring's wrap, some are 1."""
    T = 3 * S + 5
    cuts = [1, S - 3, 1, 2 * S + 4, 1]       # the 2 S + 4 push starts at S - 1 and runs over the wrap at 2 S
    cuts.append(T - sum(cuts))
    assert cuts[-1] > 0 and max(cuts) > 2 * S
    return T, cuts


@pytest.mark.parametrize("S", [16, 80])
@pytest.mark.parametrize("dt, C", [("fp32", 64), ("bf16", 256), ("fp16", 64), ("bf16", 30), ("fp16", 30), ("fp32", 37)])
def test_distances_across_seams(dt, C, S):
    T, cuts = _seam_cuts(S)
    N = 5
    x = _video(5, T, N, C, DTYPES[dt])
    segs, _, _ = _run(x, cuts, S, ratio=0.25)
    assert [s.num_frames for s in segs] == [S, S, S, 5]
    _same(torch.cat([s.dis for s in segs]), _whole(5, T, N, C, DTYPES[dt], 3), "dis rows of all segments")
    # and the ring held what was pushed: every kept frame is the input frame
    for s in segs:
        _same(s.frames[0], x[s.idx], "frames")


# ---------------------------------------------------------------------------------------------------
# 3. selection against the restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [3, 4, 5])
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("how", [dict(ratio=0.3), dict(keep=5), dict(ratio=1.0)], ids=["ratio", "keep", "all"])
@pytest.mark.parametrize("T", [53, 49])     # S = 16: a short last segment of 5 frames, and of ONE frame
def test_selection_is_the_restatement(T, how, sync, window):
    S, N, C = 16, 6, 64
    x = _video(7, T, N, C, torch.bfloat16)
    segs, _, _ = _run(x, [9, 1, 30, T - 40], S, window_size=window, sync=sync, **how)
    assert segs[-1].num_frames == T - 3 * S
    _check_against_ref(x, segs, S, window, sync, **how)
    _same(torch.cat([s.dis for s in segs]), _whole(7, T, N, C, torch.bfloat16, 3), "dis")


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("window", [3, 4])
def test_ties_across_a_seam_go_to_the_first_index(sync, window):
    """Runs of identical frames: inside a run the distance is the same value every time (the same pair of rows), so the keys
    tie exactly.  Run ENDS at k S - 1, k S and k S + 1 put the run's first frame - the only possible peak of a plateau - and
    the tied rest on either side of a seam."""
    S, N, C, T = 8, 5, 64, 40
    base = _video(11, T, N, C, torch.float32, "iid")
    starts = [0, 3, 8, 12, 17, 21, 26, 33, 37]          # runs end at 7 = S - 1, 16 = 2 S, 25 = 3 S + 1, 32 = 4 S, ...
    src = torch.zeros(T, dtype=torch.long)
    for a, b in zip(starts, starts[1:] + [T]):
        src[a:b] = a
    x = base[src.to(dev())].contiguous()
    segs, _, _ = _run(x, [T], S, keep=3, window_size=window, sync=sync)
    dis = torch.cat([s.dis for s in segs]).cpu().numpy()
    for a, b in zip(starts, starts[1:] + [T]):          # exact ties inside every run, per patch position
        assert (dis[a + 1:b] == dis[a + 1:a + 2]).all() and np.abs(dis[a + 1:b]).max() < 1e-6, (a, b)
    _check_against_ref(x, segs, S, window, sync, keep=3)
    again, _, _ = _run(x, [3, 5, 1, 1, 14, 16], S, keep=3, window_size=window, sync=sync)
    _same_segments(segs, again, "ties, another cutting")


# ---------------------------------------------------------------------------------------------------
# 4. split invariance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("dt, C", [("bf16", 256), ("fp32", 37)])
def test_split_invariance(dt, C, sync):
    S, T, N = 16, 3 * 16 + 5, 9
    x = _video(13, T, N, C, DTYPES[dt])
    runs = [_run(x, cuts, S, ratio=0.4, window_size=5, sync=sync)[0]
            for cuts in ([T], [1] * T, [17, 1, 14, 1, 20])]
    assert len(runs[0]) == 4
    _same_segments(runs[0], runs[1], "frame by frame")
    _same_segments(runs[0], runs[2], "odd cuts")


# ---------------------------------------------------------------------------------------------------
# 5. the seam artefact is gone
# ---------------------------------------------------------------------------------------------------
def test_a_segment_start_is_not_a_scene_cut():
    import retake.visual_compression as vc

    S, N, C, T = 16, 8, 64, 64
    cut = S + 3
    rng = np.random.default_rng(17)

    def plane():   # per patch position: two orthogonal directions of one length
        a, b = rng.standard_normal((2, N, C))
        b -= a * (a * b).sum(-1, keepdims=True) / (a * a).sum(-1, keepdims=True)
        return a, b * np.linalg.norm(a, axis=-1, keepdims=True) / np.linalg.norm(b, axis=-1, keepdims=True)

    # A slow drift that speeds up: frame t is frame t - 1 turned by 0.01 t rad in its scene's plane, so the distance
    # 1 - cos(0.01 t) grows with every frame (by >= 1.5e-4: far above fp32's rounding of a cosine) and NO frame is a local
    # maximum - except frame 0 (the constant 1.0), the cut (two unrelated scenes: a distance near 1) and the last frame.
    scenes, phi, frames = (plane(), plane()), 0.0, []
    for t in range(T):
        phi += 0.01 * t
        a, b = scenes[t >= cut]
        frames.append(np.cos(phi) * a + np.sin(phi) * b)
    x = torch.from_numpy(np.stack(frames).astype(np.float32)).to(dev())
    segs, _, _ = _run(x, [T], S, keep=2)
    d = torch.cat([s.dis for s in segs]).mean(1).cpu().numpy()
    assert (np.diff(d[1:cut]) > 0).all() and (np.diff(d[cut + 1:]) > 0).all() and d[cut] > 2 * d[1:cut].max()
    s1 = segs[1]
    kept = s1.idx.cpu().tolist()
    assert cut in kept and bool(s1.keypatches_mask.view(2, N)[kept.index(cut)].all())
    for k, s in enumerate(segs):
        if k == 0:
            continue    # (frame 0 IS a peak by the rule: its distance is the constant 1.0)
        m = s.keypatches_mask.view(-1, N).cpu()
        for r, g in enumerate(s.idx.cpu().tolist()):
            assert not (g == k * S and bool(m[r].any())), f"frame {g} flagged merely for starting segment {k}"
    # the per-segment whole-video call on the same frames flags every segment start
    for k in range(T // S):
        out, mask, idx, _, _ = vc.dpselect_stages(x[None, k * S:(k + 1) * S], 2, 3, True)
        assert int(idx[0]) == 0 and bool(mask[0].all()), k


# ---------------------------------------------------------------------------------------------------
# 6. lifecycle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [3, 4, 5])
def test_emission_points(window):
    S, N, C = 8, 5, 64
    T = 3 * S + 2
    la = window - 1 - window // 2
    x = _video(19, T, N, C, torch.bfloat16)
    segs, at, st = _run(x, [1] * T, S, ratio=0.5, window_size=window)
    # one frame a push: push p delivers frame p
    assert at == [(k + 1) * S - 1 + la for k in range(3)] + ["finish"]
    assert [s.first_frame for s in segs] == [0, S, 2 * S, 3 * S] and segs[-1].num_frames == 2
    assert (st.frames_seen, st.segments_emitted) == (T, 4)


def test_finish_reset_and_the_ring():
    from retake.dpselect_stream import DPSelectStream

    S, N, C = 8, 6, 64
    T = 10 * S + 3
    x = _video(23, T, N, C, torch.float16)
    st = DPSelectStream(S, ratio=0.5, sync=False)
    first = st.push(x[:5])
    assert first == [] and st.frames_seen == 5
    ptrs = (st._frames.data_ptr(), st._dis.data_ptr(), st._keys.data_ptr())
    foot = st.memory_footprint()
    assert foot >= 2 * S * N * C * 2 + 2 * S * N * 4
    run1 = st.push(x[5:]) + st.finish()
    assert len(run1) == 11 and st.finish() == []
    with pytest.raises(RuntimeError, match="finish"):
        st.push(x[:1])
    st.reset()
    assert (st.frames_seen, st.segments_emitted) == (0, 0)
    run2 = []
    for o in range(0, T, 7):
        run2 += st.push(x[None, o:o + 7])            # the [1, t, N, C] form
    run2 += st.finish()
    _same_segments(run1, run2, "after reset")
    assert ptrs == (st._frames.data_ptr(), st._dis.data_ptr(), st._keys.data_ptr()) and foot == st.memory_footprint()
    # what may not change between pushes
    st.reset()
    st.push(x[:3])
    for bad in (x[:2, :5], x[:2, :, :32], x[:2].float(), x[:2].cpu()):
        with pytest.raises((ValueError, RuntimeError)) as ei:
            st.push(bad)
        assert type(ei.value) is (RuntimeError if not bad.is_cuda else ValueError)
    assert st.frames_seen == 3
    assert st.push(x[:0]) == [] and st.frames_seen == 3
    # a non-contiguous push is made contiguous
    st.reset()
    xt = x[:S + 2].transpose(0, 1).contiguous().transpose(0, 1)
    assert not xt.is_contiguous()
    _same_segments(st.push(xt), run1[:1], "non-contiguous input")


def test_a_one_frame_stream_emits_its_frame():
    for sync in (True, False):
        x = _video(29, 4, 5, 64, torch.bfloat16)[:1]
        segs, at, _ = _run(x, [1], 4, ratio=0.5, sync=sync)
        assert len(segs) == 1 and at == ["finish"]
        s = segs[0]
        _same(s.frames, x[None], "the frame")
        assert bool(s.keypatches_mask.all()) and s.keypatches_mask.numel() == 5      # a lone peak
        assert int(s.idx.abs().sum()) == 0 and bool((s.dis == 1.0).all()) and s.dis.shape == (1, 5)


# ---------------------------------------------------------------------------------------------------
# 7. with the bounded cache
# ---------------------------------------------------------------------------------------------------
def test_stream_into_a_budgeted_cache():
    """INTEGRATION.md §1's loop for a live stream: frames -> stream.push -> per segment one chunk of keep_k * N tokens with
    cache.keypatches_mask_chunk = seg.keypatches_mask -> the update -> after_forward(), into a video_budget_rows cache."""
    from retake.dpselect_stream import DPSelectStream
    from test_budget_gpu import RATIO, _BudgetDriver
    from test_rewind_gpu import LAYERS, TEXT, _qkv

    S, N, C, keep_frames = 8, 16, 64, 4
    L = keep_frames * N                     # 64 tokens a chunk: the driver's 8 x 8 grids
    keep = int(RATIO * L)
    B = keep + keep // 2
    d = _BudgetDriver("update", "mrope", torch.bfloat16, L, B=B, S=0, reserve=TEXT + B + L + 8)
    cache = d.cache
    d.step(1, TEXT)
    stream = DPSelectStream(S, keep=keep_frames)
    x = _video(31, 10 * S + 1, N, C, torch.bfloat16, "iid")
    seen, chunks = {}, 0
    for o in range(0, x.shape[0], 5):       # frames arrive five at a time
        for seg in stream.push(x[o:o + 5]):
            assert seg.frames.shape == (1, keep_frames, N, C) and seg.keypatches_mask.shape == (L,)
            pos = d._video_ids(L, 0)
            cache.keypatches_mask_chunk = seg.keypatches_mask      # one entry per chunk token: the cache takes it as it is
            for l in range(LAYERS):
                q, k, v = _qkv(1000 * (2 + chunks) + l, L, torch.bfloat16)
                qr, kk, vv = d._feed(l, q, k, v, pos, True)
                assert cache.attention(qr, kk, vv, layer_idx=l) is not None
            cache.keypatches_mask_chunk = None
            chunks += 1
            # the key-patch rows of the newest chunk carry 1.0: read before after_forward() lets the budget drop rows (the
            # chunk's kept rows are then the region's last `keep`; the last layer's selection is the one still readable)
            idx = cache.last_keep_indices
            stored = cache.row_scores(LAYERS - 1)[-keep:]
            patch = seg.keypatches_mask[idx]
            assert int(patch.sum()) > 0 and bool((stored[patch] == 1.0).all()), chunks
            cache.after_forward()
            cache.kvcache_compression = False
            if chunks in (4, 10):
                seen[chunks] = (stream.memory_footprint(), cache.memory_footprint(),
                                [st.k.data_ptr() for st in cache._layers], stream._frames.data_ptr())
    assert chunks == 10 and stream.segments_emitted == 10
    assert seen[4] == seen[10]              # both footprints have stopped growing
    assert cache.get_seq_length(0) == TEXT + B

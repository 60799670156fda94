"""PivotKVCache.mark / rewind / crop and the follow-up glue, the parts that need no GPU: the mark object, the ids of a
follow-up question, what is refused, the prefill driver's note on `video_end`, and the host bookkeeping on adopted (CPU)
tensors.  The twin runs against a fresh cache are in tests/test_rewind_gpu.py."""
import types

import pytest
import torch


def _cfg(**extra):
    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    kw.update(extra)
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs={"kvcache_compression": True, "kvcache_compression_kwargs": kw})


def _cache(**extra):
    import retake.longvideo_cache as lc

    return lc.build_kvcache(_cfg(**extra))


def _adopted(rows=10, layers=2):
    """A cache whose layers were assigned wholesale (what HF's utilities do): `rows` rows per layer, ids included."""
    cache = _cache()
    g = torch.Generator().manual_seed(0)
    cache.key_cache = [torch.randn((1, 2, rows, 128), generator=g) for _ in range(layers)]
    cache.value_cache = [torch.randn((1, 2, rows, 128), generator=g) for _ in range(layers)]
    cache.position_cache = [torch.arange(rows).view(1, 1, rows).repeat(3, 1, 1) for _ in range(layers)]
    return cache


def test_cache_mark_is_immutable():
    import retake.longvideo_cache as lc

    cache = _adopted()
    m = cache.mark()
    assert isinstance(m, lc.CacheMark) and m.cache is cache and m.resume_position_ids is None
    assert m.n_layers == 2 and m.pos_layers == 2 and m.n_evicted == 0 and m.epoch == cache._epoch
    assert [(x.length, x.pos_len, x.pos_ndim, x.len8, x.archive_at, x.num_evicted) for x in m.layers] == [(10, 10, 3, 0, -1, 0)] * 2
    for name, value in (("serial", 0), ("layers", ()), ("resume_position_ids", torch.zeros(3)), ("anything", 1)):
        with pytest.raises(AttributeError):
            setattr(m, name, value)
    with pytest.raises(AttributeError):
        del m.serial
    assert cache.mark().serial == m.serial + 1
    del cache
    assert m.cache is None      # a weak reference: a mark does not keep gigabytes of device memory alive


@pytest.mark.parametrize("P", [1, 3])
def test_followup_position_ids(P):
    import retake._prefill as pf

    resume = torch.tensor([41, 17, 9][:P])
    mark = _adopted().mark()._with_resume(resume)
    for n in (1, 5):
        got = pf.followup_position_ids(mark, n, "cpu")
        assert got.dtype == torch.int64 and got.shape == ((3, 1, n) if P == 3 else (1, n))
        assert torch.equal(got.reshape(P, n), resume.view(P, 1) + torch.arange(n))
    assert pf.followup_position_ids(mark, 2).device.type == "cpu"
    with pytest.raises(ValueError, match="resume_position_ids"):
        pf.followup_position_ids(_adopted().mark(), 3, "cpu")


def test_defer_rerotation_has_no_marks():
    cache = _cache(defer_rerotation=True)
    with pytest.raises(NotImplementedError, match="defer_rerotation"):
        cache.mark()
    cache._compressed_in_forward = True     # what a compressed update leaves behind
    cache.after_forward()                   # ... takes no mark, and does not raise
    assert cache.video_end is None and cache.last_compressed_mark is None


def test_rewind_and_crop_bookkeeping():
    """The host side on adopted tensors: HF's crop semantics, what a rewind restores, what is refused."""
    cache = _adopted(10)
    k0 = cache.key_cache[0].clone()
    m10 = cache.mark()
    cache.crop(10 ** 9)
    cache.crop(10)
    assert cache.get_seq_length() == 10
    cache.crop(-3)
    assert [cache.get_seq_length(l) for l in range(2)] == [7, 7] and cache.position_cache[1].shape == (3, 1, 7)
    assert torch.equal(cache.key_cache[0], k0[:, :, :7])
    with pytest.raises(ValueError, match="invalidated"):      # the crop gave up rows m10 names
        cache.rewind(m10)
    m7 = cache.mark()
    cache.crop(4)
    assert cache.get_seq_length(1) == 4 and torch.equal(cache.value_cache[1], cache._layers[1].v[:, :, :4])
    with pytest.raises(ValueError):
        cache.rewind(m7)
    with pytest.raises(ValueError):
        cache.crop(-5)                                        # below row 0
    assert cache.get_seq_length() == 4
    # rewind: numbers back, later layers / counts dropped, later marks void, earlier ones good
    m4 = cache.mark()
    ptr = cache._layers[0].k.data_ptr()
    st = cache._layers[0]
    st.length, st.pos_len = 9, 9                              # rows appended at `length` (what text and decode do)
    cache._store(2)                                           # a layer that did not exist at the mark
    cache.update_num_evicted_tokens(5, 2)
    cache._prompt_len, cache._preshifted = 3, object()
    m9 = cache.mark()
    assert m9.n_layers == 3 and m9.n_evicted == 3 and m9.layers[2].num_evicted == 5 and not m9.layers[2].has_kv
    assert cache.rewind(m4) is None
    assert len(cache) == 2 and cache.num_evicted_tokens == [] and cache.get_seq_length(0) == 4 and st.pos_len == 4
    assert cache._prompt_len == 0 and cache._preshifted is None and cache._layers[0].k.data_ptr() == ptr
    with pytest.raises(ValueError, match="invalidated"):
        cache.rewind(m9)
    cache.rewind(m4)
    # refusals that change nothing
    other = _adopted(10)
    with pytest.raises(ValueError, match="another cache"):
        cache.rewind(other.mark())
    with pytest.raises(ValueError):
        cache.rewind("video_end")
    st.length = 2
    with pytest.raises(ValueError, match="shorter"):
        cache.rewind(m4)
    st.length = 4
    cache.position_cache = cache.position_cache             # buffers replaced: the epoch moves
    with pytest.raises(ValueError, match="replaced"):
        cache.rewind(m4)
    assert cache.get_seq_length(0) == 4


def test_crop_refuses_compressed_rows():
    """Below the boundary after the most recent compressed flush a length cannot restore the eviction counts."""
    cache = _adopted(10)
    cache.num_evicted_tokens[:] = [30, 30]
    cache._flushes = 1                          # a compressed flush happened ...
    with pytest.raises(ValueError, match="compressed"):
        cache.crop(9)                           # ... and no after_forward recorded its boundary: nothing may be cut
    cache._compressed_in_forward = True
    cache.after_forward()                       # the boundary: 10 rows
    assert cache.video_end is not None and cache.video_end.compressed and cache.video_end.layers[0].num_evicted == 30
    for st in cache._layers:
        st.length, st.pos_len = 14, 14          # a question and its answer
    cache.crop(-2)
    assert cache.get_seq_length() == 12
    with pytest.raises(ValueError, match="compressed"):
        cache.crop(9)
    assert cache.get_seq_length() == 12 and cache.num_evicted_tokens == [30, 30]
    cache.crop(10)
    assert cache.get_seq_length() == 10
    cache.rewind(cache.video_end)               # still good: the crop voids the marks AFTER video_end only


def test_prefill_driver_notes_the_resume_ids():
    import retake._prefill as pf

    for P in (3, 1):
        cache = _adopted(4)
        S = 20
        pos = (torch.arange(S) + 100).view(1, S).repeat(P, 1)
        pos = pos.view(3, 1, S) if P == 3 else pos
        want = pos[..., 15].reshape(P).clone()
        seen = []

        def run_text(s, e, pos=pos, cache=cache):
            seen.append((s, e, cache.video_end))
            pos[..., s:e] += 1000                 # what the Qwen2-VL attention patch does to the forward's ids, in place
            return None

        def run_video_chunk(ss, ee, cache=cache):
            cache._compressed_in_forward = True
            cache.after_forward()
            return None

        segs = [(0, 3, "text"), (3, 15, "video"), (15, S, "text")]
        pf.run_chunked_prefill(segs, 6, cache, None, run_text, run_video_chunk, position_ids=pos)
        assert seen[0][2] is None and seen[1][2].resume_position_ids is not None   # noted before the trailing text ran
        m = cache.video_end
        assert m.resume_position_ids.dtype == torch.int64 and torch.equal(m.resume_position_ids, want)
        assert torch.equal(pf.followup_position_ids(m, 5), (pos[..., 15:] - 1000))
        assert cache.kvcache_compression is False
        # segments that do not line up with the ids (the reference segments before its visual compression drops tokens):
        # nothing is noted, nothing raises; and a caller that passes no ids gets the driver as it was
        for kw in ({"position_ids": pos[..., :17]}, {}):
            cache = _adopted(4)
            pf.run_chunked_prefill(segs, 6, cache, None, lambda s, e: None,
                                   lambda ss, ee, cache=cache: (setattr(cache, "_compressed_in_forward", True), cache.after_forward()),
                                   **kw)
            assert cache.video_end is not None and cache.video_end.resume_position_ids is None

"""PivotKVCache.fork and the rtk_attention_*_shared entry points, the parts that need no GPU: the four entries are declared,
exported and bound; their host-side validation returns the stated codes without a device; the workspace-bytes equalities
of include/retake_hip.h "Shared 16-bit rows" over a small grid; and every refusal of a fork / a branch that is raised
before a launch, on adopted (CPU) tensors.  The kernels are in tests/test_attention_shared_gpu.py, the twin runs of a
branch against a fresh cache in tests/test_fork_gpu.py."""
import ctypes
import gc
import itertools
import types

import pytest
import torch

NEW = ["rtk_attention_workspace_bytes_shared", "rtk_attention_forward_shared", "rtk_attention_decode_workspace_bytes_shared",
       "rtk_attention_decode_shared"]


def test_entry_points_are_declared_exported_and_bound():
    import retake._native as nv
    import test_abi_cpu

    syms = test_abi_cpu._declared_symbols()
    lib = ctypes.CDLL(nv.LIB_PATH)
    for s in NEW:
        assert s in syms, f"{s} not declared in retake_hip.h"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in nv.EXPORTS, f"{s} not bound"
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18


def _call(nv, fn, p, q="p", ks="p", k8="p", Ls=64, L8=64, Lq=2, Lk=64, q_offset=None, D=128, dtype=None, s_sh=None, s_sl=128,
          stride8=8192, Hq=4, Hkv=2, ws=None, ws_bytes=0):
    q = p if q == "p" else q
    ks = p if ks == "p" else ks
    k8 = p if k8 == "p" else k8
    dtype = nv.RTK_BF16 if dtype is None else dtype
    q_offset = Lk - Lq if q_offset is None else q_offset
    s_sh = max(Ls, 1) * s_sl if s_sh is None else s_sh
    return getattr(nv.lib, fn)(q, Lq * D, D, p, p, Lk * D, D, ks, p, Ls, s_sh, s_sl, k8, p, p, p, L8, stride8, 64, p, Hq, Hkv,
                               Lq, Lk, q_offset, D, dtype, 0.088, ws, ws_bytes, None)


@pytest.mark.parametrize("fn", ["rtk_attention_forward_shared", "rtk_attention_decode_shared"])
def test_host_side_validation(fn):
    """Every error is raised before any launch: the codes and what the message names, with no device in the machine."""
    import retake._native as nv

    dummy = (ctypes.c_char * 512)()
    p = (ctypes.addressof(dummy) + 15) & ~15
    err = nv.lib.rtk_last_error
    c = lambda **k: _call(nv, fn, p, **k)   # noqa: E731
    assert c(q=None) == nv.RTK_EINVAL and b"NULL" in err()
    assert c(Ls=-1) == nv.RTK_EINVAL and b"Ls" in err()
    assert c(ks=None) == nv.RTK_EINVAL and b"shared" in err()
    assert c(L8=-1) == nv.RTK_EINVAL
    assert c(k8=None) == nv.RTK_EINVAL and b"archive" in err()
    assert c(q_offset=-1) == nv.RTK_EINVAL
    assert c(dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and b"dtype" in err()
    assert c(D=64) == nv.RTK_EUNSUPPORTED and b"head_dim" in err()
    assert c(ks=p + 2) == nv.RTK_EUNSUPPORTED and b"shared" in err()
    assert c(s_sl=132) == nv.RTK_EUNSUPPORTED and b"shared" in err()          # a row stride of 264 bytes
    assert c(s_sh=64 * 128 + 4) == nv.RTK_EUNSUPPORTED and b"shared" in err()
    assert c(s_sl=64) == nv.RTK_EUNSUPPORTED and b"shared" in err()           # rows that overlap
    assert c(Ls=1 << 22, s_sl=256) == nv.RTK_EUNSUPPORTED and b"2 GiB" in err()
    assert c(stride8=8200) == nv.RTK_EUNSUPPORTED
    if fn == "rtk_attention_decode_shared":
        assert c(Lq=9, Lk=64) == nv.RTK_EUNSUPPORTED and b"packed rows" in err()      # R = 18
        assert c() == nv.RTK_EWORKSPACE and b"rtk_attention_decode_workspace_bytes_shared" in err()
    else:
        assert c(Lq=2, Lk=40, Ls=1536, L8=0, k8=None) == nv.RTK_EWORKSPACE and b"rtk_attention_workspace_bytes_shared" in err()
    # no shared rows: the shared pointers are not looked at, the call is the _fp8kv one (here: its workspace error)
    assert c(ks=None, Ls=0, Lq=1, Lk=1, L8=100352) == nv.RTK_EWORKSPACE and b"fp8kv" in err()


def test_workspace_bytes_equalities():
    """Ls == 0 is the _fp8kv query (with L8 == 0 the plain one); Ls a multiple of the tile is the query over the
    concatenation; an unaligned Ls is rounded up to whole tiles (the padded index space)."""
    import retake._native as nv

    L, bf = nv.lib, nv.RTK_BF16
    grid = list(itertools.product([(4, 2), (28, 4)], [1, 2, 130], [0, 37, 64, 4096], [0, 64, 192, 1536, 100352]))
    for (Hq, Hkv), Lq, L8, Ls in grid:
        Lk = Lq + 39
        got = L.rtk_attention_workspace_bytes_shared(Hq, Hkv, Lq, Lk, L8, Ls, 128, bf)
        assert got == L.rtk_attention_workspace_bytes_fp8kv(Hq, Hkv, Lq, Lk + Ls, L8, 128, bf), (Hq, Lq, L8, Ls)
        if L8 == 0:
            assert got == L.rtk_attention_workspace_bytes(Hq, Hkv, Lq, Lk + Ls, 128, bf)
        if (Hq // Hkv) * Lq <= 16:
            got = L.rtk_attention_decode_workspace_bytes_shared(Hq, Hkv, Lq, Lk, L8, Ls, 128, bf)
            assert got == L.rtk_attention_decode_workspace_bytes_fp8kv(Hq, Hkv, Lq, Lk + Ls, L8, 128, bf) > 0
            if L8 == 0:
                assert got == L.rtk_attention_decode_workspace_bytes(Hq, Hkv, Lq, Lk + Ls, 128, bf)
    # unaligned: the segment counts as whole tiles (64 chunk, 32 decode)
    assert L.rtk_attention_workspace_bytes_shared(4, 2, 2, 40, 0, 1500, 128, bf) == \
        L.rtk_attention_workspace_bytes(4, 2, 2, 40 + 1536, 128, bf) > 0
    assert L.rtk_attention_decode_workspace_bytes_shared(4, 2, 2, 40, 45, 1045, 128, bf) == \
        L.rtk_attention_decode_workspace_bytes(4, 2, 2, 40 + 64 + 1056, 128, bf)
    # outside the envelope: 0, with the reason
    assert L.rtk_attention_workspace_bytes_shared(4, 2, 2, 40, 0, 64, 128, nv.RTK_F32) == 0 and b"unsupported" in L.rtk_last_error()
    assert L.rtk_attention_workspace_bytes_shared(4, 2, 2, 40, 0, -1, 128, bf) == 0 and b"Ls" in L.rtk_last_error()
    assert L.rtk_attention_decode_workspace_bytes_shared(4, 2, 9, 40, 0, 64, 128, bf) == 0 and b"packed rows" in L.rtk_last_error()


# ---------------------------------------------------------------------------------------------------
# fork: host bookkeeping and refusals on adopted (CPU) tensors
# ---------------------------------------------------------------------------------------------------
def _cfg(hip=True, heads=4, **extra):
    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    kw.update(extra)
    top = {"kvcache_compression": True, "kvcache_compression_kwargs": kw}
    if hip:
        top["attention_kernel"] = "hip"
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=heads, num_key_value_heads=2,
                                 longvideo_kwargs=top)


def _adopted(rows=10, dtype=torch.bfloat16, **kw):
    import retake.longvideo_cache as lc

    cache = lc.build_kvcache(_cfg(**kw))
    D = 512 // kw.get("heads", 4)
    g = torch.Generator().manual_seed(0)
    cache.key_cache = [torch.randn((1, 2, rows, D), generator=g).to(dtype) for _ in range(2)]
    cache.value_cache = [torch.randn((1, 2, rows, D), generator=g).to(dtype) for _ in range(2)]
    cache.position_cache = [torch.arange(rows).view(1, 1, rows).repeat(3, 1, 1) for _ in range(2)]
    cache.kvcache_compression = False
    return cache


def _append(cache, n, seed=1):
    """n text rows, as `update`'s else-branch stores them (which itself wants device tensors): room in the layer's own
    buffers, the rows, the ids.  Returns the last layer's K / V views as `update` does."""
    g = torch.Generator().manual_seed(seed)
    t0 = cache.get_seq_length(0)
    for l in range(2):
        k, v = (torch.randn((1, 2, n, 128), generator=g).to(torch.bfloat16) for _ in range(2))
        st = cache.reserve(l, n, k)
        st.k[:, :, st.length:st.length + n].copy_(k)
        st.v[:, :, st.length:st.length + n].copy_(v)
        st.length += n
        cache.update_position_ids(torch.arange(t0, t0 + n).view(1, 1, n).repeat(3, 1, 1), l)
    return st.k[:, :, :st.length], st.v[:, :, :st.length]


def test_fork_refusals():
    with pytest.raises(ValueError, match="attention_kernel"):
        _adopted(hip=False).fork()
    with pytest.raises(NotImplementedError, match="defer_rerotation"):
        _adopted(defer_rerotation=True).fork()
    with pytest.raises(NotImplementedError, match="float32"):
        _adopted(dtype=torch.float32).fork()
    with pytest.raises(NotImplementedError, match="head_dim"):
        _adopted(heads=8).fork()
    cache, other = _adopted(), _adopted()
    with pytest.raises(ValueError, match="another cache"):
        cache.fork(other.mark())
    with pytest.raises(ValueError):
        cache.fork("video_end")
    m = cache.mark()
    _append(cache, 3)
    m2 = cache.mark()
    cache.rewind(m)
    with pytest.raises(ValueError, match="invalidated"):       # checked as rewind checks it
        cache.fork(m2)
    br = cache.fork(m)
    with pytest.raises(NotImplementedError, match="nested"):
        br.fork()


def test_branch_bookkeeping_and_refusals():
    cache = _adopted(10)
    _append(cache, 2)
    m = cache.mark()
    _append(cache, 4, seed=2)                         # the parent goes on above the fork point
    br = cache.fork(m, reserve_tokens=16)
    assert br.forked_from is m and br.kvcache_compression is False and br.attention_kernel == "hip"
    assert br.reserve_tokens == 16 and br.num_evicted_tokens == cache.num_evicted_tokens
    for l in range(2):
        assert br.get_seq_length(l) == 12 and br.shared_len(l) == 12 and br.archive_len(l) == 0
        assert int(br.get_prev_temporal_idx(l)) == 11
        ks, vs = br.shared(l)
        st, pst = br._layers[l], cache._layers[l]
        assert ks.untyped_storage().data_ptr() == pst.k.untyped_storage().data_ptr() and ks.shape == (1, 2, 12, 128)
        assert vs.untyped_storage().data_ptr() == pst.v.untyped_storage().data_ptr()
        assert st.length == 0 and st.k.shape == (1, 2, 16, 128) and st.pos.data_ptr() != pst.pos.data_ptr()
        assert torch.equal(br.position_cache[l], cache.position_cache[l][..., :12])
        # reading gives a dense copy in sequence order
        assert torch.equal(br.key_cache[l], cache.key_cache[l][:, :, :12])
        assert br.key_cache[l].untyped_storage().data_ptr() != pst.k.untyped_storage().data_ptr()
    assert cache.shared_len(0) == 0 and cache.shared(0) is None and cache.forked_from is None
    # text rows go into the branch's own buffers; the parent's are untouched
    before = [cache.key_cache[l].clone() for l in range(2)]
    kk, vv = _append(br, 3, seed=3)
    assert kk.shape == (1, 2, 3, 128) and br.get_seq_length(0) == 15 and cache.get_seq_length(0) == 16
    assert all(torch.equal(cache.key_cache[l], before[l]) for l in range(2))
    assert torch.equal(br.key_cache[1][:, :, :12], before[1][:, :, :12]) and torch.equal(br.value_cache[1][:, :, 12:], vv)
    assert br.position_cache[0].shape == (3, 1, 15) and int(br.get_prev_temporal_idx(0)) == 14
    # mark / rewind / crop within its own rows; the crop floor is the fork point
    bm = br.mark()
    _append(br, 2, seed=4)
    br.rewind(bm)
    assert br.get_seq_length(0) == 15
    br.crop(13)
    assert br.get_seq_length(0) == 13 and br._layers[0].length == 1 and br._layers[0].pos_len == 13
    with pytest.raises(ValueError, match="compressed"):
        br.crop(11)
    br.crop(12)
    assert br.get_seq_length(0) == 12
    # what a branch refuses before any launch
    br.kvcache_compression = True
    k = torch.zeros((1, 2, 64, 128), dtype=torch.bfloat16)
    q = torch.zeros((1, 4, 64, 128), dtype=torch.bfloat16)
    ids = torch.arange(64).view(1, 1, 64).repeat(3, 1, 1)
    with pytest.raises(NotImplementedError, match="questions, not video"):
        br.update(k, k, 0, {"query_states": q, "position_ids": ids, "rotary_emb": None})
    with pytest.raises(NotImplementedError, match="questions, not video"):
        br.update_pre_rope(q, k, k, 0, ids, None)
    br.kvcache_compression = False
    assert br.get_seq_length(0) == 12
    for view in (br.key_cache, br.value_cache):
        with pytest.raises(NotImplementedError, match="branch"):
            view[0] = torch.zeros(1, 2, 3, 128)
    with pytest.raises(NotImplementedError, match="branch"):
        br.key_cache = [torch.zeros(1, 2, 3, 128)] * 2
    with pytest.raises(NotImplementedError, match="branch"):
        br.value_cache = [torch.zeros(1, 2, 3, 128)] * 2
    assert br.get_seq_length(0) == 12 and br.shared_len(0) == 12
    with pytest.raises(ValueError, match="layer_idx"):
        br.attention(None, None, None)


def test_native_attention_refusals_on_a_branch():
    """A call the native attention declines raises on a branch, naming the reason, exactly as the fp8 caches do: no other
    route sees the shared rows."""
    import retake.native_attention as na

    cache = _adopted(10)
    br = cache.fork()
    mod = types.SimpleNamespace(training=False, layer_idx=0, config=None)
    q = torch.zeros((1, 4, 2, 128), dtype=torch.bfloat16)
    k = torch.zeros((1, 2, 2, 128), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="output_attentions"):
        na.native_attention(mod, br, q, k, k, "causal", output_attentions=True)
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        na.native_attention(mod, br, q, k, k, "causal")
    # the parent, which has other routes, declines quietly
    assert na.native_attention(mod, cache, q, k, k, "causal", output_attentions=True) is None


def test_invalidation():
    cache = _adopted(10)
    m0 = cache.mark()
    _append(cache, 2)
    m = cache.mark()
    br = cache.fork(m)
    # the parent answers its own question above the fork point and rewinds to the fork point itself: the branch stays valid
    _append(cache, 3, seed=5)
    cache.rewind(m)
    _append(br, 1, seed=6)
    assert br.get_seq_length(0) == 13
    # below the fork point: every later call on the branch raises what rewind raises for such a mark
    cache.rewind(m0)
    k1 = torch.zeros((1, 2, 1, 128), dtype=torch.bfloat16)
    ids1 = torch.zeros((3, 1, 1), dtype=torch.int64)
    for call in (lambda: br.update(k1, k1, 0, {"position_ids": ids1}), lambda: br.append_pre_rope(k1, k1, k1, 0, ids1, None),
                 br.mark, lambda: br.crop(12), lambda: br.rewind(br.video_end),
                 lambda: br.attention(None, None, None, layer_idx=0), lambda: br.key_cache[0]):
        with pytest.raises(ValueError, match="invalidated"):
            call()
    with pytest.raises(ValueError, match="invalidated"):
        cache.rewind(m)
    # ... also once the parent is gone
    del cache
    gc.collect()
    with pytest.raises(ValueError, match="invalidated"):
        br.mark()
    # buffers of the parent replaced wholesale: the epoch
    cache = _adopted(10)
    br = cache.fork()
    cache.position_cache = cache.position_cache
    with pytest.raises(ValueError, match="replaced"):
        br.mark()
    # a parent that was merely released keeps the branch valid: the views own the storage
    cache = _adopted(10)
    want = cache.key_cache[0].clone()
    br = cache.fork()
    del cache
    gc.collect()
    assert br.forked_from.cache is None
    _append(br, 2, seed=7)
    assert br.get_seq_length(0) == 12 and torch.equal(br.key_cache[0][:, :, :10], want)


def test_followup_ids_of_a_branch_forked_at_video_end():
    import retake._prefill as pf

    cache = _adopted(10)
    cache.last_compressed_mark = cache._take_mark(True)          # what after_forward leaves after a video chunk
    cache.set_resume_position_ids(torch.tensor([[41], [17], [9]]))
    br = cache.fork(cache.video_end)
    assert br.forked_from is cache.video_end
    got = pf.followup_position_ids(br.forked_from, 4, "cpu")
    assert got.shape == (3, 1, 4) and torch.equal(got[:, 0, 0], torch.tensor([41, 17, 9]))
    assert torch.equal(br.video_end.resume_position_ids, torch.tensor([41, 17, 9]))

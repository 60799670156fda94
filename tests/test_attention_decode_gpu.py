"""The GQA-packed few-row attention (rtk_attention_decode / _fp8kv, chunk_attention(packed_gqa=True),
decode_attention="packed") on the GPU: float64 truth under the project's "2E" rule, splits above a row's diagonal,
causality against NaN rows, views, reproducibility, declines, the fp8 archive, and the product route through the cache.
Every case checks that the packed kernel really ran: a silent fall-back to the chunk kernels would pass the numbers."""
import math
import os
import types

import numpy as np
import pytest
import torch

import attention_ref as ar
import fp8_ref
import synth

pytestmark = pytest.mark.gpu

D = 128
SEC = [16, 24, 24]
A = synth.YARN_FACTOR4_ATTENTION_SCALING


def dev():
    return torch.device("cuda:0")


def _note(line: str):
    """Print a measured figure; also append it to $RETAKE_DECODE_ATTENTION_STATS when set
    (profiles/decode_attention_parity_stats.txt)."""
    print(line, flush=True)
    path = os.environ.get("RETAKE_DECODE_ATTENTION_STATS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _packed(q, k, v, **kw):
    """chunk_attention through the packed kernel - asserted, not assumed."""
    import retake.longvideo_cache as lc

    route = []
    out = lc.chunk_attention(q, k, v, packed_gqa=True, route=route, **kw)
    assert route == ["packed"], f"the packed kernel did not take this call: {route}"
    assert out.shape == (1, q.shape[2], q.shape[1], q.shape[3]) and out.dtype == q.dtype and out.is_contiguous()
    return out


def _inputs(kind, seed, Hq, Hkv, Lq, Lk, d, dtype):
    """attention_ref.make_inputs with k and v laid out alike (a broadcast one-row k otherwise keeps strides of its own)."""
    q, k, v = ar.make_inputs(kind, seed, Hq, Hkv, Lq, Lk, d, dtype, dev())
    return q, k.clone(memory_format=torch.contiguous_format), v.clone(memory_format=torch.contiguous_format)


def _plan(Hkv, K):
    """The rule of include/retake_hip.h (rtk_attention_decode), restated: (nsplit, keys per split)."""
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    n0 = max(1, min(ceil(512, Hkv), ceil(K, 128)))
    kps = 128 * ceil(ceil(K, n0), 128)
    return ceil(K, kps), kps


def _against_fp64(tag, q, k, v, out, dtype):
    """The "2E" rule of test_fast_path_against_fp64_within_twice_the_eager_error: within max(2 E, half an output ulp) of
    float64, E the eager expression's error on the same tensors (measured for every case: none is near the 8 GB limit)."""
    ref = ar.attention_fp64(q, k, v)
    err = (out.double() - ref).abs().max().item()
    mag = ref.abs().max().item()
    e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
    bar = max(2.0 * e, ar.half_ulp(dtype, mag))
    _note(f"fp64[{tag}]: packed {err:.3e}  eager E {e:.3e}  |ref|max {mag:.3f}  bar {bar:.3e}")
    assert err <= bar, (tag, err, bar)


# ---------------------------------------------------------------------------------------------------
# 1. float64 parity
# ---------------------------------------------------------------------------------------------------
SHAPES = [(28, 4, 1), (28, 4, 2), (32, 4, 2), (16, 1, 1), (4, 4, 1), (8, 8, 16)]   # R = 7, 14, 16, 16, 1, 16
P0S = [0, 62, 63, 64, 700, 4000]


@pytest.mark.parametrize("kind", ["synth", "peaked", "rising"])
@pytest.mark.parametrize("dtype,shapes,p0s", [(torch.bfloat16, SHAPES, P0S), (torch.float16, SHAPES[:2], [0, 63, 4000])],
                         ids=["bf16", "fp16"])
def test_packed_against_fp64_within_twice_the_eager_error(dtype, shapes, p0s, kind):
    for Hq, Hkv, Lq in shapes:
        for P0 in p0s:
            q, k, v = _inputs(kind, 11, Hq, Hkv, Lq, P0 + Lq, D, dtype)
            _against_fp64(f"{str(dtype)[6:]} {kind} Hq{Hq}/Hkv{Hkv} Lq{Lq} P0 {P0}", q, k, v, _packed(q, k, v), dtype)


@pytest.mark.parametrize("Lq,P0,dtype", [(1, 100351, torch.bfloat16), (2, 100350, torch.bfloat16), (1, 100351, torch.float16)])
def test_packed_against_fp64_over_the_long_cache(Lq, P0, dtype):
    q, k, v = _inputs("synth", 11, 28, 4, Lq, P0 + Lq, D, dtype)
    _against_fp64(f"{str(dtype)[6:]} synth Hq28/Hkv4 Lq{Lq} P0 {P0}", q, k, v, _packed(q, k, v), dtype)


# ---------------------------------------------------------------------------------------------------
# 2. splits above a row's diagonal
# ---------------------------------------------------------------------------------------------------
def test_splits_wholly_above_some_rows_diagonal():
    """(8, 8, 16) with query_offset = Lk - 16: when the last split holds fewer than 16 keys, it lies wholly above the
    diagonal of the first rows, whose partials it must leave empty (m = -inf) for the fold to skip."""
    Hq, Hkv, Lq = 8, 8, 16
    short = []
    for Lk in range(2000, 2401):
        ns, kps = _plan(Hkv, Lk)
        if 0 < Lk - (ns - 1) * kps < 16:
            short.append(Lk)
    assert short, "no length in [2000, 2400] leaves a last split of fewer than 16 keys: the inputs do not test the case"
    for Lk in short[:3]:
        q, k, v = _inputs("synth", 13, Hq, Hkv, Lq, Lk, D, torch.bfloat16)
        _against_fp64(f"bfloat16 synth Hq8/Hkv8 Lq16 Lk {Lk} (last split: {Lk - (_plan(Hkv, Lk)[0] - 1) * _plan(Hkv, Lk)[1]} keys)",
                      q, k, v, _packed(q, k, v, query_offset=Lk - Lq), torch.bfloat16)


# ---------------------------------------------------------------------------------------------------
# 3. causality
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,Lq", [(28, 4, 2), (8, 8, 16)])
def test_rows_do_not_see_later_keys_whatever_they_hold(Hq, Hkv, Lq):
    """K and V rows j > q_offset + i overwritten with NaN: output rows <= i stay bitwise unchanged, for every i."""
    P0 = 700
    Lk = P0 + Lq
    q, k, v = _inputs("synth", 3, Hq, Hkv, Lq, Lk, D, torch.bfloat16)
    a = _packed(q, k, v)
    assert torch.isfinite(a.float()).all()
    for i in range(Lq - 1):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, P0 + i + 1:] = float("nan")
        v2[:, :, P0 + i + 1:] = float("nan")
        b = _packed(q, k2, v2)
        assert torch.equal(_bits(a[:, :i + 1]), _bits(b[:, :i + 1])), i


@pytest.mark.parametrize("Hq,Hkv,Lq,Lk,T", [(28, 4, 2, 702, 703), (28, 4, 2, 702, 900), (8, 8, 16, 716, 722)])
def test_query_offset_restates_a_wider_mask(Hq, Hkv, Lq, Lk, T):
    """query_offset = T - Lq > Lk - Lq, against the masked float64 expression and the bar of the test of this name in
    tests/test_attention_gpu.py."""
    dtype = torch.bfloat16
    q, k, v = _inputs("synth", 4, Hq, Hkv, Lq, Lk, D, dtype)
    out = _packed(q, k, v, query_offset=T - Lq)
    G = Hq // Hkv
    kk, vv = (t[:, :, None].expand(1, Hkv, G, Lk, D).reshape(1, Hq, Lk, D).double() for t in (k, v))
    s = (q.double() @ kk.transpose(2, 3)) * D ** -0.5
    vis = torch.arange(Lk, device=dev())[None, :] <= (T - Lq) + torch.arange(Lq, device=dev())[:, None]
    s.masked_fill_(~vis, -math.inf)
    ref = (torch.softmax(s, -1) @ vv).transpose(1, 2)
    err = (out.double() - ref).abs().max().item()
    bar = 2 * ar.half_ulp(dtype, ref.abs().max().item())
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------
# 4. / 5. views, reproducibility
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,Lq,Lk,dtype", [(28, 4, 2, 4002, torch.bfloat16), (8, 8, 16, 637, torch.float16)])
def test_strided_views_are_read_in_place(Hq, Hkv, Lq, Lk, dtype):
    """q as the transposed view of [1, Lq, Hq*D]; k / v as [:Lk] of larger buffers whose rows beyond Lk are NaN."""
    q, k, v = _inputs("synth", 5, Hq, Hkv, Lq, Lk, D, dtype)
    qv = q.transpose(1, 2).contiguous().view(1, Lq, Hq * D).view(1, Lq, Hq, D).transpose(1, 2)
    kb = torch.full((1, Hkv, Lk + 200, D), float("nan"), dtype=dtype, device=dev())
    vb = torch.full((1, Hkv, Lk + 200, D), float("nan"), dtype=dtype, device=dev())
    kb[:, :, :Lk] = k
    vb[:, :, :Lk] = v
    kv, vv = kb[:, :, :Lk], vb[:, :, :Lk]
    assert qv.stride(1) == D and qv.stride(2) == Hq * D and kv.stride(1) == (Lk + 200) * D and not kv.is_contiguous()
    sums = [int(_bits(t).long().sum()) for t in (qv, kb, vb)]
    a = _packed(q, k, v)
    b = _packed(qv, kv, vv)
    assert not torch.isnan(b.float()).any()
    assert torch.equal(_bits(a), _bits(b))
    assert sums == [int(_bits(t).long().sum()) for t in (qv, kb, vb)]


@pytest.mark.parametrize("Lq,Lk,dtype", [(1, 100352, torch.bfloat16), (2, 4002, torch.float16)])
def test_bitwise_reproducible_and_stream_independent(Lq, Lk, dtype):
    q, k, v = _inputs("synth", 9, 28, 4, Lq, Lk, D, dtype)
    a = _packed(q, k, v)
    b = _packed(q, k, v)
    assert torch.equal(_bits(a), _bits(b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _packed(q, k, v)
    side.synchronize()
    assert torch.equal(_bits(a), _bits(c))


# ---------------------------------------------------------------------------------------------------
# 6. declines fall through to the existing call
# ---------------------------------------------------------------------------------------------------
def _cache_cfg(layers, Hq, Hkv, head_dim, **top):
    kw = {"kvcache_compression": True, "attention_kernel": "hip",
          "kvcache_compression_kwargs": {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    kw.update(top)
    return types.SimpleNamespace(hidden_size=Hq * head_dim, num_hidden_layers=layers, num_attention_heads=Hq,
                                 num_key_value_heads=Hkv, longvideo_kwargs=kw)


@pytest.mark.parametrize("Hq,Hkv,Lq,d,dtype", [(28, 4, 3, 128, torch.bfloat16), (4, 2, 1, 128, torch.float32),
                                               (4, 2, 1, 64, torch.bfloat16)], ids=["21-rows", "fp32", "D64"])
def test_declined_shapes_take_the_existing_call(Hq, Hkv, Lq, d, dtype):
    import retake.longvideo_cache as lc

    q, k, v = _inputs("synth", 1, Hq, Hkv, Lq, 72 + Lq, d, dtype)
    want = lc.chunk_attention(q, k, v)
    route = []
    got = lc.chunk_attention(q, k, v, packed_gqa=True, route=route)
    assert route == ["chunk"] and torch.equal(_bits(got), _bits(want))
    cache = lc.build_kvcache(_cache_cfg(1, Hq, Hkv, d, decode_attention="packed"))
    got = cache.attention(q, k, v)
    assert torch.equal(_bits(got), _bits(want)) and cache.attention_calls == 1 and cache.decode_attention_calls == 0


# ---------------------------------------------------------------------------------------------------
# 7. the fp8 archive
# ---------------------------------------------------------------------------------------------------
def _two_segments(kind, seed, Lq, L8, prefix, dtype, Hq=28, Hkv=4):
    """q, the archive (fp8_ref.quantize) of the first L8 keys, the 16-bit tail [prefix + Lq rows], and the dense
    [fp8_dequantize_rows(archive) | tail]."""
    import retake.longvideo_cache as lc

    q, k, v = _inputs(kind, seed, Hq, Hkv, Lq, L8 + prefix + Lq, D, dtype)
    arch, dense = [], []
    for t in (k, v):
        c, s = fp8_ref.quantize(t[0, :, :L8])
        c, s = c[None].to(dev()), s[None].to(dev())
        arch += [c, s]
        dense.append(torch.cat([lc.fp8_dequantize_rows(c, s, dtype), t[:, :, L8:]], dim=2))
    return q, (arch[0], arch[2], arch[1], arch[3]), k[:, :, L8:], v[:, :, L8:], dense[0], dense[1]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Lq,L8,prefix", [(2, 640, 68), (1, 640, 0)], ids=["70-rows", "1-row"])
def test_fp8kv_bitwise_against_the_packed_16bit_call(Lq, L8, prefix, dtype):
    """L8 % 32 == 0: the two-segment packed call == the packed call over [dequantised archive | 16-bit rows], every bit."""
    q, archive, kt, vt, kd, vd = _two_segments("synth", 21, Lq, L8, prefix, dtype)
    got = _packed(q, kt, vt, archive=archive)
    want = _packed(q, kd, vd)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(_bits(got), _bits(want))
    got = _packed(q, kt, vt, archive=archive, query_offset=L8 + prefix + 3)
    want = _packed(q, kd, vd, query_offset=L8 + prefix + 3)
    assert torch.equal(_bits(got), _bits(want))


def test_fp8kv_bitwise_over_the_long_archive():
    q, archive, kt, vt, kd, vd = _two_segments("synth", 21, 1, 100288, 63, torch.bfloat16)
    assert kt.shape[2] == 64
    assert torch.equal(_bits(_packed(q, kt, vt, archive=archive)), _bits(_packed(q, kd, vd)))


@pytest.mark.parametrize("L8", [624, 59])
def test_fp8kv_unaligned_archive_against_fp64(L8):
    """L8 % 32 != 0: the 16-bit rows start a new key tile, the sums are grouped differently - the 2E bar on the dequantised rows."""
    for Lq, prefix in ((1, 69), (2, 68)):
        for kind in ("synth", "peaked", "rising"):
            q, archive, kt, vt, kd, vd = _two_segments(kind, 11, Lq, L8, prefix, torch.bfloat16)
            _against_fp64(f"fp8kv bfloat16 {kind} Lq{Lq} L8 {L8} + {prefix + Lq} rows", q, kd, vd,
                          _packed(q, kt, vt, archive=archive), torch.bfloat16)


def test_fp8kv_empty_archive_is_the_16bit_packed_call():
    q, k, v = _inputs("synth", 21, 28, 4, 2, 702, D, torch.bfloat16)
    empty = (torch.empty((1, 4, 0, D), dtype=torch.uint8, device=dev()),) * 2 + \
            (torch.empty((1, 4, 0), dtype=torch.float32, device=dev()),) * 2
    assert torch.equal(_bits(_packed(q, k, v, archive=empty)), _bits(_packed(q, k, v)))


# ---------------------------------------------------------------------------------------------------
# 8. through the cache: decode steps and a short text segment after a compressed prefill
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8_e4m3"])
def test_decode_through_the_cache(fp8):
    """The setup of test_attention_through_the_cache_on_the_prologue_route (two layers, two chunks of L 640, after_forward),
    then a text segment of 2 tokens and three single tokens through append_pre_rope, cache.attention on the returned views
    after each: 8 calls, all through the packed kernel, each within the 2E bar of float64 on the same views (the archive
    dequantised); the caches end bitwise where a twin built without the key - and never asked for attention - ends."""
    import retake.longvideo_cache as lc

    Hq, Hkv, L, layers, dtype = 28, 4, 640, 2, torch.bfloat16
    top = {"kv_cache_dtype": "fp8_e4m3"} if fp8 else {}
    caches = [lc.build_kvcache(_cache_cfg(layers, Hq, Hkv, D, decode_attention="packed", **top)),
              lc.build_kvcache(_cache_cfg(layers, Hq, Hkv, D, **top))]
    assert caches[0].decode_attention == "packed" and caches[1].decode_attention is None
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    for with_attention, cache in zip((True, False), caches):
        g = torch.Generator(device=dev()).manual_seed(0)
        draw = lambda n: tuple((1.7 * torch.randn((1, n, h, D), generator=g, device=dev())).to(dtype).transpose(1, 2)   # noqa: E731
                               for h in (Hq, Hkv, Hkv))
        t_next = 10
        for c in range(2):
            cache.keypatches_mask_chunk = torch.from_numpy(np.random.default_rng(c).uniform(size=L) < 0.3).to(dev())
            cache.kvcache_compression = True
            pos = torch.from_numpy(synth.mrope_position_ids(t_next, L // 64, 8, 8, hw0=2)).to(dev())
            t_next += L // 64
            for l in range(layers):
                q, k, v = draw(L)
                assert cache.update_pre_rope(q.clone(), k, v, l, pos.clone(), rot, SEC) is not None
            cache.after_forward()
        cache.keypatches_mask_chunk = None
        cache.kvcache_compression = False
        for n in (2, 1, 1, 1):
            pos = torch.arange(t_next, t_next + n, device=dev()).view(1, 1, n).expand(3, 1, n).contiguous()
            t_next += n
            for l in range(layers):
                q, k, v = draw(n)
                views = cache.append_pre_rope(q.clone(), k, v, l, pos.clone(), rot, SEC)
                assert views is not None
                if not with_attention:
                    continue
                qr, kv, vv = views
                calls = cache.decode_attention_calls
                out = cache.attention(qr, kv, vv, layer_idx=l)
                assert out is not None and out.shape == (1, n, Hq, D) and cache.decode_attention_calls == calls + 1
                kd, vd = kv, vv
                if fp8:
                    assert cache.archive_len(l) > 0
                    k8, v8, ks, vs = cache.archive(l)
                    kd = torch.cat([lc.fp8_dequantize_rows(k8, ks, dtype), kv], dim=2)
                    vd = torch.cat([lc.fp8_dequantize_rows(v8, vs, dtype), vv], dim=2)
                _against_fp64(f"cache route{' fp8' if fp8 else ''} Lq{n} layer {l} keys {kd.shape[2]}", qr, kd, vd, out, dtype)
            cache.after_forward()
    a, b = caches
    assert a.decode_attention_calls == 8 and a.attention_calls == 8 and b.attention_calls == 0
    for l in range(layers):
        assert torch.equal(a.key_cache[l], b.key_cache[l]) and torch.equal(a.value_cache[l], b.value_cache[l])
        assert torch.equal(a.position_cache[l], b.position_cache[l])
        if fp8:
            for x, y in zip(a.archive(l), b.archive(l)):
                assert torch.equal(x, y)
    fp = a.memory_footprint()["attention_workspace"]
    assert fp > 0 and fp == sum(t.numel() for t in a._attn_ws.values())
    before = torch.cuda.memory_allocated()
    a.attention(qr, kv, vv, layer_idx=layers - 1)
    assert a.memory_footprint()["attention_workspace"] == fp and torch.cuda.memory_allocated() <= before + Hq * D * 2 + 1024

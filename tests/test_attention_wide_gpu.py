"""The wide packed attention (rtk_attention_decode_wide / _wide_fp8kv / _wide_shared, chunk_attention(packed_wide=True),
multi_token_attention="packed": 16 < (Hq / Hkv) * Lq <= 64 packed rows) on the GPU: float64 truth under the project's "2E"
rule, splits above a row's diagonal, causality against NaN rows, views, reproducibility, the identities the header
states, and the product route through the cache - the verification step of assisted generation with `crop`.
Every case checks that the wide kernel really ran: a silent fall-back to the chunk kernels would pass the numbers."""
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
BF16, F16 = torch.bfloat16, torch.float16


def dev():
    return torch.device("cuda:0")


def _note(line: str):
    """Print a measured figure; also append it to $RETAKE_WIDE_ATTENTION_STATS when set
    (profiles/wide_decode_parity_stats.txt)."""
    print(line, flush=True)
    path = os.environ.get("RETAKE_WIDE_ATTENTION_STATS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _wide(q, k, v, **kw):
    """chunk_attention through the wide packed kernel - asserted, not assumed."""
    import retake.longvideo_cache as lc

    route = []
    out = lc.chunk_attention(q, k, v, packed_gqa=True, packed_wide=True, route=route, **kw)
    assert route == ["wide"], f"the wide kernel did not take this call: {route}"
    assert out.shape == (1, q.shape[2], q.shape[1], q.shape[3]) and out.dtype == q.dtype and out.is_contiguous()
    return out


def _inputs(kind, seed, Hq, Hkv, Lq, Lk, dtype):
    """attention_ref.make_inputs with k and v laid out alike (a broadcast one-row k otherwise keeps strides of its own)."""
    q, k, v = ar.make_inputs(kind, seed, Hq, Hkv, Lq, Lk, D, dtype, dev())
    return q, k.clone(memory_format=torch.contiguous_format), v.clone(memory_format=torch.contiguous_format)


def _plan(Hkv, K):
    """The rule of include/retake_hip.h (rtk_attention_decode), restated: (nsplit, keys per split)."""
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    n0 = max(1, min(ceil(512, Hkv), ceil(K, 128)))
    kps = 128 * ceil(ceil(K, n0), 128)
    return ceil(K, kps), kps


def _against_fp64(tag, q, k, v, out, dtype, also=None):
    """The "2E" rule of tests/test_attention_decode_gpu.py::_against_fp64: within max(2 E, half an output ulp) of float64,
    E the eager expression's error on the same tensors.  also: a second output held to the same bar (the twin's)."""
    ref = ar.attention_fp64(q, k, v)
    err = (out.double() - ref).abs().max().item()
    mag = ref.abs().max().item()
    e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
    bar = max(2.0 * e, ar.half_ulp(dtype, mag))
    line = f"fp64[{tag}]: wide {err:.3e}  eager E {e:.3e}  |ref|max {mag:.3f}  bar {bar:.3e}"
    if also is not None:
        twin = (also.double() - ref).abs().max().item()
        line += f"  twin {twin:.3e}"
    _note(line)
    assert err <= bar, (tag, err, bar)
    if also is not None:
        assert twin <= bar, (tag, "twin", twin, bar)


# ---------------------------------------------------------------------------------------------------
# 1. float64 parity
# ---------------------------------------------------------------------------------------------------
# R = 21 (NCG 2), 35 (NCG 3), 63 (NCG 4, one idle column), 64 (full), 17 (G = 1, one column in the second group), 33 (the
# diagonal leaves the first tile), 64 (the diagonal over two tiles, two waves), 64 (G = 16)
SHAPES = [(28, 4, 3), (28, 4, 5), (28, 4, 9), (32, 4, 8), (8, 8, 17), (4, 4, 33), (2, 2, 64), (16, 1, 4)]
P0S = [0, 31, 62, 63, 64, 700, 4000]


@pytest.mark.parametrize("kind", ["synth", "peaked", "rising"])
@pytest.mark.parametrize("dtype,shapes", [(BF16, SHAPES), (F16, SHAPES[:2])], ids=["bf16", "fp16"])
def test_wide_against_fp64_within_twice_the_eager_error(dtype, shapes, kind):
    for Hq, Hkv, Lq in shapes:
        for P0 in P0S:
            q, k, v = _inputs(kind, 11, Hq, Hkv, Lq, P0 + Lq, dtype)
            _against_fp64(f"{str(dtype)[6:]} {kind} Hq{Hq}/Hkv{Hkv} Lq{Lq} P0 {P0}", q, k, v, _wide(q, k, v), dtype)


def test_wide_against_fp64_over_the_long_cache():
    Lq, Lk = 6, 100352
    q, k, v = _inputs("synth", 11, 28, 4, Lq, Lk, BF16)
    _against_fp64(f"bfloat16 synth Hq28/Hkv4 Lq{Lq} Lk {Lk}", q, k, v, _wide(q, k, v), BF16)


# ---------------------------------------------------------------------------------------------------
# 2. splits above a row's diagonal
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,Lq", [(4, 4, 33), (2, 2, 64)])
def test_splits_wholly_above_some_rows_diagonal(Hq, Hkv, Lq):
    """query_offset = Lk - Lq: when the last split holds fewer than Lq keys, it lies wholly above the diagonal of the first
    rows, whose partials it must leave empty (m = -inf) for the fold to skip."""
    short = []
    for Lk in range(2000, 2401):
        ns, kps = _plan(Hkv, Lk)
        if 0 < Lk - (ns - 1) * kps < Lq:
            short.append(Lk)
    assert short, f"no length in [2000, 2400] leaves a last split of fewer than {Lq} keys: the inputs do not test the case"
    for Lk in (short[0], short[len(short) // 2], short[-1]):
        q, k, v = _inputs("synth", 13, Hq, Hkv, Lq, Lk, BF16)
        ns, kps = _plan(Hkv, Lk)
        _against_fp64(f"bfloat16 synth Hq{Hq}/Hkv{Hkv} Lq{Lq} Lk {Lk} (last split: {Lk - (ns - 1) * kps} keys)",
                      q, k, v, _wide(q, k, v, query_offset=Lk - Lq), BF16)


# ---------------------------------------------------------------------------------------------------
# 3. causality
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,Lq", [(28, 4, 5), (2, 2, 64)])
def test_rows_do_not_see_later_keys_whatever_they_hold(Hq, Hkv, Lq):
    """K and V rows j > q_offset + i overwritten with NaN: output rows <= i stay bitwise unchanged, for every i."""
    P0 = 700
    Lk = P0 + Lq
    q, k, v = _inputs("synth", 3, Hq, Hkv, Lq, Lk, BF16)
    a = _wide(q, k, v)
    assert torch.isfinite(a.float()).all()
    for i in range(Lq - 1):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, P0 + i + 1:] = float("nan")
        v2[:, :, P0 + i + 1:] = float("nan")
        b = _wide(q, k2, v2)
        assert torch.equal(_bits(a[:, :i + 1]), _bits(b[:, :i + 1])), i


@pytest.mark.parametrize("Hq,Hkv,Lq,Lk,T", [(28, 4, 5, 705, 706), (28, 4, 5, 705, 900), (2, 2, 64, 764, 790)])
def test_query_offset_restates_a_wider_mask(Hq, Hkv, Lq, Lk, T):
    """query_offset = T - Lq > Lk - Lq, against the masked float64 expression and the bar of the test of this name in
    tests/test_attention_decode_gpu.py."""
    q, k, v = _inputs("synth", 4, Hq, Hkv, Lq, Lk, BF16)
    out = _wide(q, k, v, query_offset=T - Lq)
    G = Hq // Hkv
    kk, vv = (t[:, :, None].expand(1, Hkv, G, Lk, D).reshape(1, Hq, Lk, D).double() for t in (k, v))
    s = (q.double() @ kk.transpose(2, 3)) * D ** -0.5
    vis = torch.arange(Lk, device=dev())[None, :] <= (T - Lq) + torch.arange(Lq, device=dev())[:, None]
    s.masked_fill_(~vis, -math.inf)
    ref = (torch.softmax(s, -1) @ vv).transpose(1, 2)
    err = (out.double() - ref).abs().max().item()
    bar = 2 * ar.half_ulp(BF16, ref.abs().max().item())
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------
# 4. / 5. views, reproducibility
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,Lq,Lk,dtype", [(28, 4, 6, 4006, BF16), (2, 2, 64, 637, F16)])
def test_strided_views_are_read_in_place(Hq, Hkv, Lq, Lk, dtype):
    """q as the transposed view of [1, Lq, Hq*D]; k / v as [:Lk] of larger buffers whose rows beyond Lk are NaN."""
    q, k, v = _inputs("synth", 5, Hq, Hkv, Lq, Lk, dtype)
    qv = q.transpose(1, 2).contiguous().view(1, Lq, Hq * D).view(1, Lq, Hq, D).transpose(1, 2)
    kb = torch.full((1, Hkv, Lk + 200, D), float("nan"), dtype=dtype, device=dev())
    vb = torch.full((1, Hkv, Lk + 200, D), float("nan"), dtype=dtype, device=dev())
    kb[:, :, :Lk] = k
    vb[:, :, :Lk] = v
    kv, vv = kb[:, :, :Lk], vb[:, :, :Lk]
    assert qv.stride(1) == D and qv.stride(2) == Hq * D and kv.stride(1) == (Lk + 200) * D and not kv.is_contiguous()
    sums = [int(t.view(torch.int16).long().sum()) for t in (qv, kb, vb)]
    a = _wide(q, k, v)
    b = _wide(qv, kv, vv)
    assert not torch.isnan(b.float()).any()
    assert torch.equal(_bits(a), _bits(b))
    assert sums == [int(t.view(torch.int16).long().sum()) for t in (qv, kb, vb)]


@pytest.mark.parametrize("Lq,Lk,dtype", [(6, 100352, BF16), (9, 4009, F16)])
def test_bitwise_reproducible_and_stream_independent(Lq, Lk, dtype):
    q, k, v = _inputs("synth", 9, 28, 4, Lq, Lk, dtype)
    a = _wide(q, k, v)
    b = _wide(q, k, v)
    assert torch.equal(_bits(a), _bits(b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _wide(q, k, v)
    side.synchronize()
    assert torch.equal(_bits(a), _bits(c))


# ---------------------------------------------------------------------------------------------------
# 6. the identities of the header
# ---------------------------------------------------------------------------------------------------
def test_at_most_16_rows_through_the_wide_entry_point_is_the_packed_call():
    import retake.longvideo_cache as lc

    q, k, v = _inputs("synth", 21, 28, 4, 2, 702, BF16)
    route = []
    got = lc.chunk_attention(q, k, v, packed_wide=True, route=route)      # rtk_attention_decode_wide alone
    assert route == ["wide"]
    route = []
    want = lc.chunk_attention(q, k, v, packed_gqa=True, route=route)      # rtk_attention_decode
    assert route == ["packed"]
    assert torch.isfinite(want.float()).all() and torch.equal(_bits(got), _bits(want))


def _segments(kind, seed, Hq, Hkv, Lq, Lk, Ls, L8, dtype):
    """One sequence of L8 + Ls + Lk keys cut three ways: q, the archive (fp8_ref.quantize) of the first L8 rows or None, the
    next Ls rows as views of a NaN-padded buffer of their own or None, the own rows, and the dense [dequantised archive |
    shared | own] rows."""
    import retake.longvideo_cache as lc

    q, k, v = _inputs(kind, seed, Hq, Hkv, Lq, L8 + Ls + Lk, dtype)
    archive, dense = None, [k, v]
    if L8:
        arch, dense = [], []
        for t in (k, v):
            c, s = fp8_ref.quantize(t[0, :, :L8])
            c, s = c[None].to(dev()), s[None].to(dev())
            arch += [c, s]
            dense.append(torch.cat([lc.fp8_dequantize_rows(c, s, dtype), t[:, :, L8:]], dim=2))
        archive = (arch[0], arch[2], arch[1], arch[3])
    shared = None
    if Ls:
        shared = []
        for t in (k, v):
            buf = torch.full((1, Hkv, Ls + 7, D), float("nan"), dtype=dtype, device=dev())   # rows past Ls must never be read
            buf[:, :, :Ls].copy_(t[:, :, L8:L8 + Ls])
            shared.append(buf[:, :, :Ls])
        shared = tuple(shared)
    return q, archive, shared, (k[:, :, L8 + Ls:], v[:, :, L8 + Ls:]), dense


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Hq,Hkv,Lq", [(28, 4, 6), (2, 2, 64)])
def test_aligned_segments_bitwise_against_the_plain_wide_call(Hq, Hkv, Lq, dtype):
    """L8 = 64, Ls = 96 (whole key tiles): the segmented call == the plain wide call over [dequantised archive | shared | own]."""
    q, archive, shared, own, dense = _segments("synth", 21, Hq, Hkv, Lq, 39 + Lq, 96, 64, dtype)
    want = _wide(q, dense[0], dense[1])
    assert torch.isfinite(want.float()).all()
    assert torch.equal(_bits(_wide(q, own[0], own[1], archive=archive, shared=shared)), _bits(want))
    off = 64 + 96 + 39 + 3
    assert torch.equal(_bits(_wide(q, own[0], own[1], archive=archive, shared=shared, query_offset=off)),
                       _bits(_wide(q, dense[0], dense[1], query_offset=off)))


@pytest.mark.parametrize("L8,Ls", [(70, 45), (70, 0), (0, 45)])
def test_unaligned_segments_against_fp64(L8, Ls):
    """A segment that ends inside a key tile: the next one starts a new tile, the sums are grouped differently - the 2E bar
    on the dequantised rows."""
    for Hq, Hkv, Lq in ((28, 4, 6), (28, 4, 9), (2, 2, 64)):
        for kind in ("synth", "peaked", "rising"):
            q, archive, shared, own, dense = _segments(kind, 11, Hq, Hkv, Lq, 37 + Lq, Ls, L8, BF16)
            _against_fp64(f"segments bfloat16 {kind} Hq{Hq}/Hkv{Hkv} Lq{Lq} L8 {L8} Ls {Ls} + {37 + Lq} rows", q, dense[0], dense[1],
                          _wide(q, own[0], own[1], archive=archive, shared=shared), BF16)


# ---------------------------------------------------------------------------------------------------
# 7. through the cache: the verification steps of assisted generation after a compressed prefill
# ---------------------------------------------------------------------------------------------------
def _cache_cfg(layers, Hq, Hkv, **top):
    kw = {"kvcache_compression": True, "attention_kernel": "hip", "decode_attention": "packed",
          "kvcache_compression_kwargs": {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    kw.update(top)
    return types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=layers, num_attention_heads=Hq,
                                 num_key_value_heads=Hkv, longvideo_kwargs=kw)


Hq_, Hkv_, L_, LAYERS = 28, 4, 640, 2


def _session(mode, wide, steps):
    """A 2-layer cache after two compressed chunks (the setup of tests/test_attention_decode_gpu.py::
    test_decode_through_the_cache), then `steps` through append_pre_rope + attention on the cache itself, or - mode "fork" -
    on a branch at `video_end`.  A step is n (new rows), ("crop", r) (give up the last r rows) or (n, keep): n rows drawn
    as for a step of n, of which only the first `keep` are ever shown to the cache.  Returns the cache that took the steps
    and, per attention call, (n, layer, q, dense keys, dense values, output, route counters after the call)."""
    import retake.longvideo_cache as lc

    top = {"kv_cache_dtype": "fp8_e4m3"} if mode == "fp8_e4m3" else {}
    if wide:
        top["multi_token_attention"] = "packed"
    cache = lc.build_kvcache(_cache_cfg(LAYERS, Hq_, Hkv_, **top))
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    g = torch.Generator(device=dev()).manual_seed(0)
    draw = lambda n: tuple((1.7 * torch.randn((1, n, h, D), generator=g, device=dev())).to(BF16).transpose(1, 2)   # noqa: E731
                           for h in (Hq_, Hkv_, Hkv_))
    t_next = 10
    for c in range(2):
        cache.keypatches_mask_chunk = torch.from_numpy(np.random.default_rng(c).uniform(size=L_) < 0.3).to(dev())
        cache.kvcache_compression = True
        pos = torch.from_numpy(synth.mrope_position_ids(t_next, L_ // 64, 8, 8, hw0=2)).to(dev())
        t_next += L_ // 64
        for l in range(LAYERS):
            q, k, v = draw(L_)
            assert cache.update_pre_rope(q.clone(), k, v, l, pos.clone(), rot, SEC) is not None
        cache.after_forward()
    cache.keypatches_mask_chunk = None
    cache.kvcache_compression = False
    if mode == "fork":
        cache = cache.fork(cache.video_end)
        assert cache.multi_token_attention == ("packed" if wide else None) and cache.decode_attention == "packed"
    calls = []
    for step in steps:
        if isinstance(step, tuple) and step[0] == "crop":
            cache.crop(-step[1])
            t_next -= step[1]
            continue
        n, keep = step if isinstance(step, tuple) else (step, step)
        pos = torch.arange(t_next, t_next + keep, device=dev()).view(1, 1, keep).expand(3, 1, keep).contiguous()
        t_next += keep
        for l in range(LAYERS):
            q, k, v = (t[:, :, :keep] for t in draw(n))
            views = cache.append_pre_rope(q.clone(), k, v, l, pos.clone(), rot, SEC)
            assert views is not None
            qr, kv, vv = views
            out = cache.attention(qr, kv, vv, layer_idx=l)
            assert out is not None and out.shape == (1, keep, Hq_, D)
            kd, vd = [kv], [vv]
            if cache.shared_len(l):
                ks, vs = cache.shared(l)
                kd, vd = [ks] + kd, [vs] + vd
            if cache.archive_len(l):
                k8, v8, ks8, vs8 = cache.archive(l)
                kd, vd = [lc.fp8_dequantize_rows(k8, ks8, BF16)] + kd, [lc.fp8_dequantize_rows(v8, vs8, BF16)] + vd
            calls.append((keep, l, qr.clone(), torch.cat(kd, dim=2), torch.cat(vd, dim=2), out,
                          (cache.attention_calls, cache.decode_attention_calls, cache.wide_attention_calls)))
        cache.after_forward()
    return cache, calls


@pytest.mark.parametrize("mode", ["16bit", "fp8_e4m3", "fork"])
def test_verification_steps_through_the_cache(mode):
    """n = 1, 2, 6, 9, 10 new rows at Hq 28 / Hkv 4: 6 and 9 take the wide kernel (42 and 63 packed rows), 1 and 2 the packed
    one, 10 (70 rows) the chunk kernel.  Against a twin built without the key: the same bits where the route is the same,
    and where it is not, both inside the float64 bar.  Then two of the ten rows are given up (`crop`, a rejected draft) and
    a 6-row step follows: bitwise what a cache that never saw the two rows computes."""
    steps = [1, 2, 6, 9, 10]
    cache, calls = _session(mode, True, steps + [("crop", 2), 6])
    twin, tcalls = _session(mode, False, steps)
    assert cache.multi_token_attention == "packed" and twin.multi_token_attention is None
    if mode == "fp8_e4m3":
        assert cache.archive_len(0) > 0
    if mode == "fork":
        assert cache.shared_len(0) > 0
    assert twin.wide_attention_calls == 0 and twin.decode_attention_calls == 2 * LAYERS and twin.attention_calls == 5 * LAYERS
    assert [c[0] for c in calls] == [n for n in steps + [6] for _ in range(LAYERS)]
    before = (0, 0, 0)
    for (n, l, q, kd, vd, out, counts), (tn, tl, tq, tkd, tvd, tout, _) in zip(calls, tcalls):
        assert (n, l) == (tn, tl) and torch.equal(q, tq) and torch.equal(kd, tkd) and torch.equal(vd, tvd)
        took = tuple(a - b for a, b in zip(counts, before))
        before = counts
        assert took == {1: (1, 1, 0), 2: (1, 1, 0), 6: (1, 0, 1), 9: (1, 0, 1), 10: (1, 0, 0)}[n], (n, l, took)
        if n in (6, 9):
            _against_fp64(f"cache route {mode} Lq{n} layer {l} keys {kd.shape[2]}", q, kd, vd, out, BF16, also=tout)
        else:
            assert torch.equal(_bits(out), _bits(tout)), (n, l)
    assert cache.wide_attention_calls == 3 * LAYERS and cache.decode_attention_calls == 2 * LAYERS
    # the rejected draft: a cache that was shown only the first 8 of the 10 rows
    clean, ccalls = _session(mode, True, steps[:-1] + [(10, 8), 6])
    for (n, l, q, kd, vd, out, _), (cn, cl, cq, ckd, cvd, cout, _) in zip(calls[-LAYERS:], ccalls[-LAYERS:]):
        assert n == cn == 6 and l == cl
        assert torch.equal(q, cq) and torch.equal(kd, ckd) and torch.equal(vd, cvd), l
        assert torch.isfinite(out.float()).all() and torch.equal(_bits(out), _bits(cout)), l
    assert clean.wide_attention_calls == 4 * LAYERS    # 6, 9, the 8 rows (56 packed rows) and the last 6
    assert cache.get_seq_length() == clean.get_seq_length()


@pytest.mark.parametrize("Hq,Hkv,Lq", [(8, 8, 17), (8, 4, 9), (16, 1, 4)], ids=["G1", "G2", "G16"])
def test_geometries_that_did_not_measure_faster_keep_the_chunk_kernel(Hq, Hkv, Lq):
    """Inside the wide kernel's envelope, outside the dispatcher's (native_attention.wide_dispatch): the cache takes the
    chunk kernel, bit for bit what it takes without the key; chunk_attention(packed_wide=True) still reaches the wide one."""
    import retake.longvideo_cache as lc

    q, k, v = _inputs("synth", 1, Hq, Hkv, Lq, 700 + Lq, BF16)
    want = lc.chunk_attention(q, k, v)
    cache = lc.build_kvcache(_cache_cfg(1, Hq, Hkv, multi_token_attention="packed"))
    got = cache.attention(q, k, v)
    assert torch.equal(_bits(got), _bits(want))
    assert (cache.attention_calls, cache.decode_attention_calls, cache.wide_attention_calls) == (1, 0, 0)
    _against_fp64(f"outside the dispatcher Hq{Hq}/Hkv{Hkv} Lq{Lq}", q, k, v, _wide(q, k, v), BF16)

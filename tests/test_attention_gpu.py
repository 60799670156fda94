"""The native chunk attention (rtk_attention_forward, PivotKVCache.attention, attention_kernel="hip") on the GPU: the
reference's recorded layer outputs, float64 truth with the reference's own error as the yardstick, views, causality,
reproducibility, the product route through the cache, memory, and clean declines."""
import math
import os
import types

import numpy as np
import pytest
import torch

import attention_ref as ar
import golden_util as gu
import synth

pytestmark = pytest.mark.gpu

SEC = [16, 24, 24]
A = synth.YARN_FACTOR4_ATTENTION_SCALING


def dev():
    return torch.device("cuda:0")


def _note(line: str):
    """Print a measured figure; also append it to $RETAKE_ATTENTION_STATS when set (profiles/attention_parity_stats.txt)."""
    print(line, flush=True)
    path = os.environ.get("RETAKE_ATTENTION_STATS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---------------------------------------------------------------------------------------------------
# 1. the reference's recorded layer outputs, through the four patches with the switch on
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["qwen2vl", "qwen2vl_sdpa", "qwen2vl_fa2", "qwen2vl_ratio1", "llava", "llava_ratio1"])
def test_patches_with_native_attention_match_reference(model):
    """The loop of test_attention_patch_with_pivotkv_cache_matches_reference (tests/test_hip_parity.py) with
    attention_kernel="hip" and NO stand-in for `_flash_attention_forward`: two patched layers sharing one cache through
    text(5) -> video(32) -> video(32) -> text(3) -> decode(1), fp32, head_dim 16 (the general kernel).  Same bars - layer
    output < 2e-5 of max(1, |ref|max), ids and final caches as recorded - and every (step, layer) must have gone through the
    native entry point.  With compression_ratio 0.5 the recorded 4-D masks are wider than the compressed keys: the eager,
    SDPA and LLaVA references see keys j <= (T - Lq) + i there, the flash-attn reference j <= (Lk - Lq) + i."""
    import glue_stubs as gs
    import retake.llava_onevision as lo
    import retake.longvideo_cache as lc
    import retake.qwen2_vl as q

    g = gu.load("glue_attention_" + model)
    ratio = 1 if "ratio1" in model else 0.5
    assert float(g["ratio"]) == ratio
    fa2 = bool(g["fa2"])
    llava = bool(g["llava"])
    S = float(g["attention_scaling"])
    layers = [gs.StubAttention(l, 64, 4, 2, None if llava else (2, 3, 3), S,
                               weights=[g[f"w{l}_{i}"] for i in range(7)]).to_device(dev()).eval() for l in range(2)]
    llm = types.SimpleNamespace(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2)
    kw = {"kvcache_compression": True, "attention_kernel": "hip",
          "kvcache_compression_kwargs": {"compression_ratio": ratio, "compression_method": "pivotkv",
                                         "pos_embed_reforge": True}}
    if llava:
        cfg = types.SimpleNamespace(text_config=llm, longvideo_kwargs=kw)
    else:
        llm.longvideo_kwargs = kw
        cfg = llm
    cache = lc.build_kvcache(cfg)
    assert cache.attention_kernel == "hip"
    total = 0
    worst = 0.0
    calls = 0
    for si in range(int(g["n_steps"])):
        kind = str(g[f"s{si}_kind"])
        x = torch.from_numpy(g[f"s{si}_x"]).to(dev())
        n = x.shape[1]
        total += n
        mask4 = torch.from_numpy(g[f"s{si}_mask4"]).to(dev())
        cp = torch.arange(total - n, total, device=dev())
        cache.kvcache_compression = kind == "video"
        cache.keypatches_mask_chunk = torch.from_numpy(g[f"s{si}_kpmask"]).to(dev()) if kind == "video" else None
        pos_shared = torch.from_numpy(g[f"s{si}_pos_in"]).to(dev())
        for l, att in enumerate(layers):
            with torch.no_grad():
                if llava:
                    o = lo.retake_Qwen2Attention_forward(att, x, None, mask4, cache, cp, position_ids=pos_shared)
                elif fa2:
                    o = q.retake_Qwen2VLFlashAttention2_forward(att, x, None, pos_shared, cache, False, True, cp)
                elif "sdpa" in model:
                    o = q.retake_Qwen2VLSdpaAttention_forward(att, x, mask4, pos_shared, cache, False, True, cp)
                else:
                    o = q.retake_Qwen2VLAttention_forward(att, x, mask4, pos_shared, cache, False, True, cp)
            calls += 1
            assert cache.attention_calls == calls, f"step {si} layer {l} did not take the native entry point"
            ref = g[f"s{si}_l{l}_out"]
            err = np.abs(o[0].cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())
            worst = max(worst, err)
            assert err < 2e-5, (si, l, err)
            np.testing.assert_array_equal(pos_shared.cpu().numpy(), g[f"s{si}_l{l}_pos_after"])
        cache.after_forward()
    _note(f"patches[{model}]: worst layer-output error {worst:.3e} of max(1, |ref|max) over {calls} native calls (bar 2e-5)")
    for l in range(2):
        assert np.abs(cache.key_cache[l].cpu().numpy() - g[f"cache_k{l}"]).max() <= 1e-5
        assert np.abs(cache.value_cache[l].cpu().numpy() - g[f"cache_v{l}"]).max() <= 1e-5
        np.testing.assert_array_equal(cache.position_cache[l].cpu().numpy(), g[f"cache_pos{l}"])
    assert cache.num_evicted_tokens == g["num_evicted"].tolist()


# ---------------------------------------------------------------------------------------------------
# 2. float64 truth, the reference's own error as the yardstick
# ---------------------------------------------------------------------------------------------------
SHAPES = [  # (Hq, Hkv, Lq, P0)
    (28, 4, 2304, 0), (28, 4, 2304, 3456), (28, 4, 2304, 1153), (28, 4, 6272, 6272), (28, 4, 600, 37), (28, 4, 32, 5),
    (28, 4, 5, 0), (28, 4, 3, 72), (28, 4, 1, 4000), (28, 4, 1, 100351), (4, 2, 600, 37), (8, 8, 32, 5),
]
SUBSET_16 = [(28, 4, 2304, 1153), (28, 4, 600, 37), (28, 4, 5, 0), (28, 4, 1, 100351)]
SUBSET_32 = [(28, 4, 600, 37), (28, 4, 32, 5), (28, 4, 3, 72), (28, 4, 1, 4000), (28, 4, 1, 100351)]
EAGER_LIMIT = 8e9   # bytes of the eager expression's fp32 logits above which its error is not measured


def _errors(shape, kind, dtype, D=128):
    import retake.longvideo_cache as lc

    Hq, Hkv, Lq, P0 = shape
    Lk = P0 + Lq
    q, k, v = ar.make_inputs(kind, 11, Hq, Hkv, Lq, Lk, D, dtype, dev())
    out = lc.chunk_attention(q, k, v)
    assert out is not None and out.shape == (1, Lq, Hq, D) and out.dtype == dtype and out.is_contiguous()
    ref = ar.attention_fp64(q, k, v)
    err = (out.double() - ref).abs().max().item()
    mag = ref.abs().max().item()
    e = None
    if dtype != torch.float32 and ar.eager_bytes(Hq, Lq, Lk) <= EAGER_LIMIT:
        e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
    del q, k, v, out, ref
    torch.cuda.empty_cache()
    return err, e, mag


@pytest.mark.parametrize("dtype,shapes,kinds", [
    (torch.bfloat16, SHAPES, ("synth", "peaked", "rising")),
    (torch.float16, SUBSET_16, ("synth", "peaked", "rising")),
], ids=["bf16", "fp16"])
def test_fast_path_against_fp64_within_twice_the_eager_error(dtype, shapes, kinds):
    """DESIGN §2's "2E" rule: on the same 16-bit inputs, E = max abs error of the reference's eager expression
    (qwen2_vl.py:88-117) against float64; the native result must be within max(2 E, half an ulp of the output dtype at the
    output's magnitude).  A case whose eager logits exceed 8 GB takes the largest E of the other cases of its dtype and
    input set (at most 2 cases may).  Inputs: synth.qkv_chunk, q x8 (peaked rows), and keys ordered so that each row's
    largest logit is its last visible key (the running maximum moves at every tile)."""
    lost = 0
    for kind in kinds:
        rows = [(s,) + _errors(s, kind, dtype) for s in shapes]
        known = [e for _, _, e, _ in rows if e is not None]
        assert known
        for s, err, e, mag in rows:
            borrowed = e is None
            if borrowed:
                e = max(known)
            bar = max(2.0 * e, ar.half_ulp(dtype, mag))
            _note(f"fp64[{str(dtype)[6:]} {kind} Hq{s[0]}/Hkv{s[1]} Lq{s[2]} P0 {s[3]}]: native {err:.3e}  eager E {e:.3e}"
                  f"{' (borrowed)' if borrowed else ''}  |ref|max {mag:.3f}  bar {bar:.3e}")
            assert err <= bar, (kind, s, err, bar)
        lost = max(lost, sum(1 for _, _, e, _ in rows if e is None))
    assert lost <= 2


@pytest.mark.parametrize("D", [128, 16])
def test_general_path_fp32_against_fp64(D):
    """fp32 (the parity dtype) runs the general kernel: <= 1e-5 of max(1, |ref|max) against float64."""
    for kind in ("synth", "rising"):
        for s in SUBSET_32 if D == 128 else [(4, 2, 32, 5), (4, 2, 5, 0), (4, 2, 3, 72), (4, 2, 1, 73)]:
            err, _, mag = _errors(s, kind, torch.float32, D)
            _note(f"fp64[float32 {kind} D{D} Hq{s[0]}/Hkv{s[1]} Lq{s[2]} P0 {s[3]}]: native {err:.3e}  |ref|max {mag:.3f}"
                  f"  bar {1e-5 * max(1.0, mag):.3e}")
            assert err <= 1e-5 * max(1.0, mag), (kind, s, err)


def test_general_path_16bit_small_heads_against_fp64():
    """16-bit payloads at a head_dim the fast path does not take (64, 80, 256): the general kernel, same 2E bar."""
    for dtype in (torch.bfloat16, torch.float16):
        for D in (64, 80, 256):
            err, e, mag = _errors((4, 2, 600, 37), "synth", dtype, D)
            bar = max(2.0 * e, ar.half_ulp(dtype, mag))
            _note(f"fp64[{str(dtype)[6:]} synth D{D} Hq4/Hkv2 Lq600 P0 37]: native {err:.3e}  eager E {e:.3e}  bar {bar:.3e}")
            assert err <= bar


# ---------------------------------------------------------------------------------------------------
# 3. - 5. views, causality, reproducibility
# ---------------------------------------------------------------------------------------------------
def _viewed(Hq, Hkv, Lq, Lk, D, dtype, cap_extra=200, seed=5):
    """q as the transposed view of [1, Lq, Hq*D]; k / v as [:Lk] of [1, Hkv, cap, D] buffers whose rows [Lk:cap] are NaN."""
    q, k, v = ar.make_inputs("synth", seed, Hq, Hkv, Lq, Lk, D, dtype, dev())
    qv = q.transpose(1, 2).contiguous().view(1, Lq, Hq * D).view(1, Lq, Hq, D).transpose(1, 2)
    cap = Lk + cap_extra
    kb = torch.full((1, Hkv, cap, D), float("nan"), dtype=dtype, device=dev())
    vb = torch.full((1, Hkv, cap, D), float("nan"), dtype=dtype, device=dev())
    kb[:, :, :Lk] = k
    vb[:, :, :Lk] = v
    return (q, k, v), (qv, kb[:, :, :Lk], vb[:, :, :Lk]), (kb, vb)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("case", [(28, 4, 600, 637, 128, torch.bfloat16), (28, 4, 2304, 3457, 128, torch.float16),
                                  (28, 4, 3, 5000, 128, torch.bfloat16), (4, 2, 32, 37, 16, torch.float32),
                                  (4, 2, 1, 6000, 16, torch.float32)])
def test_views_are_read_in_place(case):
    import retake.longvideo_cache as lc

    Hq, Hkv, Lq, Lk, D, dtype = case
    (q, k, v), (qv, kv, vv), (kb, vb) = _viewed(Hq, Hkv, Lq, Lk, D, dtype)
    assert qv.stride(1) == D and qv.stride(2) == Hq * D and kv.stride(1) == kb.shape[2] * D and not kv.is_contiguous()
    sums = [int(_bits(t).long().sum()) for t in (qv, kb, vb)]
    a = lc.chunk_attention(q, k, v)
    b = lc.chunk_attention(qv, kv, vv)
    assert not torch.isnan(b.float()).any()
    assert torch.equal(_bits(a), _bits(b))
    assert sums == [int(_bits(t).long().sum()) for t in (qv, kb, vb)]


@pytest.mark.parametrize("case", [(28, 4, 600, 637, 128, torch.bfloat16), (28, 4, 130, 4000, 128, torch.float16),
                                  (28, 4, 20, 9000, 128, torch.bfloat16), (4, 2, 32, 69, 16, torch.float32)])
def test_rows_do_not_see_later_keys(case):
    """Changing key / value rows j > (Lk - Lq) + i leaves output row i bitwise unchanged: perturb the last 7 keys and
    values, compare every row but the last 7."""
    import retake.longvideo_cache as lc

    Hq, Hkv, Lq, Lk, D, dtype = case
    q, k, v = ar.make_inputs("synth", 3, Hq, Hkv, Lq, Lk, D, dtype, dev())
    a = lc.chunk_attention(q, k, v)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, Lk - 7:] = k2[:, :, Lk - 7:] * -3.0 + 1.0
    v2[:, :, Lk - 7:] = v2[:, :, Lk - 7:] * 5.0 - 2.0
    b = lc.chunk_attention(q, k2, v2)
    assert torch.equal(_bits(a[:, :Lq - 7]), _bits(b[:, :Lq - 7]))
    assert not torch.equal(_bits(a[:, Lq - 7:]), _bits(b[:, Lq - 7:]))


@pytest.mark.parametrize("case", [(28, 4, 2304, 3457, 128, torch.bfloat16), (28, 4, 1, 100352, 128, torch.bfloat16),
                                  (28, 4, 5, 100352, 128, torch.float16), (28, 4, 600, 637, 128, torch.bfloat16),
                                  (4, 2, 1, 20000, 16, torch.float32)])
def test_bitwise_reproducible_and_stream_independent(case):
    import retake._native as nv
    import retake.longvideo_cache as lc

    Hq, Hkv, Lq, Lk, D, dtype = case
    q, k, v = ar.make_inputs("synth", 9, Hq, Hkv, Lq, Lk, D, dtype, dev())
    split = nv.lib.rtk_attention_workspace_bytes(Hq, Hkv, Lq, Lk, D, nv.dtype_code(q)) > 0
    assert split == (Lq < 2304)     # the few-row cases above are the key-split ones
    a = lc.chunk_attention(q, k, v)
    b = lc.chunk_attention(q, k, v)
    assert torch.equal(_bits(a), _bits(b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = lc.chunk_attention(q, k, v)
    side.synchronize()
    assert torch.equal(_bits(a), _bits(c))


def test_query_offset_restates_a_wider_mask():
    """query_offset = T - Lq: the rows see keys j <= (T - Lq) + i of the Lk < T keys - what an additive mask built over T
    uncompressed positions and sliced to the compressed keys lets through."""
    import retake.longvideo_cache as lc

    for Hq, Hkv, Lq, Lk, T, D, dtype in ((4, 2, 32, 53, 69, 16, torch.float32), (28, 4, 600, 900, 1100, 128, torch.bfloat16)):
        q, k, v = ar.make_inputs("synth", 4, Hq, Hkv, Lq, Lk, D, dtype, dev())
        out = lc.chunk_attention(q, k, v, query_offset=T - Lq)
        G = Hq // Hkv
        kk, vv = (t[:, :, None].expand(1, Hkv, G, Lk, D).reshape(1, Hq, Lk, D).double() for t in (k, v))
        s = (q.double() @ kk.transpose(2, 3)) * D ** -0.5
        vis = torch.arange(Lk, device=dev())[None, :] <= (T - Lq) + torch.arange(Lq, device=dev())[:, None]
        s.masked_fill_(~vis, -math.inf)
        ref = (torch.softmax(s, -1) @ vv).transpose(1, 2)
        err = (out.double() - ref).abs().max().item()
        bar = 1e-5 * max(1.0, ref.abs().max().item()) if dtype == torch.float32 else 2 * ar.half_ulp(dtype, ref.abs().max().item())
        assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------
# 6. through the cache on the product route
# ---------------------------------------------------------------------------------------------------
def _cache_cfg(layers, Hq, Hkv, D, **top):
    kw = {"kvcache_compression": True,
          "kvcache_compression_kwargs": {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    kw.update(top)
    return types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=layers, num_attention_heads=Hq,
                                 num_key_value_heads=Hkv, longvideo_kwargs=kw)


def test_attention_through_the_cache_on_the_prologue_route():
    """Two chunks x two layers at L 640, head_dim 128, bf16: update_pre_rope, then cache.attention on the views it
    returned, against float64 on the same views with SDPA's error (fed the same views through repeat_kv) as E - the bar of
    the fp64 test; after after_forward() the compressed cache is bitwise what the same run without the attention calls
    leaves (the attention reads the chunk's tail before the deferred compaction moves it)."""
    import retake.longvideo_cache as lc

    Hq, Hkv, D, L, layers = 28, 4, 128, 640, 2
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    g = torch.Generator(device=dev()).manual_seed(0)
    pool = [tuple((1.7 * torch.randn((1, L, h, D), generator=g, device=dev())).bfloat16().transpose(1, 2)
                  for h in (Hq, Hkv, Hkv)) for _ in range(4)]
    caches = [lc.build_kvcache(_cache_cfg(layers, Hq, Hkv, D, attention_kernel="hip")),
              lc.build_kvcache(_cache_cfg(layers, Hq, Hkv, D))]
    for with_attention, cache in zip((True, False), caches):
        call = 0
        for c in range(2):
            cache.keypatches_mask_chunk = torch.from_numpy(np.random.default_rng(c).uniform(size=L) < 0.3).to(dev())
            cache.kvcache_compression = True
            pos = torch.from_numpy(synth.mrope_position_ids(10 + 7 * c, L // 64, 8, 8, hw0=2)).to(dev())
            for l in range(layers):
                q, k, v = pool[call]
                call += 1
                fused = cache.update_pre_rope(q.clone(), k, v, l, pos, rot, SEC)
                assert fused is not None
                if not with_attention:
                    continue
                qr, kv, vv = fused
                P0 = kv.shape[2] - L
                assert P0 == (0 if c == 0 else L // 4) and not kv.is_contiguous()
                out = cache.attention(qr, kv, vv)
                assert out is not None and out.shape == (1, L, Hq, D)
                ref = ar.attention_fp64(qr, kv, vv)
                vis = ar.causal_visible(L, P0 + L, torch.arange(L, device=dev()), dev())
                sd = torch.nn.functional.scaled_dot_product_attention(
                    qr, lc.repeat_kv(kv, Hq // Hkv), lc.repeat_kv(vv, Hq // Hkv), attn_mask=vis[None, None]).transpose(1, 2)
                err = (out.double() - ref).abs().max().item()
                e = (sd.double() - ref).abs().max().item()
                bar = max(2 * e, ar.half_ulp(torch.bfloat16, ref.abs().max().item()))
                _note(f"cache route[chunk {c} layer {l} P0 {P0}]: native {err:.3e}  SDPA E {e:.3e}  bar {bar:.3e}")
                assert err <= bar
            cache.after_forward()
    assert caches[0].attention_calls == 4
    for l in range(layers):
        assert torch.equal(caches[0].key_cache[l], caches[1].key_cache[l])
        assert torch.equal(caches[0].value_cache[l], caches[1].value_cache[l])
        assert torch.equal(caches[0].position_cache[l], caches[1].position_cache[l])


# ---------------------------------------------------------------------------------------------------
# 7. memory
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,P0,dtype", [(2304, 3456, torch.bfloat16), (6272, 6272, torch.bfloat16), (640, 160, torch.float16)])
def test_allocates_the_output_and_nothing_else(Lq, P0, dtype):
    """For Lq >= 512 the allocator peak across the call exceeds the bytes held before it by no more than the output + 1 MiB:
    no repeat_kv copy, no mask, no logits."""
    import retake.longvideo_cache as lc

    Hq, Hkv, D = 28, 4, 128
    cache = lc.build_kvcache(_cache_cfg(1, Hq, Hkv, D, attention_kernel="hip"))
    _, (qv, kv, vv), _ = _viewed(Hq, Hkv, Lq, P0 + Lq, D, dtype)
    cache.attention(qv, kv, vv)        # any one-time workspace is allocated here and accounted for below
    torch.cuda.synchronize()
    fp = cache.memory_footprint()
    assert fp["attention_workspace"] == sum(t.numel() for t in cache._attn_ws.values())
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = cache.attention(qv, kv, vv)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert out.numel() * out.element_size() == Lq * Hq * D * 2
    assert peak - before <= Lq * Hq * D * 2 + (1 << 20), (peak - before, Lq * Hq * D * 2)


def test_key_split_workspace_is_in_the_footprint():
    import retake._native as nv
    import retake.longvideo_cache as lc

    Hq, Hkv, D, Lk = 28, 4, 128, 100352
    cache = lc.build_kvcache(_cache_cfg(1, Hq, Hkv, D, attention_kernel="hip"))
    q, k, v = ar.make_inputs("synth", 2, Hq, Hkv, 1, Lk, D, torch.bfloat16, dev())
    assert cache.memory_footprint()["attention_workspace"] == 0
    assert cache.attention(q, k, v) is not None
    need = nv.lib.rtk_attention_workspace_bytes(Hq, Hkv, 1, Lk, D, nv.RTK_BF16)
    assert need > 0 and cache.memory_footprint()["attention_workspace"] == need
    before = torch.cuda.memory_allocated()
    cache.attention(q, k, v)           # allocated once per geometry
    assert cache.memory_footprint()["attention_workspace"] == need and torch.cuda.memory_allocated() <= before + 1024


# ---------------------------------------------------------------------------------------------------
# 8. declines
# ---------------------------------------------------------------------------------------------------
def test_declines_return_none_and_the_patch_takes_its_own_route():
    """A shape the library declines (RTK_EUNSUPPORTED) comes back as None and the patch then produces today's output bit
    for bit.  Declined here: an over-2-GiB head extent, and head_dim 20 (not a multiple of 8).  head_dim 80 is NOT
    declined: it is a multiple of 8 and runs the general kernel (test_general_path_16bit_small_heads_against_fp64)."""
    import glue_stubs as gs
    import retake.longvideo_cache as lc
    import retake.qwen2_vl as q

    # a head_dim the kernels do not take
    qq, k, v = ar.make_inputs("synth", 1, 4, 2, 8, 40, 20, torch.float32, dev())
    assert lc.chunk_attention(qq, k, v) is None
    # one head of k / v spanning 2 GiB or more: 64 rows at a row stride of 2^24 elements of a 2 GiB buffer
    big = torch.zeros((1, 1, 1 << 23, 128), dtype=torch.bfloat16, device=dev())
    kb = big[:, :, ::1 << 17]
    assert kb.shape == (1, 1, 64, 128) and kb.stride(2) == 1 << 24
    qb = torch.randn((1, 4, 8, 128), device=dev()).bfloat16()
    cache = lc.build_kvcache(_cache_cfg(1, 4, 1, 128, attention_kernel="hip"))
    assert cache.attention(qb, kb, kb) is None and cache.attention_calls == 0
    del big, kb
    torch.cuda.empty_cache()
    # ... and a patch whose native call is declined produces what it produces with the switch off, bit for bit
    outs = []
    for kind in ("hip", None):
        layer = gs.StubAttention(0, 80, 4, 2, (2, 3, 5), 1.0, seed=3).to_device(dev()).eval()   # head_dim 20
        cache = lc.build_kvcache(_cache_cfg(1, 4, 2, 20, attention_kernel=kind))
        cache.kvcache_compression = False
        total = 0
        got = []
        for n in (5, 3, 1):
            x = torch.randn((1, n, 80), generator=torch.Generator().manual_seed(n)).to(dev())
            total += n
            mask4 = gs.causal_mask(n, total).to(dev())
            pos = torch.arange(total - n, total)[None, None].expand(3, 1, n).contiguous().to(dev())
            with torch.no_grad():
                o = q.retake_Qwen2VLAttention_forward(layer, x, mask4, pos, cache, False, True,
                                                      torch.arange(total - n, total, device=dev()))
            got.append(o[0])
            cache.after_forward()
        assert cache.attention_calls == 0
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.equal(a, b)

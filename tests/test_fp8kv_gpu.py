"""kv_cache_dtype="fp8_e4m3" on the GPU: the conversion instructions against tests/fp8_ref.py (the specification), the
archive kernel against its 16-bit twin, the two-segment chunk attention bit for bit against the 16-bit kernel over the
dequantised rows, a cache run beside its bf16 twin, refusals and memory.

What the KERNELS add to the quantisation's own error is bounded here (bitwise, or the 16-bit kernel's fp64 bars); how far
the quantisation itself moves an attention output is measured and recorded (profiles/fp8kv_parity_stats.txt), not barred."""
import ctypes as C
import gc
import os
import types

import numpy as np
import pytest
import torch

import attention_ref as ar
import fp8_ref
import synth

pytestmark = pytest.mark.gpu

Hq, Hkv, D = 28, 4, 128
SEC = [16, 24, 24]
A = synth.YARN_FACTOR4_ATTENTION_SCALING


def dev():
    return torch.device("cuda:0")


def _note(line: str):
    """Print a measured figure; also append it to $RETAKE_FP8KV_STATS when set (profiles/fp8kv_parity_stats.txt)."""
    print(line, flush=True)
    path = os.environ.get("RETAKE_FP8KV_STATS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _archive_call(k_src, v_src, keep_idx, keep, mode, P=0, pos_src=None, pos_dst=None, inv=None, scaling=1.0, sec=None):
    """rtk_pivotkv_archive_batched on one unit: k_src / v_src [Hkv, L, D] contiguous -> (k8, v8, ks, vs) on the device."""
    import retake._native as nv

    H, L, d = k_src.shape
    k8 = torch.full((H, keep, d), 0xAA, dtype=torch.uint8, device=dev())
    v8 = torch.full((H, keep, d), 0xAA, dtype=torch.uint8, device=dev())
    ks = torch.full((H, keep), -1.0, dtype=torch.float32, device=dev())
    vs = torch.full((H, keep), -1.0, dtype=torch.float32, device=dev())
    units = (nv.ArchiveUnit * 1)()
    u = units[0]
    u.k_src, u.k_src_stride_h, u.v_src, u.v_src_stride_h = k_src.data_ptr(), L * d, v_src.data_ptr(), L * d
    u.keep_idx = keep_idx.data_ptr() if keep_idx is not None else None
    if pos_src is not None:
        u.pos_src, u.pos_src_stride = pos_src.data_ptr(), pos_src.stride(0)
    if pos_dst is not None:
        u.pos_dst, u.pos_dst_stride = pos_dst.data_ptr(), pos_dst.stride(0)
    u.k8, u.v8, u.dst_stride_h = k8.data_ptr(), v8.data_ptr(), keep * d
    u.k_scale, u.v_scale, u.scale_stride_h = ks.data_ptr(), vs.data_ptr(), keep
    secs = (C.c_int * len(sec))(*sec) if sec else None
    nv.check(nv.lib.rtk_pivotkv_archive_batched(units, 1, H, d, keep, P, nv.dtype_code(k_src), mode, nv.ptr(inv), scaling, secs,
                                                len(sec) if sec else 0, nv.round_mode(k_src.dtype), nv.stream()),
             "rtk_pivotkv_archive_batched")
    torch.cuda.synchronize()
    return k8, v8, ks, vs


def _dequant_gpu(codes, scales, dtype):
    """rtk_fp8kv_dequant: codes [H, L, D] uint8 + scales [H, L] -> [H, L, D] of dtype."""
    import retake._native as nv

    H, L, d = codes.shape
    out = torch.empty((H, L, d), dtype=dtype, device=dev())
    nv.check(nv.lib.rtk_fp8kv_dequant(nv.ptr(codes), L * d, nv.ptr(scales), L, nv.ptr(out), L * d, H, L, d,
                                      nv.dtype_code(out), nv.stream()), "rtk_fp8kv_dequant")
    return out


# ---------------------------------------------------------------------------------------------------
# 1. the conversion instructions, exhaustively
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_conversion_exhaustive(dtype):
    """Every bit pattern of the dtype with |x| <= 448 through the archive kernel's conversion (rows pinned to scale 1):
    the codes are fp8_ref's.  And every code x a range of scales back through the dequantisation the attention uses."""
    import retake._native as nv

    rows = fp8_ref.exhaustive_rows(dtype)
    want_c, want_s = fp8_ref.quantize(rows)
    src = rows.to(dev())[None].contiguous()
    k8, v8, ks, vs = _archive_call(src, src.clone(), None, rows.shape[0], nv.COMPACT_K_COPY)
    assert torch.equal(ks.cpu()[0], want_s) and torch.equal(vs.cpu()[0], want_s)
    bad = (k8.cpu()[0] != want_c)
    assert not bad.any(), [(hex(rows.view(torch.int16)[i, j].item() & 0xffff), int(k8.cpu()[0][i, j]), int(want_c[i, j]))
                           for i, j in bad.nonzero()[:8].tolist()]
    assert torch.equal(v8.cpu()[0], want_c)
    # all 256 codes (NaN codes 0x7f / 0xff excluded: the rule never writes them) under scales 2^-30 .. 2^14
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    codes[codes & 0x7f == 0x7f] = 0
    # (fp16: down to 2^-14, where the smallest code, 2^-9, is still an fp16 subnormal - every product is exact)
    exps = list(range(-30, 15)) if dtype == torch.bfloat16 else list(range(-14, 6))
    c = codes.repeat(len(exps), 1)[:, :128].contiguous(), codes.repeat(len(exps), 1)[:, 128:].contiguous()
    sc = torch.tensor([2.0 ** e for e in exps], dtype=torch.float32)
    for half in c:
        got = _dequant_gpu(half[None].to(dev()), sc[None].to(dev()), dtype)[0].cpu()
        want = fp8_ref.dequantize(half, sc, dtype)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------
# 2. the archive kernel against the reference and its 16-bit twin
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2304, 6272])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_archive_kernel(dtype, L):
    import retake._native as nv

    keep = L // 4
    g = torch.Generator(device=dev()).manual_seed(L)
    k0 = (1.7 * torch.randn((Hkv, L, D), generator=g, device=dev())).to(dtype)
    v0 = (1.7 * torch.randn((Hkv, L, D), generator=g, device=dev())).to(dtype)
    v0[1, 5] = 0                                   # a zero row
    v0[2, 7] = 1e-4 * v0[2, 7]; v0[2, 7, 3] = 300   # one huge + many tiny  # noqa: E702
    score = torch.rand(L, generator=g, device=dev())
    score[:8] = 2.0    # rows 5 and 7 are kept
    keep_idx = torch.topk(score, keep).indices.sort().values.contiguous()
    pos_all = torch.from_numpy(synth.mrope_position_ids(40, L // 64, 8, 8, hw0=2)).to(dev()).reshape(3, L)
    pos_new = pos_all[:, keep_idx].contiguous()
    inv = torch.from_numpy(synth.inv_freq(D)).to(dev())
    for idx, n in ((keep_idx, keep), (None, L)):
        # copy mode: the gathered rows, quantised
        k8, v8, ks, vs = _archive_call(k0, v0, idx, n, nv.COMPACT_K_COPY)
        for codes, scales, src in ((k8, ks, k0), (v8, vs, v0)):
            rows = src if idx is None else src[:, idx]
            wc, ws = fp8_ref.quantize(rows)
            assert torch.equal(scales.cpu(), ws) and torch.equal(codes.cpu(), wc)
            assert torch.equal(_dequant_gpu(codes, scales, dtype).cpu().view(torch.int16),
                               fp8_ref.dequantize(wc, ws, dtype).view(torch.int16))
    # rotate mode: the K rows rtk_pivotkv_compact_batched writes for the same unit, quantised; ids copied
    k_tail, v_tail = torch.zeros_like(k0), v0.clone()
    units = (nv.CompactUnit * 1)()
    u = units[0]
    u.k_src, u.k_src_stride_h = k0.data_ptr(), L * D
    u.k_tail, u.k_tail_stride_h, u.v_tail, u.v_tail_stride_h = k_tail.data_ptr(), L * D, v_tail.data_ptr(), L * D
    u.keep_idx, u.pos_src, u.pos_src_stride = keep_idx.data_ptr(), pos_new.data_ptr(), keep
    n_ints = nv.lib.rtk_pivotkv_compact_sync_ints(1, Hkv, keep, D, nv.dtype_code(k0))
    sync = torch.zeros(n_ints, dtype=torch.int32, device=dev())
    sec = (C.c_int * 3)(*SEC)
    nv.check(nv.lib.rtk_pivotkv_compact_batched(units, 1, Hkv, D, keep, 3, nv.dtype_code(k0), nv.COMPACT_K_ROTATE, nv.ptr(inv), A,
                                                sec, 3, nv.round_mode(dtype), nv.ptr(sync), n_ints, nv.stream()),
             "rtk_pivotkv_compact_batched")
    torch.cuda.synchronize()
    pos_dst = torch.full((3, keep + 5), -7, dtype=torch.int64, device=dev())
    k8, v8, ks, vs = _archive_call(k0, v0, keep_idx, keep, nv.COMPACT_K_ROTATE, P=3, pos_src=pos_new, pos_dst=pos_dst, inv=inv,
                                   scaling=A, sec=SEC)
    wc, ws = fp8_ref.quantize(k_tail[:, :keep])
    assert torch.equal(ks.cpu(), ws) and torch.equal(k8.cpu(), wc)
    wc, ws = fp8_ref.quantize(v_tail[:, :keep])
    assert torch.equal(vs.cpu(), ws) and torch.equal(v8.cpu(), wc)
    assert torch.equal(pos_dst[:, :keep], pos_new) and (pos_dst[:, keep:] == -7).all()


# ---------------------------------------------------------------------------------------------------
# 3. / 4. the attention over [archive | 16-bit rows]
# ---------------------------------------------------------------------------------------------------
def _two_segments(kind, seed, Lq, L8, prefix, dtype):
    """q, the archive of the first L8 keys, the 16-bit tail [prefix + Lq rows] and the dense [dequant(archive) | tail]."""
    Lk = L8 + prefix + Lq
    q, k, v = ar.make_inputs(kind, seed, Hq, Hkv, Lq, Lk, D, dtype, dev())
    arch, dense = [], []
    for t in (k, v):
        if L8:
            c, s = fp8_ref.quantize(t[0, :, :L8])
            arch += [c[None].to(dev()), s[None].to(dev())]
            dense.append(torch.cat([fp8_ref.dequantize(c, s, dtype)[None].to(dev()), t[:, :, L8:]], dim=2))
        else:
            dense.append(t)
    if L8:
        archive = (arch[0], arch[2], arch[1], arch[3])
    else:   # an empty archive: the two-segment entry point with L8 = 0
        archive = (torch.empty((1, Hkv, 0, D), dtype=torch.uint8, device=dev()),) * 2 + \
                  (torch.empty((1, Hkv, 0), dtype=torch.float32, device=dev()),) * 2
    return q, archive, k[:, :, L8:], v[:, :, L8:], dense[0], dense[1]


@pytest.mark.parametrize("Lq,L8,prefix,dtype", [
    (2304, 3456, 17, torch.bfloat16), (2304, 0, 0, torch.bfloat16), (6272, 12544, 0, torch.bfloat16),
    (5, 100352, 0, torch.bfloat16), (1, 100352, 0, torch.bfloat16), (2304, 3456, 17, torch.float16),
], ids=["chunk+text", "no-archive", "baseline", "few-rows-5", "decode-1", "fp16"])
def test_attention_bitwise_against_the_16bit_kernel(Lq, L8, prefix, dtype):
    """L8 % 64 == 0: rtk_attention_forward_fp8kv(q, archive, tail) == rtk_attention_forward(q, [dequant(archive) | tail]) with
    q_offset + L8, every bit of every output element."""
    import retake.longvideo_cache as lc

    assert L8 % 64 == 0
    q, archive, kt, vt, kd, vd = _two_segments("synth", 21, Lq, L8, prefix, dtype)
    got = lc.chunk_attention(q, kt, vt, archive=archive)
    want = lc.chunk_attention(q, kd, vd)
    assert got is not None and want is not None and got.shape == want.shape == (1, Lq, Hq, D)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if L8:   # explicit offsets: the whole-sequence offset of the two-segment call, the same number for the dense call
        got = lc.chunk_attention(q, kt, vt, archive=archive, query_offset=L8 + prefix + 3)
        want = lc.chunk_attention(q, kd, vd, query_offset=L8 + prefix + 3)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("k", [1, 3, 7])
def test_attention_unaligned_archive_against_fp64(k):
    """L8 = 624 k (configs[4]'s keep per chunk: not a multiple of 64), so the 16-bit rows start a new key tile and the sums
    are grouped differently from the 16-bit kernel's: held to that kernel's own bars (tests/test_attention_gpu.py, the "2E"
    rule: within max(2 E, half an output ulp) of float64 on the same - dequantised - inputs, E the eager expression's error)."""
    import retake.longvideo_cache as lc
    import test_attention_gpu as tag

    Lq, L8, dtype = 2304, 624 * k, torch.bfloat16
    for kind in ("synth", "peaked", "rising"):
        q, archive, kt, vt, kd, vd = _two_segments(kind, 11, Lq, L8, 0, dtype)
        got = lc.chunk_attention(q, kt, vt, archive=archive)
        ref = ar.attention_fp64(q, kd, vd)
        err = (got.double() - ref).abs().max().item()
        mag = ref.abs().max().item()
        assert ar.eager_bytes(Hq, Lq, L8 + Lq) <= tag.EAGER_LIMIT
        e = (ar.attention_eager_reference(q, kd, vd).double() - ref).abs().max().item()
        twin = (lc.chunk_attention(q, kd, vd).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(dtype, mag))
        _note(f"fp64[fp8kv bf16 {kind} Lq{Lq} L8 {L8}]: native {err:.3e}  16-bit kernel {twin:.3e}  eager E {e:.3e}  "
              f"|ref|max {mag:.3f}  bar {bar:.3e}")
        assert err <= bar, (kind, k, err, bar)
        del q, archive, kt, vt, kd, vd, got, ref
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------
# 5. the cache beside its 16-bit twin
# ---------------------------------------------------------------------------------------------------
def _cfg(layers, ratio=0.25, reforge=True, fp8=True, head_dim=D, **extra):
    kw = {"compression_ratio": ratio, "compression_method": "pivotkv", "pos_embed_reforge": reforge}
    kw.update(extra)
    top = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": kw}
    if fp8:
        top["kv_cache_dtype"] = "fp8_e4m3"
    return types.SimpleNamespace(hidden_size=Hq * head_dim, num_hidden_layers=layers, num_attention_heads=Hq,
                                 num_key_value_heads=Hkv, longvideo_kwargs=top)


def _qkv(g, n, dtype, d=D):
    return tuple((1.7 * torch.randn((1, n, h, d), generator=g, device=dev())).to(dtype).transpose(1, 2) for h in (Hq, Hkv, Hkv))


class _Twins:
    """An fp8 cache and its 16-bit twin fed the same tensors, step by step."""

    def __init__(self, layers, ratio, reforge, mrope, dtype, tag):
        import retake.longvideo_cache as lc

        self.lc, self.layers, self.mrope, self.dtype, self.tag = lc, layers, mrope, dtype, tag
        self.sec = SEC if mrope else None
        self.a = lc.build_kvcache(_cfg(layers, ratio, reforge))
        self.b = lc.build_kvcache(_cfg(layers, ratio, reforge, fp8=False))
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.g = torch.Generator(device=dev()).manual_seed(3)
        self.t_next = 0
        self.dev_max = self.dev_mean = self.dev_rel = 0.0
        self.n_bitwise = self.n_unaligned = 0

    def text_ids(self, n):
        p = torch.arange(self.t_next, self.t_next + n, device=dev()).view(1, 1, n)
        self.t_next += n
        return p.expand(3, 1, n).contiguous() if self.mrope else p[0].contiguous()

    def video_ids(self, L):
        p = torch.from_numpy(synth.mrope_position_ids(self.t_next, L // 64, 8, 8, hw0=self.t_next)).to(dev())
        self.t_next += L // 64
        return p if self.mrope else p[0].contiguous()

    def feed(self, cache, l, q, k, v, pos, video):
        """One layer's prologue + cache update on `cache`: (rotated q, keys, values) as the attention patch gets them."""
        cache.kvcache_compression = video
        pos = pos.clone()
        out = (cache.update_pre_rope if video else cache.append_pre_rope)(q.clone(), k, v, l, pos, self.rot, self.sec)
        if out is not None:
            return out
        cache.shift_temporal_ids_(pos, l)   # the op-by-op route of the patches (no reforge: no shift, no ids kept)
        qr = synth.rope_forward(q.float(), pos, self.rot, self.sec).to(q.dtype)
        kr = synth.rope_forward(k.float(), pos, self.rot, self.sec).to(q.dtype)
        kw = {"query_states": qr, "position_ids": pos, "rotary_emb": self.rot, "mrope_section": self.sec}
        kk, vv = cache.update(kr, v, l, kw)
        return qr, kk, vv

    def step(self, n, video, mask=None):
        lc, a, b = self.lc, self.a, self.b
        pos = self.video_ids(n) if video else self.text_ids(n)
        a.keypatches_mask_chunk = b.keypatches_mask_chunk = mask
        for l in range(self.layers):
            q, k, v = _qkv(self.g, n, self.dtype)
            qa, ka, va = self.feed(a, l, q, k, v, pos, video)
            qb, kb, vb = self.feed(b, l, q, k, v, pos, video)
            assert torch.equal(qa, qb)
            n8 = a.archive_len(l)
            assert ka.shape[2] + n8 == kb.shape[2]
            calls = a.attention_calls
            oa = a.attention(qa, ka, va, layer_idx=l)
            ob = b.attention(qb, kb, vb, layer_idx=l)
            assert a.attention_calls == calls + 1 and oa.shape == ob.shape
            # the kernel's part: the 16-bit kernel over [dequant(archive) | 16-bit rows]
            if n8:
                k8, v8, ks, vs = a.archive(l)
                kd = torch.cat([fp8_ref.dequantize(k8[0].cpu(), ks[0].cpu(), self.dtype)[None].to(dev()), ka], dim=2)
                vd = torch.cat([fp8_ref.dequantize(v8[0].cpu(), vs[0].cpu(), self.dtype)[None].to(dev()), va], dim=2)
            else:
                kd, vd = ka, va
            want = lc.chunk_attention(qa, kd, vd)
            if n8 % 64 == 0:
                assert torch.equal(oa.view(torch.int16), want.view(torch.int16)), (self.tag, l, n8)
                self.n_bitwise += 1
            else:   # another grouping of the fp32 sums: both within the 16-bit kernel's bar of float64
                ref = ar.attention_fp64(qa, kd, vd)
                e = (ar.attention_eager_reference(qa, kd, vd).double() - ref).abs().max().item()
                bar = max(2.0 * e, ar.half_ulp(self.dtype, ref.abs().max().item()))
                assert (oa.double() - ref).abs().max().item() <= bar, (self.tag, l, n8)
                self.n_unaligned += 1
            # the quantisation's part: recorded
            d = (oa.float() - ob.float()).abs()
            rms = ob.float().pow(2).mean().sqrt().item()
            self.dev_max, self.dev_mean = max(self.dev_max, d.max().item()), max(self.dev_mean, d.mean().item())
            self.dev_rel = max(self.dev_rel, d.max().item() / rms)
            if not n8:
                assert torch.equal(oa, ob)
        a.after_forward()
        b.after_forward()
        self.compare()

    def compare(self):
        a, b = self.a, self.b
        assert a.num_evicted_tokens == b.num_evicted_tokens
        if a._batch is not None:
            assert torch.equal(a._batch.keep_idx, b._batch.keep_idx)
        pa, pb = a.position_cache, b.position_cache
        assert len(pa) == len(pb)
        for x, y in zip(pa, pb):
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
        for l in range(self.layers):
            assert a.get_seq_length(l) == b.get_seq_length(l)
            assert torch.equal(a.get_prev_temporal_idx(l), b.get_prev_temporal_idx(l)) if a.pos_embed_reforge else True
            st = a._layers[l]
            n8, at = st.len8, st.archive_at
            for which, view, twin in (("k", a.key_cache[l], b.key_cache[l]), ("v", a.value_cache[l], b.value_cache[l])):
                assert view.shape == twin.shape
                if not n8:
                    assert torch.equal(view, twin)
                    continue
                codes, scales = (st.k8, st.ks8) if which == "k" else (st.v8, st.vs8)
                wc, ws = fp8_ref.quantize(twin[0, :, at:at + n8])      # the twin's kept rows, quantised
                assert torch.equal(codes[0, :, :n8].cpu(), wc) and torch.equal(scales[0, :, :n8].cpu(), ws), (self.tag, l, which)
                # the dense view: [16-bit rows before archive_at | dequantised archive | remaining 16-bit rows]
                assert torch.equal(view[:, :, :at], twin[:, :, :at]) and torch.equal(view[:, :, at + n8:], twin[:, :, at + n8:])
                assert torch.equal(view[0, :, at:at + n8].cpu().view(torch.int16),
                                   fp8_ref.dequantize(wc, ws, self.dtype).view(torch.int16))


@pytest.mark.parametrize("tag,ratio,reforge,mrope", [
    ("mrope-reforge-0.25", 0.25, True, True), ("rope-reforge-0.25", 0.25, True, False),
    ("mrope-noreforge-0.25", 0.25, False, True), ("mrope-reforge-ratio1", 1, True, True),
])
def test_cache_beside_its_16bit_twin(tag, ratio, reforge, mrope):
    """Text prefix, 4 chunks x 2 layers (key-patch mask), text suffix, 3 decode steps through both caches: identical
    bookkeeping at every step, the archive = fp8_ref.quantize of the twin's kept rows bit for bit, every attention output of
    the fp8 cache = the 16-bit kernel over [dequant(archive) | 16-bit rows] (bitwise where len8 % 64 == 0), the dense views
    in the documented order.  The deviation from the twin's attention outputs - the quantisation's error - is recorded."""
    L, layers, dtype = 640, 2, torch.bfloat16
    t = _Twins(layers, ratio, reforge, mrope, dtype, tag)
    t.step(17, False)
    for c in range(4):
        mask = torch.from_numpy(np.random.default_rng(c).uniform(size=L) < 0.3).to(dev())
        t.step(L, True, mask)
        keep = max(1, int(ratio * L))
        assert t.a.archive_len(0) == (c + 1) * keep and t.a._layers[0].length == 17 and t.a._layers[0].archive_at == 17
    t.a.kvcache_compression = t.b.kvcache_compression = False
    t.step(9, False)
    for _ in range(3):
        t.step(1, False)
    assert t.n_bitwise > 0 and (t.n_unaligned > 0 or ratio == 1)
    assert t.a._layers[0].length == 17 + 9 + 3
    _note(f"twin[{tag} bf16 L{L} x4 chunks x{layers} layers]: fp8-cache attention output vs the bf16 twin's: max |d| "
          f"{t.dev_max:.3e}  worst mean |d| {t.dev_mean:.3e}  max |d| / rms(out) {t.dev_rel:.3e}  "
          f"({t.n_bitwise} calls bitwise vs the 16-bit kernel on the dequantised rows, {t.n_unaligned} within its fp64 bar)")
    # 7. memory_footprint counts the archive under cache_rows, exactly
    fp = t.a.memory_footprint()
    want = 0
    for st in t.a._layers:
        want += st.length * 2 * Hkv * D * 2 + st.len8 * 2 * Hkv * (D + 4) + (8 * st.pos.shape[0] * st.pos_len if st.pos is not None else 0)
    assert fp["cache_rows"] == want
    assert set(fp) == set(t.b.memory_footprint())      # no new keys


# ---------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cache_usable():
    import retake.longvideo_cache as lc

    L = 640
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    g = torch.Generator(device=dev()).manual_seed(1)
    pos = torch.from_numpy(synth.mrope_position_ids(0, L // 64, 8, 8)).to(dev())
    cache = lc.build_kvcache(_cfg(1))
    cache.kvcache_compression = True
    q, k, v = _qkv(g, L, torch.float32)
    with pytest.raises(NotImplementedError, match="bfloat16 or float16"):           # an fp32 model
        cache.update_pre_rope(q, k, v, 0, pos.clone(), rot, SEC)
    qr = synth.rope_forward(q, pos, rot, SEC)
    with pytest.raises(NotImplementedError, match="bfloat16 or float16"):
        cache.update(qr[:, :Hkv], v, 0, {"query_states": qr, "position_ids": pos.clone(), "rotary_emb": rot, "mrope_section": SEC})
    assert cache.memory_footprint()["total"] == 0 and cache.get_seq_length() == 0 and cache._batch is None

    class Dyn:   # a rotary module that has to be called
        inv_freq, attention_scaling, rope_type = rot.inv_freq, A, "dynamic"

        def __call__(self, x, p):
            return rot(x, p)

    q, k, v = _qkv(g, L, torch.bfloat16)
    qr = synth.rope_forward(q.float(), pos, rot, SEC).to(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="native RoPE"):
        cache.update(qr[:, :Hkv], v, 0, {"query_states": qr, "position_ids": pos.clone(), "rotary_emb": Dyn(), "mrope_section": SEC})
    with pytest.raises(NotImplementedError, match="position ids"):                   # reforge without the chunk's ids
        cache.update(qr[:, :Hkv], v, 0, {"query_states": qr, "rotary_emb": rot, "mrope_section": SEC})
    assert cache.memory_footprint()["total"] == 0 and cache._batch is None
    c64 = lc.build_kvcache(_cfg(1, head_dim=64))                                     # head_dim 64
    c64.kvcache_compression = True
    q64, k64, v64 = _qkv(g, L, torch.bfloat16, 64)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        c64.update_pre_rope(q64, k64, v64, 0, pos.clone(), synth.RotaryStub(synth.inv_freq(64), A, device=dev()), [8, 12, 12])
    assert c64.memory_footprint()["total"] == 0
    # the cache still works: a chunk, its attention, the flush
    out = cache.update_pre_rope(q.clone(), k, v, 0, pos.clone(), rot, SEC)
    assert out is not None
    module = types.SimpleNamespace(training=False, attention_dropout=0.0, config=None, layer_idx=0)
    calls = cache.attention_calls
    for kw, why in (({"output_attentions": True}, "attention weights"),):
        with pytest.raises(NotImplementedError, match=why):
            lc.native_attention(module, cache, *out, "causal", **kw)
    with pytest.raises(NotImplementedError, match="sliding window"):
        lc.native_attention(types.SimpleNamespace(training=False, layer_idx=0, config=types.SimpleNamespace(
            use_sliding_window=True, sliding_window=128, max_window_layers=0)), cache, *out, "causal")
    with pytest.raises(NotImplementedError, match="dropout"):
        lc.native_attention(types.SimpleNamespace(training=True, attention_dropout=0.1, config=None, layer_idx=0), cache, *out,
                            "causal")
    with pytest.raises(NotImplementedError, match="padded batch"):
        lc.native_attention(module, cache, *out, None)
    assert cache.attention_calls == calls                                            # nothing was launched
    o = lc.native_attention(module, cache, *out, "causal")
    assert o is not None and cache.attention_calls == calls + 1
    cache.after_forward()
    assert cache.archive_len(0) == L // 4 and cache.get_seq_length(0) == L // 4
    with pytest.raises(NotImplementedError, match="dequantised copies"):
        cache.key_cache[0] = cache.key_cache[0]
    with pytest.raises(NotImplementedError, match="dequantised copies"):
        cache.value_cache[0] = cache.value_cache[0]
    # a second chunk over the archive, through the patch's switch with a 4-D mask over the uncompressed positions
    out = cache.update_pre_rope(q.clone(), k, v, 0, pos.clone() + 10, rot, SEC)
    mask4 = torch.zeros((1, 1, L, 2 * L), dtype=torch.bfloat16, device=dev())
    o = lc.native_attention(module, cache, *out, mask4)
    k8, v8, ks, vs = cache.archive(0)
    want = lc.chunk_attention(out[0], out[1], out[2], archive=(k8, v8, ks, vs), query_offset=L)
    assert torch.equal(o, want)
    with pytest.raises(NotImplementedError, match="padded batch"):                  # a mask narrower than the keys
        lc.native_attention(module, cache, *out, mask4[..., :L])
    cache.after_forward()
    assert cache.archive_len(0) == L // 2
    # the flash-attn patch with a 2-D padding mask: its own route would miss the archive - it raises before the projections
    # or the cache are touched (the module stub has neither)
    import retake.qwen2_vl as qv

    pad = torch.ones(1, L, dtype=torch.long, device=dev())
    pad[0, 0] = 0
    stub = types.SimpleNamespace(config=types.SimpleNamespace(), layer_idx=0, is_causal=True)
    with pytest.raises(NotImplementedError, match="padded batch"):
        qv.retake_Qwen2VLFlashAttention2_forward(stub, torch.zeros(1, L, Hq * D, dtype=torch.bfloat16, device=dev()), pad, None,
                                                 cache, False, True, None)
    assert cache.archive_len(0) == L // 2 and cache.get_seq_length(0) == L // 2 and not cache._layers[0].pending


# ---------------------------------------------------------------------------------------------------
# 7. memory with the reserves the patches compute
# ---------------------------------------------------------------------------------------------------
def test_memory_with_the_patches_reserves():
    """A 17-token text prefix + 6 chunks of L = 2304 x 16 layers through both caches, built with the reserves the patched
    forwards pass (_prefill.cache_reserves): memory_footprint() is the allocator's view of the fp8 cache (2 % of
    memory_allocated(), the existing test's criterion - and 0.5 % of the bytes REQUESTED from the allocator, which leaves
    its block rounding out), and its K / V allocation is at most (D + 4) / (2 D) of the twin's video rows plus the 16-bit
    working buffer (text + one chunk + generation)."""
    import retake._prefill as pf
    import retake.longvideo_cache as lc

    if os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING") == "1":
        pytest.skip("torch keeps no allocator statistics without its caching allocator (memory_allocated() is 0)")
    layers, n_chunks, L, dtype, text = 16, 6, 2304, torch.bfloat16, 17
    keep = L // 4
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    g = torch.Generator(device=dev()).manual_seed(0)
    pool = [_qkv(g, L, dtype) for _ in range(4)]
    tq = _qkv(g, text, dtype)
    segs = [(0, text, "text"), (text, text + n_chunks * L, "video")]
    n_in = segs[-1][1]
    held, alloc = {}, {}
    requested = lambda: torch.cuda.memory_stats()["requested_bytes.all.current"]   # noqa: E731
    q = k = v = None
    for fp8 in (True, False):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base, rbase = torch.cuda.memory_allocated(), requested()
        cfg = _cfg(layers, fp8=fp8)
        reserves = pf.cache_reserves(cfg, n_in, L, segs)
        cache = lc.build_kvcache(cfg, **reserves)
        cache.kvcache_compression = False
        tp = torch.arange(text, device=dev()).view(1, 1, text).expand(3, 1, text).contiguous()
        for l in range(layers):
            assert cache.append_pre_rope(tq[0].clone(), tq[1], tq[2], l, tp.clone(), rot, SEC) is not None
        call = 0
        for c in range(n_chunks):
            cache.kvcache_compression = True
            cache.keypatches_mask_chunk = torch.from_numpy(np.random.default_rng(c).uniform(size=L) < 0.3).to(dev())
            pos = torch.from_numpy(synth.mrope_position_ids(text + 36 * c, L // 64, 8, 8, hw0=text)).to(dev())
            for l in range(layers):
                q, k, v = pool[call % len(pool)]
                call += 1
                out = cache.update_pre_rope(q.clone(), k, v, l, pos, rot, SEC)
                assert out is not None and cache.attention(*out, layer_idx=l) is not None
                del out
            cache.after_forward()
        cache.keypatches_mask_chunk = None
        del pos, tp
        torch.cuda.synchronize()
        held[fp8] = torch.cuda.memory_allocated() - base
        req = requested() - rbase
        fp = cache.memory_footprint()
        print(f"\n[memory] fp8 {fp8}: footprint {fp['total']}  allocated {held[fp8]}  requested {req}")
        assert abs(fp["total"] - held[fp8]) <= 0.02 * held[fp8], (fp8, fp["total"], held[fp8])
        assert abs(fp["total"] - req) <= 0.005 * req, (fp8, fp["total"], req)
        nb = lambda t: 0 if t is None else t.numel() * t.element_size()   # noqa: E731
        alloc[fp8] = sum(nb(st.k) + nb(st.v) + nb(st.k8) + nb(st.v8) + nb(st.ks8) + nb(st.vs8) for st in cache._layers)
        if fp8:
            assert reserves == {"reserve_tokens": text + L + 2048, "reserve_archive_tokens": n_chunks * keep}
            assert all(st.len8 == n_chunks * keep and st.length == text for st in cache._layers)
            assert fp["cache_rows"] == layers * (text * 2 * Hkv * D * 2 + n_chunks * keep * 2 * Hkv * (D + 4)
                                                 + 3 * 8 * (text + n_chunks * keep))
            working = layers * 2 * Hkv * D * 2 * reserves["reserve_tokens"]
        del cache
    video_rows_16 = layers * 2 * Hkv * D * 2 * n_chunks * keep
    assert alloc[True] <= (D + 4) / (2 * D) * video_rows_16 + working, (alloc, video_rows_16, working)
    _note(f"memory[bf16 L{L} x{n_chunks} chunks x{layers} layers, patches' reserves]: K/V allocation fp8 {alloc[True] / 2**20:.1f} MiB "
          f"vs 16-bit {alloc[False] / 2**20:.1f} MiB; held by the cache {held[True] / 2**20:.1f} vs {held[False] / 2**20:.1f} MiB")

"""kv_cache_dtype="fp8_e4m3" without a GPU: the properties of the quantisation rule (tests/fp8_ref.py is its
specification), the ABI of the new entry points, and the configuration checks of build_kvcache."""
import ctypes
import os
import subprocess
import types

import pytest
import torch

import fp8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(dtype):
    """[n, 128] rows of `dtype`: gaussian at many magnitudes, exact powers of two, zero rows, one huge + many tiny."""
    g = torch.Generator().manual_seed(7)
    out = []
    for mag in (1e-6, 1e-3, 0.3, 1.0, 1.7, 40.0, 3000.0):
        out.append(torch.randn(64, 128, generator=g) * mag)
    p2 = torch.ldexp(torch.ones(40, 128), torch.randint(-12, 12, (40, 128), generator=g).float())
    p2 *= torch.where(torch.rand(40, 128, generator=g) < 0.5, -1.0, 1.0)
    out.append(p2)
    for e in range(-14, 15):   # rows whose maximum is an exact power of two / just below / just above the m <= 0.875 switch
        for m in (1.0, 1.75, 1.7578125, 1.9921875):
            r = torch.randn(128, generator=g) * 0.1 * m * 2.0 ** e
            r[5] = -m * 2.0 ** e
            out.append(r[None])
    out.append(torch.zeros(3, 128))
    ht = torch.randn(16, 128, generator=g) * 1e-4
    ht[:, 17] = 250.0
    out.append(ht)
    return torch.cat(out).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_reference_properties(dtype):
    x = _rows(dtype)
    xf = x.float()
    codes, scale = fp8_ref.quantize(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scale.dtype == torch.float32 and scale.shape == x.shape[:1]
    amax = xf.abs().amax(-1)
    nz = amax > 0
    assert torch.equal(scale[~nz], torch.ones_like(scale[~nz]))
    m, e = torch.frexp(scale)
    assert torch.equal(m, torch.full_like(m, 0.5))                      # powers of two
    top = amax[nz].double() / scale[nz].double()
    assert (top > 224).all() and (top <= 448).all()
    assert (codes & 0x7f != 0x7f).all()                                 # no NaN code: nothing saturated or overflowed
    deq32 = fp8_ref.dequantize(codes, scale, torch.float32)
    deq = fp8_ref.dequantize(codes, scale, dtype)
    if dtype == torch.bfloat16:
        assert torch.equal(deq.float(), deq32)                          # 3 mantissa bits inside bf16's 7: exact
    c2, s2 = fp8_ref.quantize(deq32)                                    # idempotent
    same_scale = s2 == scale    # (a row whose largest code rounded up across the m <= 0.875 switch may pick the next scale)
    assert torch.equal(c2[same_scale], codes[same_scale])
    assert torch.equal(fp8_ref.dequantize(c2, s2, torch.float32), deq32)
    # per-element error: 3 mantissa bits (half an ulp = 2^-4 relative) on normal codes, 2^-9 spacing below 2^-6
    err = (deq32.double() - xf.double()).abs()
    sc = scale.double()[:, None]
    normal = xf.double().abs() / sc >= 2.0 ** -6
    assert (err[normal] <= 2.0 ** -4 * xf.double().abs()[normal]).all()
    assert (err[~normal] <= (2.0 ** -10 * sc).expand_as(err)[~normal]).all()


def test_reference_exhaustive_scale_one():
    """Every bf16 / fp16 value with |x| <= 448 in rows pinned to scale 1 (one element 448): the layout the GPU test uses."""
    for dtype in (torch.bfloat16, torch.float16):
        x = fp8_ref.exhaustive_rows(dtype)
        codes, scale = fp8_ref.quantize(x)
        assert torch.equal(scale, torch.ones_like(scale))
        want = x.float().to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(codes, want)


def test_new_entry_points_are_declared_exported_and_bound(tmp_path):
    import retake._native as nv
    import test_abi_cpu

    new = ["rtk_pivotkv_archive_batched", "rtk_attention_forward_fp8kv", "rtk_attention_workspace_bytes_fp8kv",
           "rtk_fp8kv_dequant"]
    syms = test_abi_cpu._declared_symbols()
    lib = ctypes.CDLL(nv.LIB_PATH)
    for s in new:
        assert s in syms, f"{s} not declared in retake_hip.h"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in nv.EXPORTS, f"{s} not bound"
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18
    # rtk_archive_unit: the ctypes mirror has the layout gcc gives the header's struct
    st, cname = nv.ArchiveUnit, "rtk_archive_unit"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             f'  printf("{cname} %zu\\n", sizeof({cname}));', f'  printf("max %d\\n", RTK_ARCHIVE_MAX_UNITS);']
    lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(st)
    assert int(got["max"]) == nv.ARCHIVE_MAX_UNITS
    for f, _ in st._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, f
    # argument errors without a launch
    dummy = (ctypes.c_char * 512)()
    p = ctypes.addressof(dummy)
    units = (nv.ArchiveUnit * 1)()
    call = lambda D=128, dt=nv.RTK_BF16, mode=nv.COMPACT_K_COPY, P=0: lib_call(nv, units, D, dt, mode, P, p)   # noqa: E731
    assert call() == nv.RTK_EINVAL and b"NULL" in nv.lib.rtk_last_error()
    u = units[0]
    u.k_src = u.v_src = u.k8 = u.v8 = u.k_scale = u.v_scale = p
    assert call(D=64) == nv.RTK_EUNSUPPORTED
    assert call(dt=nv.RTK_F32) == nv.RTK_EUNSUPPORTED
    assert call(mode=nv.COMPACT_K_INPLACE) == nv.RTK_EINVAL
    assert call(mode=nv.COMPACT_K_ROTATE, P=3) == nv.RTK_EINVAL and b"pos_src" in nv.lib.rtk_last_error()
    u.k_src = p + 2
    assert call() == nv.RTK_EUNSUPPORTED and b"aligned" in nv.lib.rtk_last_error()
    L = nv.lib
    assert L.rtk_attention_workspace_bytes_fp8kv(28, 4, 2304, 2321, 3456, 128, nv.RTK_BF16) == 0          # not split
    # few rows: the split covers the concatenation (archive padded to whole 64-key tiles)
    assert L.rtk_attention_workspace_bytes_fp8kv(28, 4, 1, 1, 100352, 128, nv.RTK_BF16) == \
        L.rtk_attention_workspace_bytes(28, 4, 1, 100353, 128, nv.RTK_BF16) > 0
    assert L.rtk_attention_workspace_bytes_fp8kv(28, 4, 1, 1, 100, 128, nv.RTK_BF16) == \
        L.rtk_attention_workspace_bytes(28, 4, 1, 129, 128, nv.RTK_BF16)
    assert L.rtk_attention_workspace_bytes_fp8kv(28, 4, 1, 1, 64, 128, nv.RTK_F32) == 0 and b"unsupported" in L.rtk_last_error()
    fw = lambda **k: fwd_call(nv, p, **k)   # noqa: E731
    assert fw(q=None) == nv.RTK_EINVAL
    assert fw(dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED
    assert fw(D=64) == nv.RTK_EUNSUPPORTED
    assert fw(L8=-1) == nv.RTK_EINVAL
    assert fw(k8=None) == nv.RTK_EINVAL and b"archive" in L.rtk_last_error()
    assert fw(q_offset=-1) == nv.RTK_EINVAL
    assert fw(stride8=8200) == nv.RTK_EUNSUPPORTED
    assert fw(Lq=1, Lk=1, L8=100352) == nv.RTK_EWORKSPACE
    assert L.rtk_fp8kv_dequant(None, 0, None, 0, None, 0, 1, 1, 128, nv.RTK_BF16, None) == nv.RTK_EINVAL
    assert L.rtk_fp8kv_dequant(p, 128, p, 1, p, 128, 1, 1, 64, nv.RTK_BF16, None) == nv.RTK_EUNSUPPORTED


def lib_call(nv, units, D, dt, mode, P, p):
    return nv.lib.rtk_pivotkv_archive_batched(units, 1, 4, D, 4, P, dt, mode, p, 1.0, None, 0, 1, None)


def fwd_call(nv, p, q="p", k8="p", L8=64, Lq=64, Lk=64, q_offset=0, D=128, dtype=None, stride8=8192):
    q = p if q == "p" else q
    k8 = p if k8 == "p" else k8
    dtype = nv.RTK_BF16 if dtype is None else dtype
    return nv.lib.rtk_attention_forward_fp8kv(q, Lq * D, D, p, p, Lk * D, D, k8, p, p, p, L8, stride8, 64, p, 28, 4, Lq, Lk,
                                              q_offset, D, dtype, 0.088, None, 0, None)


def _cfg(**top):
    kw = {"kvcache_compression": True,
          "kvcache_compression_kwargs": {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}}
    extra = top.pop("compression_kwargs", {})
    kw["kvcache_compression_kwargs"].update(extra)
    kw.update(top)
    return types.SimpleNamespace(hidden_size=28 * 128, num_hidden_layers=2, num_attention_heads=28, num_key_value_heads=4,
                                 longvideo_kwargs=kw)


def test_config_validation():
    import retake.longvideo_cache as lc

    c = lc.build_kvcache(_cfg(attention_kernel="hip", kv_cache_dtype="fp8_e4m3"), reserve_tokens=100, reserve_archive_tokens=7)
    assert c.kv_cache_dtype == "fp8_e4m3" and c.attention_kernel == "hip"
    assert c.reserve_tokens == 100 and c.reserve_archive_tokens == 7
    assert c.get_seq_length() == 0 and c.archive_len(0) == 0 and c.archive(0) is None
    assert c.memory_footprint()["total"] == 0
    assert lc.build_kvcache(_cfg(attention_kernel="hip")).kv_cache_dtype is None            # the default is unchanged
    assert lc.build_kvcache(_cfg()).kv_cache_dtype is None
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        lc.build_kvcache(_cfg(attention_kernel="hip", kv_cache_dtype="fp8_e5m2"))
    with pytest.raises(ValueError, match="attention_kernel"):
        lc.build_kvcache(_cfg(kv_cache_dtype="fp8_e4m3"))
    with pytest.raises(ValueError, match="defer_rerotation"):
        lc.build_kvcache(_cfg(attention_kernel="hip", kv_cache_dtype="fp8_e4m3", compression_kwargs={"defer_rerotation": True}))
    with pytest.raises(NotImplementedError):     # the list views are dequantised copies in this mode
        c.key_cache[0] = torch.zeros(1, 4, 3, 128)
    with pytest.raises(ValueError, match="layer_idx"):
        c.attention(None, None, None)


def test_patch_reserves():
    """What the patched forwards hand build_kvcache: unchanged by default; in fp8 mode the kept video rows are reserved in
    the archive and the 16-bit buffers shrink to text + one chunk + generation."""
    import retake._prefill as pf

    segs = [(0, 17, "text"), (17, 17 + 8 * 2304, "video"), (17 + 8 * 2304, 17 + 8 * 2304 + 9, "text")]
    n = segs[-1][1]
    cfg = _cfg(attention_kernel="hip")
    assert pf.cache_reserves(cfg, n, 2304, segs) == {"reserve_tokens": pf.expected_cache_tokens(cfg, n, 2304)}
    cfg = _cfg(attention_kernel="hip", kv_cache_dtype="fp8_e4m3")
    assert pf.cache_reserves(cfg, n, 2304, segs) == {"reserve_tokens": 26 + 2304 + 2048, "reserve_archive_tokens": 8 * 576}
    assert pf.cache_reserves(types.SimpleNamespace(longvideo_kwargs=None), n, 2304, segs) == {"reserve_tokens": None}


def test_flash_attention_patch_refuses_what_the_native_route_cannot_serve():
    """The flash-attn patch only takes the native route for an unpadded causal call; with fp8 rows its own route would attend
    over the 16-bit rows alone, so a padding mask, a non-causal layer or a top-left-mask flash-attn build raise - before
    the projections or the cache are touched (the module stub has neither)."""
    import retake.longvideo_cache as lc
    import retake.qwen2_vl as q

    cache = lc.build_kvcache(_cfg(attention_kernel="hip", kv_cache_dtype="fp8_e4m3"))
    x = torch.zeros(1, 8, 16)
    pad = torch.ones(1, 8, dtype=torch.long)
    pad[0, 0] = 0
    mod = lambda **kw: types.SimpleNamespace(config=types.SimpleNamespace(), layer_idx=0, **kw)   # noqa: E731
    for m, mask, why in ((mod(is_causal=True), pad, "padded batch"), (mod(is_causal=False), None, "non-causal"),
                         (mod(is_causal=True, _flash_attn_uses_top_left_mask=True), None, "top-left")):
        with pytest.raises(NotImplementedError, match=why):
            q.retake_Qwen2VLFlashAttention2_forward(m, x, mask, None, cache, False, True, None)
    assert cache.get_seq_length() == 0 and cache.memory_footprint()["total"] == 0 and cache.attention_calls == 0

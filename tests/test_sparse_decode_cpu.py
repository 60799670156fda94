"""Page-sparse decode without a GPU: the entry points are exported and bound, the unit struct has the header's layout, the
workspace queries state their rule, every host-side refusal of the four calls returns before any launch (the pointers are
never dereferenced), and sparse_decode(cache) refuses what it does not serve."""
import ctypes
import os
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 32   # a 256-byte aligned address nobody reads
D = 128
NEW = ("rtk_pivotkv_page_summary_batched", "rtk_attention_page_bound", "rtk_attention_decode_paged",
       "rtk_attention_decode_paged_workspace_bytes", "rtk_attention_decode_sparse", "rtk_attention_decode_sparse_workspace_bytes")


def test_entry_points_are_appended_without_an_abi_bump():
    import retake._native as nv

    header = open(os.path.join(ROOT, "include", "retake_hip.h")).read()
    for name in NEW:
        assert name in nv.EXPORTS and hasattr(nv.lib, name) and f" {name}(" in header
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18
    assert '"Page-sparse decode"' in header and "RTK_PAGE_ROWS 32" in header and nv.PAGE_ROWS == 32


def test_unit_struct_has_the_headers_layout(tmp_path):
    import retake._native as nv

    st, cname = nv.PageSummaryUnit, "rtk_page_summary_unit"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             f'  printf("size %zu\\n", sizeof({cname}));', '  printf("max %d\\n", RTK_PAGE_SUMMARY_MAX_UNITS);']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(st) and int(got["max"]) == nv.PAGE_SUMMARY_MAX_UNITS
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def _plan(Hkv, K):
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    n0 = max(1, min(ceil(512, Hkv), ceil(K, 128)))
    kps = 128 * ceil(ceil(K, n0), 128)
    return ceil(K, kps)


def test_workspace_queries_state_their_rule():
    import retake._native as nv

    lib = nv.lib
    for Hq, Hkv, Lq, first, n, tail, keep in [(28, 4, 1, 37, 100352, 64, 256), (4, 2, 2, 5, 293, 3, 3), (14, 2, 1, 0, 288, 0, 9)]:
        ve = first + n
        Lk, pages = ve + tail, -(-n // 32)
        K = -(-first // 32) * 32 + 32 * keep + tail
        partials = _plan(Hkv, K) * Hq * Lq * (D + 2) * 4
        assert lib.rtk_attention_decode_paged_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, nv.RTK_BF16) == partials
        a16 = lambda b: -(-b // 16) * 16   # noqa: E731
        assert lib.rtk_attention_decode_sparse_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, nv.RTK_F16) == \
            a16(Hkv * pages * 4) + a16(Hkv * keep * 4) + partials
        # with the identity list over aligned rows the plan is the packed call's over the rows as they lie
        if first % 32 == 0 and n % 32 == 0 and keep == pages:
            assert partials == lib.rtk_attention_decode_workspace_bytes(Hq, Hkv, Lq, Lk, D, nv.RTK_BF16)
    for q in (lib.rtk_attention_decode_paged_workspace_bytes, lib.rtk_attention_decode_sparse_workspace_bytes):
        assert q(28, 4, 1, 500, 32, 320, 0, D, nv.RTK_BF16) == 0 and b"keep_pages" in lib.rtk_last_error()
        assert q(28, 4, 1, 500, 32, 320, 10, D, nv.RTK_BF16) == 0          # 9 pages
        assert q(28, 4, 1, 500, 321, 320, 1, D, nv.RTK_BF16) == 0 and b"first" in lib.rtk_last_error()
        assert q(28, 4, 1, 300, 32, 320, 1, D, nv.RTK_BF16) == 0 and b"ve" in lib.rtk_last_error()
        assert q(28, 4, 3, 500, 32, 320, 1, D, nv.RTK_BF16) == 0 and b"packed rows" in lib.rtk_last_error()
        assert q(28, 4, 1, 500, 32, 320, 1, 64, nv.RTK_BF16) == 0 and q(28, 4, 1, 500, 32, 320, 1, D, nv.RTK_F32) == 0


def refusals_of_the_paged_calls():
    """Every RTK_EINVAL / RTK_EUNSUPPORTED of rtk_attention_decode_paged and rtk_attention_decode_sparse, each under the
    call's own name, before any launch (tests/test_attention_paged_gpu.py runs this on a machine with a GPU as well)."""
    import retake._native as nv

    lib = nv.lib
    ok = dict(q=BASE, q_sh=D, q_sl=28 * D, k=BASE, v=BASE, kv_sh=4096 * D, kv_sl=D, out=BASE, Hq=28, Hkv=4, Lq=1, Lk=500, off=499,
              D=D, dtype=nv.RTK_BF16, scale=D ** -0.5, first=32, ve=320, extra=BASE, keep=4, ws=BASE, ws_bytes=1 << 24)

    def paged(s):
        return lib.rtk_attention_decode_paged(s["q"], s["q_sh"], s["q_sl"], s["k"], s["v"], s["kv_sh"], s["kv_sl"], s["out"], s["Hq"],
                                              s["Hkv"], s["Lq"], s["Lk"], s["off"], s["D"], s["dtype"], s["scale"], s["first"],
                                              s["ve"], s["extra"], s["keep"], s["ws"], s["ws_bytes"], None)

    def sparse(s):
        return lib.rtk_attention_decode_sparse(s["q"], s["q_sh"], s["q_sl"], s["k"], s["v"], s["kv_sh"], s["kv_sl"], s["out"], s["Hq"],
                                               s["Hkv"], s["Lq"], s["Lk"], s["off"], s["D"], s["dtype"], s["scale"], s["first"],
                                               s["ve"], s["extra"], s.get("summ_sh", 9 * 2 * D), s["keep"], s["ws"], s["ws_bytes"],
                                               None)

    inval, unsup = nv.RTK_EINVAL, nv.RTK_EUNSUPPORTED
    cases = [(dict(q=None), inval, b"NULL"), (dict(k=None), inval, b"NULL"), (dict(v=None), inval, b"NULL"),
             (dict(out=None), inval, b"NULL"), (dict(extra=None), inval, b"NULL"),
             (dict(Hq=-28), inval, b"positive"), (dict(Lq=0), inval, b"positive"), (dict(Lk=-1), inval, b"positive"),
             (dict(Hq=30), inval, b"multiple"),
             (dict(first=-1), inval, b"first"), (dict(first=321), inval, b"first"), (dict(ve=501), inval, b"ve"),
             (dict(keep=0), inval, b"keep_pages"), (dict(keep=10), inval, b"keep_pages"), (dict(keep=-3), inval, b"keep_pages"),
             (dict(off=318), inval, b"ve - 1"), (dict(Lk=321, off=318), inval, b"ve - 1"),
             (dict(q=BASE + 2), inval, b"16 bytes"), (dict(k=BASE + 8), inval, b"16 bytes"), (dict(out=BASE + 4), inval, b"16 bytes"),
             (dict(kv_sl=D + 1), inval, b"16 bytes"), (dict(q_sh=D + 4), inval, b"16 bytes"),
             (dict(ws=None), inval, b"workspace"), (dict(ws_bytes=64), inval, b"workspace"), (dict(ws=BASE + 8), inval, b"workspace"),
             (dict(scale=0.0), inval, b"scale"),
             (dict(dtype=nv.RTK_F32), unsup, b"dtype"), (dict(D=64), unsup, b"head_dim"), (dict(Lq=3, off=497), unsup, b"packed rows"),
             (dict(kv_sl=1 << 23), unsup, b"2 GiB")]
    for name, call in (("rtk_attention_decode_paged", paged), ("rtk_attention_decode_sparse", sparse)):
        for change, code, word in cases:
            rc = call({**ok, **change})
            msg = lib.rtk_last_error()
            assert rc == code and word in msg and msg.startswith(name.encode() + b":"), (name, change, rc, msg)
    assert paged({**ok, "extra": BASE + 2}) == inval and b"list" in lib.rtk_last_error()
    assert sparse({**ok, "extra": BASE + 8}) == inval and b"summ" in lib.rtk_last_error()
    assert sparse({**ok, "summ_sh": 9 * 2 * D - 8}) == inval and b"summ" in lib.rtk_last_error()


def test_the_attention_calls_refuse_on_the_host():
    refusals_of_the_paged_calls()


def test_summary_and_bound_refuse_on_the_host():
    import retake._native as nv

    lib = nv.lib
    assert lib.rtk_pivotkv_page_summary_batched(None, 0, 4, D, nv.RTK_BF16, None) == 0         # nothing to do
    assert lib.rtk_pivotkv_page_summary_batched(None, 1, 4, D, nv.RTK_BF16, None) == nv.RTK_EINVAL
    assert lib.rtk_pivotkv_page_summary_batched(None, -1, 4, D, nv.RTK_BF16, None) == nv.RTK_EINVAL
    u = (nv.PageSummaryUnit * 1)()

    def summary(Hkv=4, d=D, dtype=nv.RTK_BF16, **f):
        base = dict(k=BASE, k_stride_h=4096 * D, first=37, n=100, summ=BASE, summ_stride_h=4 * 2 * D)
        for name, val in {**base, **f}.items():
            setattr(u[0], name, val)
        return lib.rtk_pivotkv_page_summary_batched(u, 1, Hkv, d, dtype, None)

    assert summary(dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and summary(d=64) == nv.RTK_EUNSUPPORTED
    for bad in (dict(k=None), dict(summ=None), dict(first=-1), dict(n=-1), dict(k=BASE + 2), dict(summ=BASE + 4),
                dict(k_stride_h=4096 * D + 1), dict(summ_stride_h=4 * 2 * D - 8), dict(k_stride_h=100 * D), dict(Hkv=0)):
        assert summary(**bad) == nv.RTK_EINVAL, bad
        assert lib.rtk_last_error().startswith(b"rtk_pivotkv_page_summary_batched:")

    def bound(q=BASE, q_sh=D, q_sl=28 * D, summ=BASE, s_sh=9 * 2 * D, Hq=28, Hkv=4, Lq=1, pages=9, d=D, dtype=nv.RTK_BF16, ub=BASE):
        return lib.rtk_attention_page_bound(q, q_sh, q_sl, summ, s_sh, Hq, Hkv, Lq, pages, d, dtype, ub, None)

    assert bound(dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and bound(d=256) == nv.RTK_EUNSUPPORTED
    for bad in (dict(q=None), dict(summ=None), dict(ub=None), dict(Hq=0), dict(Hq=30), dict(Lq=0), dict(pages=0), dict(pages=-2),
                dict(q=BASE + 2), dict(summ=BASE + 8), dict(ub=BASE + 2), dict(q_sl=28 * D + 1), dict(q_sl=64), dict(s_sh=9 * 2 * D - 8)):
        assert bound(**bad) == nv.RTK_EINVAL, bad
        assert lib.rtk_last_error().startswith(b"rtk_attention_page_bound:")


def _cache(**top):
    import retake.longvideo_cache as lc

    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    kw.update(top.pop("kw", {}))
    cfg = types.SimpleNamespace(hidden_size=4 * D, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                longvideo_kwargs=dict({"kvcache_compression": True, "kvcache_compression_kwargs": kw,
                                                       "attention_kernel": "hip"}, **top))
    return lc.build_kvcache(cfg)


def test_arming_refuses_what_the_route_does_not_serve():
    import retake._sparse_decode as sd

    c = _cache()
    assert c._sparse is None and c.sparse_attention_calls == 0 and c.page_summary_calls == 0
    assert "page_summaries" not in c.memory_footprint()
    for bad in (0, -1, True, 8192.0, "8192", None):
        with pytest.raises(ValueError, match="keep_rows"):
            sd.sparse_decode(c, bad)
    with pytest.raises(ValueError, match="video_end"):
        sd.sparse_decode(c)
    with pytest.raises(ValueError, match="video_end"):
        sd.sparse_decode(c, 4096)
    c.attention_kernel = None
    with pytest.raises(ValueError, match="attention_kernel"):
        sd.sparse_decode(c)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        sd.sparse_decode(_cache(kv_cache_dtype="fp8_e4m3"))
    with pytest.raises(NotImplementedError, match="defer_rerotation"):
        sd.sparse_decode(_cache(kw={"defer_rerotation": True}))
    c = _cache()
    c.forked_from = object()
    with pytest.raises(NotImplementedError, match="branch"):
        sd.sparse_decode(c)
    c = _cache()
    c.focused_from = object()
    with pytest.raises(NotImplementedError, match="focused"):
        sd.sparse_decode(c)
    c = _cache()
    for name in ("page_summaries", "sparse_pages", "sparse_bounds"):
        with pytest.raises(ValueError, match="not armed"):
            getattr(sd, name)(c, 0)
    sd.dense_decode(c)   # disarming an unarmed cache is nothing
    assert c._sparse is None

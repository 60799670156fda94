"""Page-sparse decode over an fp8 archive without a GPU: the entry points are exported and bound, the unit struct has the
header's layout, the workspace queries state their rule (K = 32 keep_pages + Lk), every host-side refusal of the three
calls returns before any launch (the pointers are never dereferenced), and sparse_decode(cache, archive=...) refuses what
it does not serve."""
import ctypes
import os
import subprocess

import pytest

from test_sparse_decode_cpu import BASE, ROOT, _cache, _plan

D = 128
NEW = ("rtk_pivotkv_page_summary_fp8k_batched", "rtk_attention_decode_paged_fp8kv", "rtk_attention_decode_paged_fp8kv_workspace_bytes",
       "rtk_attention_decode_sparse_fp8kv", "rtk_attention_decode_sparse_fp8kv_workspace_bytes")


def test_entry_points_are_appended_without_an_abi_bump():
    import retake._native as nv

    header = open(os.path.join(ROOT, "include", "retake_hip.h")).read()
    for name in NEW:
        assert name in nv.EXPORTS and hasattr(nv.lib, name) and f" {name}(" in header
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18
    assert "rtk_page_summary_fp8k_unit" in header


def test_unit_struct_has_the_headers_layout(tmp_path):
    import retake._native as nv

    st, cname = nv.PageSummaryFp8kUnit, "rtk_page_summary_fp8k_unit"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             f'  printf("size %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_workspace_queries_state_their_rule():
    import retake._native as nv

    lib = nv.lib
    a16 = lambda b: -(-b // 16) * 16   # noqa: E731
    for Hq, Hkv, Lq, L8, Lk, keep in [(28, 4, 1, 100352, 101, 256), (4, 2, 2, 293, 3, 3), (14, 2, 1, 288, 40, 9), (14, 2, 2, 293, 72, 10)]:
        pages = -(-L8 // 32)
        K = 32 * keep + Lk
        partials = _plan(Hkv, K) * Hq * Lq * (D + 2) * 4
        assert lib.rtk_attention_decode_paged_fp8kv_workspace_bytes(Hq, Hkv, Lq, Lk, L8, keep, D, nv.RTK_BF16) == partials
        assert lib.rtk_attention_decode_sparse_fp8kv_workspace_bytes(Hq, Hkv, Lq, Lk, L8, keep, D, nv.RTK_F16) == \
            a16(Hkv * pages * 4) + a16(Hkv * keep * 4) + partials
        # with every page kept the plan is rtk_attention_decode_fp8kv's over the archive as it lies
        if keep == pages:
            assert partials == lib.rtk_attention_decode_workspace_bytes_fp8kv(Hq, Hkv, Lq, Lk, L8, D, nv.RTK_BF16)
    for q in (lib.rtk_attention_decode_paged_fp8kv_workspace_bytes, lib.rtk_attention_decode_sparse_fp8kv_workspace_bytes):
        assert q(28, 4, 1, 101, 288, 0, D, nv.RTK_BF16) == 0 and b"keep_pages" in lib.rtk_last_error()
        assert q(28, 4, 1, 101, 288, 10, D, nv.RTK_BF16) == 0 and b"keep_pages" in lib.rtk_last_error()   # 9 pages
        assert q(28, 4, 1, 101, 0, 1, D, nv.RTK_BF16) == 0 and b"L8" in lib.rtk_last_error()
        assert q(28, 4, 1, 101, -3, 1, D, nv.RTK_BF16) == 0 and b"L8" in lib.rtk_last_error()
        assert q(28, 4, 1, 0, 288, 1, D, nv.RTK_BF16) == 0 and b"positive" in lib.rtk_last_error()
        assert q(28, 4, 3, 101, 288, 1, D, nv.RTK_BF16) == 0 and b"packed rows" in lib.rtk_last_error()
        assert q(28, 4, 1, 101, 288, 1, 64, nv.RTK_BF16) == 0 and q(28, 4, 1, 101, 288, 1, D, nv.RTK_F32) == 0
        assert q(28, 4, 1, 101, 1 << 24, 1, D, nv.RTK_BF16) == 0 and b"extent" in lib.rtk_last_error()


def refusals_of_the_fp8_paged_calls():
    """Every RTK_EINVAL / RTK_EUNSUPPORTED of rtk_attention_decode_paged_fp8kv and rtk_attention_decode_sparse_fp8kv, each under
    the call's own name, before any launch (tests/test_attention_paged_fp8_gpu.py runs this on a machine with a GPU as well)."""
    import retake._native as nv

    lib = nv.lib
    ok = dict(q=BASE, q_sh=D, q_sl=28 * D, k=BASE, v=BASE, kv_sh=4096 * D, kv_sl=D, k8=BASE, v8=BASE, ks=BASE, vs=BASE, L8=293,
              sh8=4096 * D, shs=4096, out=BASE, Hq=28, Hkv=4, Lq=1, Lk=101, off=100, D=D, dtype=nv.RTK_BF16, scale=D ** -0.5,
              extra=BASE, keep=4, ws=BASE, ws_bytes=1 << 24)

    def head(s):
        return (s["q"], s["q_sh"], s["q_sl"], s["k"], s["v"], s["kv_sh"], s["kv_sl"], s["k8"], s["v8"], s["ks"], s["vs"], s["L8"],
                s["sh8"], s["shs"], s["out"], s["Hq"], s["Hkv"], s["Lq"], s["Lk"], s["off"], s["D"], s["dtype"], s["scale"])

    def paged(s):
        return lib.rtk_attention_decode_paged_fp8kv(*head(s), s["extra"], s["keep"], s["ws"], s["ws_bytes"], None)

    def sparse(s):
        return lib.rtk_attention_decode_sparse_fp8kv(*head(s), s["extra"], s.get("summ_sh", 10 * 2 * D), s["keep"], s["ws"],
                                                     s["ws_bytes"], None)

    inval, unsup = nv.RTK_EINVAL, nv.RTK_EUNSUPPORTED
    cases = [(dict(q=None), inval, b"NULL"), (dict(k=None), inval, b"NULL"), (dict(v=None), inval, b"NULL"),
             (dict(out=None), inval, b"NULL"), (dict(extra=None), inval, b"NULL"),
             (dict(k8=None), inval, b"NULL"), (dict(v8=None), inval, b"NULL"), (dict(ks=None), inval, b"NULL"),
             (dict(vs=None), inval, b"NULL"),
             (dict(Hq=-28), inval, b"positive"), (dict(Lq=0), inval, b"positive"), (dict(Lk=0), inval, b"positive"),
             (dict(Hq=30), inval, b"multiple"), (dict(L8=-1), inval, b"L8"), (dict(L8=0), inval, b"L8"),
             (dict(keep=0), inval, b"keep_pages"), (dict(keep=11), inval, b"keep_pages"), (dict(keep=-3), inval, b"keep_pages"),
             (dict(off=99), inval, b"q_offset"), (dict(Lq=2, off=98), inval, b"q_offset"),
             (dict(q=BASE + 2), inval, b"16 bytes"), (dict(k=BASE + 8), inval, b"16 bytes"), (dict(out=BASE + 4), inval, b"16 bytes"),
             (dict(k8=BASE + 8), inval, b"16 bytes"), (dict(v8=BASE + 4), inval, b"16 bytes"), (dict(sh8=4096 * D + 4), inval, b"16 bytes"),
             (dict(kv_sl=D + 1), inval, b"16 bytes"), (dict(q_sh=D + 4), inval, b"16 bytes"),
             (dict(ks=BASE + 2), inval, b"4-byte"), (dict(vs=BASE + 1), inval, b"4-byte"),
             (dict(ws=None), inval, b"workspace"), (dict(ws_bytes=64), inval, b"workspace"), (dict(ws=BASE + 8), inval, b"workspace"),
             (dict(scale=0.0), inval, b"scale"),
             (dict(dtype=nv.RTK_F32), unsup, b"dtype"), (dict(D=64), unsup, b"head_dim"), (dict(Lq=3, off=98), unsup, b"packed rows"),
             (dict(kv_sl=1 << 23), unsup, b"2 GiB"), (dict(L8=1 << 24), unsup, b"extent")]
    for name, call in (("rtk_attention_decode_paged_fp8kv", paged), ("rtk_attention_decode_sparse_fp8kv", sparse)):
        for change, code, word in cases:
            rc = call({**ok, **change})
            msg = lib.rtk_last_error()
            assert rc == code and word in msg and msg.startswith(name.encode() + b":"), (name, change, rc, msg)
    assert paged({**ok, "extra": BASE + 2}) == inval and b"list" in lib.rtk_last_error()
    assert sparse({**ok, "extra": BASE + 8}) == inval and b"summ" in lib.rtk_last_error()
    assert sparse({**ok, "summ_sh": 10 * 2 * D - 8}) == inval and b"summ" in lib.rtk_last_error()


def test_the_attention_calls_refuse_on_the_host():
    refusals_of_the_fp8_paged_calls()


def refusals_of_the_fp8_summary_call():
    import retake._native as nv

    lib = nv.lib
    assert lib.rtk_pivotkv_page_summary_fp8k_batched(None, 0, 4, D, nv.RTK_BF16, None) == 0         # nothing to do
    assert lib.rtk_pivotkv_page_summary_fp8k_batched(None, 1, 4, D, nv.RTK_BF16, None) == nv.RTK_EINVAL
    assert lib.rtk_pivotkv_page_summary_fp8k_batched(None, -1, 4, D, nv.RTK_BF16, None) == nv.RTK_EINVAL
    u = (nv.PageSummaryFp8kUnit * 1)()

    def summary(Hkv=4, d=D, dtype=nv.RTK_BF16, **f):
        base = dict(k8=BASE, k8_stride_h=4096 * D, k_scale=BASE, scale_stride_h=4096, n=100, summ=BASE, summ_stride_h=4 * 2 * D)
        for name, val in {**base, **f}.items():
            setattr(u[0], name, val)
        return lib.rtk_pivotkv_page_summary_fp8k_batched(u, 1, Hkv, d, dtype, None)

    assert summary(dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and summary(d=64) == nv.RTK_EUNSUPPORTED
    for bad in (dict(k8=None), dict(k_scale=None), dict(summ=None), dict(n=-1), dict(k8=BASE + 2), dict(summ=BASE + 4),
                dict(k_scale=BASE + 2), dict(k8_stride_h=4096 * D + 8), dict(summ_stride_h=4 * 2 * D - 8), dict(k8_stride_h=99 * D),
                dict(scale_stride_h=99), dict(scale_stride_h=-1), dict(Hkv=0),
                dict(n=1 << 24, k8_stride_h=1 << 31, scale_stride_h=1 << 24, summ_stride_h=(1 << 19) * 2 * D)):   # 2 GiB of codes
        assert summary(**bad) == nv.RTK_EINVAL, bad
        assert lib.rtk_last_error().startswith(b"rtk_pivotkv_page_summary_fp8k_batched:")
    assert summary(n=0, k8=None, k_scale=None, summ=None) == 0   # an empty unit is skipped: nothing to launch


def test_the_summary_call_refuses_on_the_host():
    refusals_of_the_fp8_summary_call()


def test_arming_refuses_what_the_route_does_not_serve():
    import retake._sparse_decode as sd

    for bad in (1, 0, "True", None, 1.0):
        with pytest.raises(ValueError, match="archive must be a bool"):
            sd.sparse_decode(_cache(kv_cache_dtype="fp8_e4m3"), 8192, archive=bad)
        with pytest.raises(ValueError, match="archive must be a bool"):
            sd.sparse_decode(_cache(), archive=bad)
    with pytest.raises(ValueError, match="archive=True needs a cache with kv_cache_dtype"):
        sd.sparse_decode(_cache(), 8192, archive=True)
    # off is off: without the key an fp8 cache is refused as before; the message now names the key
    with pytest.raises(ValueError, match="kv_cache_dtype.*archive=True"):
        sd.sparse_decode(_cache(kv_cache_dtype="fp8_e4m3"), archive=False)
    c = _cache(kv_cache_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="video_end"):
        sd.sparse_decode(c, archive=True)
    assert c._sparse is None and c.page_summary_calls == 0
    with pytest.raises(ValueError, match="keep_rows"):
        sd.sparse_decode(c, 0, archive=True)
    c.forked_from = object()
    with pytest.raises(NotImplementedError, match="branch"):
        sd.sparse_decode(c, archive=True)
    c = _cache(kv_cache_dtype="fp8_e4m3")
    c.focused_from = object()
    with pytest.raises(NotImplementedError, match="focused"):
        sd.sparse_decode(c, archive=True)
    c = _cache(kv_cache_dtype="fp8_e4m3")
    c.attention_kernel = None
    with pytest.raises(ValueError, match="attention_kernel"):
        sd.sparse_decode(c, archive=True)

"""The wide family of the page-sparse decode calls without a GPU: the four entry points are exported and bound without an
ABI bump, the workspace queries state their rule (0 beyond 64 packed rows, the narrow query's value at up to 16), every
host-side refusal returns before any launch (the pointers are never dereferenced), and sparse_decode(cache) refuses a
`wide` that is no bool and wide=True over the fp8 archive."""
import os

import pytest

from test_sparse_decode_cpu import BASE, D, _cache, _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtk_attention_decode_paged_wide", "rtk_attention_decode_paged_wide_workspace_bytes", "rtk_attention_decode_sparse_wide",
       "rtk_attention_decode_sparse_wide_workspace_bytes")


def test_entry_points_are_appended_without_an_abi_bump():
    import retake._native as nv

    header = open(os.path.join(ROOT, "include", "retake_hip.h")).read()
    for name in NEW:
        assert name in nv.EXPORTS and hasattr(nv.lib, name) and f" {name}(" in header
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18


def test_workspace_queries_state_their_rule():
    import retake._native as nv

    lib = nv.lib
    a16 = lambda b: -(-b // 16) * 16   # noqa: E731
    #            Hq Hkv Lq first n      tail keep      R
    for Hq, Hkv, Lq, first, n, tail, keep in [(28, 4, 6, 37, 100352, 64, 256),    # 42
                                              (28, 4, 9, 37, 100352, 64, 512),    # 63
                                              (14, 2, 3, 5, 293, 3, 3),           # 21
                                              (16, 2, 8, 0, 288, 7, 9),           # 64
                                              (2, 2, 33, 32, 288, 40, 9)]:        # 33
        ve = first + n
        Lk, pages = ve + tail, -(-n // 32)
        K = -(-first // 32) * 32 + 32 * keep + tail
        partials = _plan(Hkv, K) * Hq * Lq * (D + 2) * 4
        assert lib.rtk_attention_decode_paged_wide_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, nv.RTK_BF16) == partials
        assert lib.rtk_attention_decode_sparse_wide_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, nv.RTK_F16) == \
            a16(Hkv * pages * 4) + a16(Hkv * keep * 4) + partials
        # the narrow family does not take these rows
        assert lib.rtk_attention_decode_paged_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep, D, nv.RTK_BF16) == 0
        # with the identity list over aligned rows the plan is the wide call's over the rows as they lie
        if first % 32 == 0 and n % 32 == 0 and keep == pages:
            assert partials == lib.rtk_attention_decode_wide_workspace_bytes(Hq, Hkv, Lq, Lk, D, nv.RTK_BF16)
    pairs = ((lib.rtk_attention_decode_paged_wide_workspace_bytes, lib.rtk_attention_decode_paged_workspace_bytes),
             (lib.rtk_attention_decode_sparse_wide_workspace_bytes, lib.rtk_attention_decode_sparse_workspace_bytes))
    for wide, narrow in pairs:
        # at most 16 packed rows: the narrow query
        for Hq, Hkv, Lq in [(28, 4, 1), (28, 4, 2), (4, 2, 2), (16, 1, 1), (8, 8, 16)]:
            got = wide(Hq, Hkv, Lq, 500, 37, 330, 4, D, nv.RTK_BF16)
            assert got and got == narrow(Hq, Hkv, Lq, 500, 37, 330, 4, D, nv.RTK_BF16)
        # beyond 64 packed rows: 0
        assert wide(28, 4, 10, 500, 32, 320, 1, D, nv.RTK_BF16) == 0 and b"packed rows" in lib.rtk_last_error()
        assert wide(2, 2, 65, 500, 32, 320, 1, D, nv.RTK_BF16) == 0 and b"at most 64" in lib.rtk_last_error()
        assert wide(28, 4, 6, 500, 32, 320, 0, D, nv.RTK_BF16) == 0 and b"keep_pages" in lib.rtk_last_error()
        assert wide(28, 4, 6, 500, 32, 320, 10, D, nv.RTK_BF16) == 0          # 9 pages
        assert wide(28, 4, 6, 500, 321, 320, 1, D, nv.RTK_BF16) == 0 and b"first" in lib.rtk_last_error()
        assert wide(28, 4, 6, 300, 32, 320, 1, D, nv.RTK_BF16) == 0 and b"ve" in lib.rtk_last_error()
        assert wide(28, 4, 6, 500, 32, 320, 1, 64, nv.RTK_BF16) == 0 and wide(28, 4, 6, 500, 32, 320, 1, D, nv.RTK_F32) == 0


def refusals_of_the_wide_paged_calls():
    """Every RTK_EINVAL / RTK_EUNSUPPORTED of rtk_attention_decode_paged_wide and rtk_attention_decode_sparse_wide at 42
    packed rows, each under the call's own name, before any launch: the narrow calls' list (tests/test_sparse_decode_cpu.py)
    with the wide envelope (tests/test_attention_paged_wide_gpu.py runs this on a machine with a GPU as well)."""
    import retake._native as nv

    lib = nv.lib
    ok = dict(q=BASE, q_sh=6 * D, q_sl=D, k=BASE, v=BASE, kv_sh=4096 * D, kv_sl=D, out=BASE, Hq=28, Hkv=4, Lq=6, Lk=500, off=494,
              D=D, dtype=nv.RTK_BF16, scale=D ** -0.5, first=32, ve=320, extra=BASE, keep=4, ws=BASE, ws_bytes=1 << 24)

    def paged(s):
        return lib.rtk_attention_decode_paged_wide(s["q"], s["q_sh"], s["q_sl"], s["k"], s["v"], s["kv_sh"], s["kv_sl"], s["out"],
                                                   s["Hq"], s["Hkv"], s["Lq"], s["Lk"], s["off"], s["D"], s["dtype"], s["scale"],
                                                   s["first"], s["ve"], s["extra"], s["keep"], s["ws"], s["ws_bytes"], None)

    def sparse(s):
        return lib.rtk_attention_decode_sparse_wide(s["q"], s["q_sh"], s["q_sl"], s["k"], s["v"], s["kv_sh"], s["kv_sl"], s["out"],
                                                    s["Hq"], s["Hkv"], s["Lq"], s["Lk"], s["off"], s["D"], s["dtype"], s["scale"],
                                                    s["first"], s["ve"], s["extra"], s.get("summ_sh", 9 * 2 * D), s["keep"], s["ws"],
                                                    s["ws_bytes"], None)

    inval, unsup = nv.RTK_EINVAL, nv.RTK_EUNSUPPORTED
    cases = [(dict(q=None), inval, b"NULL"), (dict(k=None), inval, b"NULL"), (dict(v=None), inval, b"NULL"),
             (dict(out=None), inval, b"NULL"), (dict(extra=None), inval, b"NULL"),
             (dict(Hq=-28), inval, b"positive"), (dict(Lq=0), inval, b"positive"), (dict(Lk=-1), inval, b"positive"),
             (dict(Hq=30), inval, b"multiple"),
             (dict(first=-1), inval, b"first"), (dict(first=321), inval, b"first"), (dict(ve=501), inval, b"ve"),
             (dict(keep=0), inval, b"keep_pages"), (dict(keep=10), inval, b"keep_pages"), (dict(keep=-3), inval, b"keep_pages"),
             (dict(off=318), inval, b"ve - 1"), (dict(Lk=325, off=318), inval, b"ve - 1"),
             (dict(q=BASE + 2), inval, b"16 bytes"), (dict(k=BASE + 8), inval, b"16 bytes"), (dict(out=BASE + 4), inval, b"16 bytes"),
             (dict(kv_sl=D + 1), inval, b"16 bytes"), (dict(q_sh=6 * D + 4), inval, b"16 bytes"),
             (dict(ws=None), inval, b"workspace"), (dict(ws_bytes=64), inval, b"workspace"), (dict(ws=BASE + 8), inval, b"workspace"),
             (dict(scale=0.0), inval, b"scale"),
             (dict(dtype=nv.RTK_F32), unsup, b"dtype"), (dict(D=64), unsup, b"head_dim"),
             (dict(Lq=10, off=490), unsup, b"packed rows"), (dict(Hq=4, Hkv=4, Lq=65, off=435), unsup, b"packed rows"),
             (dict(kv_sl=1 << 23), unsup, b"2 GiB")]
    for name, call in (("rtk_attention_decode_paged_wide", paged), ("rtk_attention_decode_sparse_wide", sparse)):
        for change, code, word in cases:
            rc = call({**ok, **change})
            msg = lib.rtk_last_error()
            assert rc == code and word in msg and msg.startswith(name.encode() + b":"), (name, change, rc, msg)
    assert paged({**ok, "extra": BASE + 2}) == inval and b"list" in lib.rtk_last_error()
    assert sparse({**ok, "extra": BASE + 8}) == inval and b"summ" in lib.rtk_last_error()
    assert sparse({**ok, "summ_sh": 9 * 2 * D - 8}) == inval and b"summ" in lib.rtk_last_error()
    # at most 16 packed rows the call IS the narrow call: its refusals come under the narrow call's name
    few = {**ok, "Lq": 2, "q_sh": 2 * D, "off": 318}
    assert paged(few) == inval and lib.rtk_last_error().startswith(b"rtk_attention_decode_paged:")
    assert sparse(few) == inval and lib.rtk_last_error().startswith(b"rtk_attention_decode_sparse:")


def test_the_wide_calls_refuse_on_the_host():
    refusals_of_the_wide_paged_calls()


def test_arming_refuses_a_wide_that_is_no_bool_and_the_archive():
    import retake._sparse_decode as sd

    c = _cache()
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="wide must be a bool"):
            sd.sparse_decode(c, 8192, wide=bad)
    with pytest.raises(ValueError, match="wide paged kernel over the fp8 archive is not built"):
        sd.sparse_decode(_cache(kv_cache_dtype="fp8_e4m3"), 8192, archive=True, wide=True)
    with pytest.raises(ValueError, match="wide paged kernel over the fp8 archive is not built"):
        sd.sparse_decode(c, 8192, True, True)
    with pytest.raises(ValueError, match="video_end"):   # wide=True gets as far as wide=False: no video rows yet
        sd.sparse_decode(c, 8192, wide=True)
    with pytest.raises(ValueError, match="not armed"):
        sd.sparse_wide_calls(c)
    assert c._sparse is None and c.page_summary_calls == 0

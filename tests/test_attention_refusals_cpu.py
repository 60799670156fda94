"""The host-side refusals of the native attention entry points (include/retake_hip.h "Chunk attention"): one refusing call per
row of ROWS, its return code and the whole rtk_last_error() text compared with tests/golden/attention_refusals.json.  The
file pins the order of the checks, the codes and the wording - what a caller's logs and `nv.check` show - across rewrites of
the code around the kernels.  Nothing here launches a kernel: every row is refused before any launch, and every launching
call goes without a workspace (or with a misaligned one) for a shape that needs one.

    python tests/test_attention_refusals_cpu.py --record     rewrites the golden file from the library as built
"""
import ctypes
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_refusals.json")
P = 0x10000   # a 16-byte aligned non-NULL "pointer"
SIX = ("rtk_attention_forward", "rtk_attention_forward_fp8kv", "rtk_attention_forward_shared", "rtk_attention_decode",
       "rtk_attention_decode_fp8kv", "rtk_attention_decode_shared")
GROUP, GROUP_WS = "rtk_attention_decode_group", "rtk_attention_decode_group_workspace_bytes"
# every row starts from this error text (no row's own), so a refusal that sets none - the group query's Hq / Hkv test - is
# recorded as such
SENTINEL = "rtk_attention_workspace_bytes: unsupported head_dim 4 (a multiple of 8 up to 256)"


def _reset(nv):
    assert nv.lib.rtk_attention_workspace_bytes(1, 1, 1, 1, 4, nv.RTK_F32) == 0 and nv.lib.rtk_last_error().decode() == SENTINEL


def _query(fn):
    return fn.replace("_forward", "_workspace_bytes") if "_forward" in fn else fn.replace("_decode", "_decode_workspace_bytes")


def _defaults(fn):
    """A call that passes every check but the workspace's: 4 query heads x 2 rows over 2048 keys (the chunk plan splits the
    keys four ways; the packed plan always leaves partials), no workspace."""
    d = dict(q=P, qsh=256, qsl=128, k=P, v=P, ksh=128 * 2048, ksl=128, out=P, Hq=4, Hkv=2, Lq=2, Lk=2048, off=None, D=128,
             dtype="bf16", scale=0.1, ws=None, ws_bytes=0)
    if not fn.endswith(("_fp8kv", "_shared")):
        return d
    d.update(k8=P, v8=P, ksc=P, vsc=P, L8=64, sh8=8192, shs=64)
    if fn.endswith("_shared"):
        d.update(ks=P, vs=P, Ls=64, ssh=128 * 64, ssl=128)
    return d


def _call_six(nv, fn, over):
    a = _defaults(fn)
    unknown = set(over) - set(a) - {"ws_need"}
    assert not unknown, (fn, unknown)
    a.update(over)
    code = {"f32": nv.RTK_F32, "bf16": nv.RTK_BF16, "f16": nv.RTK_F16, "refround": nv.RTK_BF16_REFROUND}[a["dtype"]]
    shape = [a["Hq"], a["Hkv"], a["Lq"], a["Lk"]] + ([a["L8"]] if "L8" in a else []) + ([a["Ls"]] if "Ls" in a else []) + [a["D"], code]
    need = getattr(nv.lib, _query(fn))(*shape)
    # no row may get as far as a launch: the shape is refused (the query says why) or needs a workspace the row withholds
    assert need > 0 or nv.lib.rtk_last_error().decode() != SENTINEL, (fn, over, "the shape needs no workspace")
    _reset(nv)
    if a.pop("ws_need", False):
        a["ws_bytes"] = need
    assert a["ws"] is None or a["ws"] % 16 != 0 or a["ws_bytes"] < need, (fn, over)
    off = a["Lk"] - a["Lq"] if a["off"] is None else a["off"]
    args = [a["q"], a["qsh"], a["qsl"], a["k"], a["v"], a["ksh"], a["ksl"]]
    if "Ls" in a:
        args += [a["ks"], a["vs"], a["Ls"], a["ssh"], a["ssl"]]
    if "L8" in a:
        args += [a["k8"], a["v8"], a["ksc"], a["vsc"], a["L8"], a["sh8"], a["shs"]]
    args += [a["out"], a["Hq"], a["Hkv"], a["Lq"], a["Lk"], off, a["D"], code, a["scale"], a["ws"], a["ws_bytes"], None]
    return getattr(nv.lib, fn)(*args)


def _call_group(nv, fn, over):
    a = dict(own=(3, 3), brs=True, q=P, k=P, q_sh=128, kv_sh=8 * 128, kv_sl=128, ks=P, vs=P, Ls=64, ssh=64 * 128, ssl=128, k8=None,
             v8=None, ksc=None, vsc=None, L8=0, sh8=8192, shs=64, out=P, Hq=4, Hkv=2, D=128, dtype="bf16", scale=0.088, ws=None,
             ws_bytes=0, B=None)
    unknown = set(over) - set(a) - {"ws_need"}
    assert not unknown, (fn, unknown)
    a.update(over)
    code = {"f32": nv.RTK_F32, "bf16": nv.RTK_BF16, "f16": nv.RTK_F16}[a["dtype"]]
    own = a["own"]
    B = len(own) if a["B"] is None else a["B"]
    rows = (ctypes.c_int * max(1, len(own)))(*own)
    if fn == GROUP_WS:
        return nv.lib.rtk_attention_decode_group_workspace_bytes(rows if a["brs"] else None, B, a["Hq"], a["Hkv"], a["L8"], a["Ls"],
                                                                 a["D"], code)
    if a.pop("ws_need", False):
        a["ws_bytes"] = nv.lib.rtk_attention_decode_group_workspace_bytes(rows, B, a["Hq"], a["Hkv"], a["L8"], a["Ls"], a["D"], code)
        _reset(nv)
        assert a["ws_bytes"] > 0
    assert a["ws"] is None or a["ws"] % 16 != 0   # (the group's partials always live in the caller's workspace)
    brs = (nv.DecodeBranch * max(1, len(own)))()
    for br, lk in zip(brs, own):
        br.q, br.q_stride_h, br.k, br.v = a["q"], a["q_sh"], a["k"], a["k"]
        br.kv_stride_h, br.kv_stride_l, br.Lk = a["kv_sh"], a["kv_sl"], lk
    return nv.lib.rtk_attention_decode_group(brs if a["brs"] else None, B, a["ks"], a["vs"], a["Ls"], a["ssh"], a["ssl"], a["k8"],
                                             a["v8"], a["ksc"], a["vsc"], a["L8"], a["sh8"], a["shs"], a["out"], a["Hq"], a["Hkv"],
                                             a["D"], code, a["scale"], a["ws"], a["ws_bytes"], None)


def _rows():
    rows = []
    for fn in SIX:
        fp8, shared, decode = fn.endswith(("_fp8kv", "_shared")), fn.endswith("_shared"), "_decode" in fn
        r = [("null_q", dict(q=None)), ("null_k", dict(k=None)), ("null_v", dict(v=None)), ("null_out", dict(out=None)),
             ("null_before_shape", dict(out=None, Hq=0)),
             ("not_positive", dict(Lq=0)), ("divisibility", dict(Hq=5)), ("lk_lt_lq", dict(Lq=65, Lk=64)),
             ("dtype_code", dict(dtype="refround")), ("head_dim_not_8n", dict(D=84)), ("head_dim_over_256", dict(D=264)),
             ("hq_over_65535", dict(Hq=65536, Hkv=1)), ("shape_before_scale", dict(Hq=5, scale=0.0)),
             ("dtype_f32", dict(dtype="f32")), ("head_dim_64", dict(D=64, qsl=64, ksl=64)),
             ("scale_zero", dict(scale=0.0)), ("scale_nan", dict(scale=float("nan"))), ("scale_inf", dict(scale=float("inf"))),
             ("scale_before_q_offset", dict(scale=-1.0, off=0)), ("q_offset_small", dict(off=2045)),
             ("q_offset_huge", dict(off=0x40000000)),
             ("layout_q_pointer", dict(q=P + 2)), ("layout_out_pointer", dict(out=P + 8)), ("layout_q_stride_h", dict(qsh=4)),
             ("layout_kv_stride_l", dict(ksl=132)), ("layout_kv_row_short", dict(ksl=64)), ("layout_kv_stride_h_negative", dict(ksh=-128)),
             ("layout_before_extent", dict(q=P + 2, ksl=1 << 20)),
             ("extent_kv_2gib", dict(ksl=1 << 20)), ("extent_q_2gib", dict(qsl=1 << 30)),
             ("workspace_missing", dict()), ("workspace_null_with_bytes", dict(ws=None, ws_need=True)),
             ("workspace_too_small", dict(ws=P, ws_bytes=16)), ("workspace_misaligned", dict(ws=P + 4, ws_need=True))]
        if decode:
            r += [("envelope_packed_rows", dict(Hq=28, Hkv=4, Lq=3)), ("envelope_before_operands", dict(Hq=28, Hkv=4, Lq=3, scale=0.0))]
        if fp8:   # (L8 == 0 falls through to the 16-bit call in the _fp8kv entry points; in the _shared ones the archive is just empty)
            r += [("l8_negative", dict(L8=-1)), ("archive_extent", dict(L8=1 << 24)), ("archive_keys_extent", dict(L8=0x3fffffc0)),
                  ("null_archive_k8", dict(k8=None)), ("null_archive_v_scale", dict(vsc=None)),
                  ("null_archive_before_scale", dict(k8=None, scale=0.0)),
                  ("layout_archive_pointer", dict(v8=P + 8)), ("layout_archive_scale_pointer", dict(ksc=P + 2)),
                  ("layout_archive_stride", dict(sh8=8200)), ("layout_archive_scale_stride_negative", dict(shs=-1)),
                  ("l8_zero_workspace", dict(L8=0)), ("l8_zero_scale", dict(L8=0, scale=0.0)),
                  ("l8_zero_q_offset", dict(L8=0, off=0)), ("l8_zero_null_archive_pointers", dict(L8=0, k8=None))]
        if shared:
            r += [("ls_negative", dict(Ls=-1)), ("l8_before_ls", dict(L8=-1, Ls=-1)), ("shared_keys_extent", dict(Ls=0x40000000)),
                  ("null_shared_ks", dict(ks=None)), ("null_shared_vs", dict(vs=None)),
                  ("null_shared_before_null_archive", dict(ks=None, k8=None)),
                  ("layout_shared_pointer", dict(ks=P + 2)), ("layout_shared_stride_l", dict(ssl=132)),
                  ("layout_shared_row_short", dict(ssl=64)), ("layout_shared_stride_h", dict(ssh=-128)),
                  ("extent_shared_2gib", dict(Ls=1024, ssl=1 << 20)), ("shared_before_own_layout", dict(ks=P + 2, q=P + 2)),
                  ("shared_without_archive_workspace", dict(L8=0, k8=None, v8=None, ksc=None, vsc=None)),
                  ("ls_zero_falls_through_workspace", dict(Ls=0)), ("ls_zero_falls_through_null_archive", dict(Ls=0, k8=None)),
                  ("ls_zero_falls_through_scale", dict(Ls=0, scale=0.0)),
                  ("ls_zero_ignores_shared_pointers", dict(Ls=0, ks=None, vs=None)),
                  ("ls_zero_l8_zero_falls_through_twice", dict(Ls=0, L8=0)),
                  ("ls_zero_l8_zero_falls_through_twice_q_offset", dict(Ls=0, L8=0, off=0))]
        rows += [(f"{fn}/{name}", fn, over) for name, over in r]
    g = [("null_branches", dict(brs=False)), ("null_out", dict(out=None)), ("no_branches", dict(B=0)),
         ("not_positive", dict(Hkv=0)), ("divisibility", dict(Hq=5)),
         ("dtype_f32", dict(dtype="f32")), ("head_dim_64", dict(D=64)), ("dtype_before_head_dim", dict(dtype="f32", D=64)),
         ("envelope_branches", dict(own=(1,) * 9)), ("envelope_packed_rows", dict(own=(1,) * 5, Hq=14)),
         ("null_branch_q", dict(q=None)), ("null_branch_k", dict(k=None)), ("branch_without_rows", dict(own=(3, 0))),
         ("l8_negative", dict(L8=-1)), ("ls_negative", dict(Ls=-1)), ("archive_extent", dict(L8=1 << 24)),
         ("shared_keys_extent", dict(Ls=0x40000000)),
         ("null_shared", dict(ks=None)), ("layout_shared_pointer", dict(vs=P + 2)), ("layout_shared_stride_l", dict(ssl=132)),
         ("extent_shared_2gib", dict(Ls=1024, ssl=1 << 20)), ("null_shared_before_null_archive", dict(ks=None, L8=64)),
         ("null_archive", dict(L8=64)), ("null_archive_before_scale", dict(L8=64, scale=0.0)),
         ("scale_zero", dict(scale=0.0)), ("layout_q_pointer", dict(q=P + 2)), ("layout_kv_stride_l", dict(kv_sl=132)),
         ("layout_kv_row_short", dict(kv_sl=64)), ("layout_q_stride_h", dict(q_sh=4)),
         ("layout_archive_stride", dict(L8=64, k8=P, v8=P, ksc=P, vsc=P, sh8=8200)),
         ("extent_kv_2gib", dict(own=(3, 1024), kv_sl=1 << 20)),
         ("workspace_missing", dict()), ("workspace_too_small", dict(ws=P + 4, ws_bytes=16)),
         ("workspace_misaligned", dict(ws=P + 4, ws_need=True)),
         ("no_shared_rows_workspace", dict(own=(1,) * 4, Hq=14, Ls=0, ks=None, vs=None))]
    rows += [(f"{GROUP}/{name}", GROUP, over) for name, over in g]
    w = [("null_own_rows", dict(brs=False)), ("no_branches", dict(B=0)), ("not_positive", dict(Hq=0)), ("divisibility", dict(Hq=5)),
         ("dtype_f32", dict(dtype="f32")), ("head_dim_64", dict(D=64)), ("envelope_branches", dict(own=(1,) * 9)),
         ("envelope_packed_rows", dict(own=(1,) * 5, Hq=14)), ("branch_without_rows", dict(own=(3, 0))),
         ("l8_negative", dict(L8=-1)), ("ls_negative", dict(Ls=-1)), ("archive_extent", dict(L8=1 << 24)),
         ("shared_keys_extent", dict(Ls=0x40000000))]
    rows += [(f"{GROUP_WS}/{name}", GROUP_WS, over) for name, over in w]
    return rows


ROWS = _rows()


def _refusals(nv):
    got = {}
    for rid, fn, over in ROWS:
        _reset(nv)
        rc = (_call_six if fn in SIX else _call_group)(nv, fn, over)
        got[rid] = [rc, nv.lib.rtk_last_error().decode()]
    return got


def test_every_refusal_returns_the_recorded_code_and_text():
    import retake._native as nv

    assert len({rid for rid, _, _ in ROWS}) == len(ROWS) and {fn for _, fn, _ in ROWS} == set(SIX) | {GROUP, GROUP_WS}
    want = json.load(open(GOLDEN))
    got = _refusals(nv)
    assert sorted(got) == sorted(want)
    for rid, _, _ in ROWS:
        assert got[rid] == want[rid], rid
        # a refusal: an error code (the workspace query's is 0 bytes), never RTK_EHIP - nothing reached the device
        assert got[rid][0] in ((0,) if rid.startswith(GROUP_WS) else (nv.RTK_EINVAL, nv.RTK_EUNSUPPORTED, nv.RTK_EWORKSPACE)), rid


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-retake_amd"))
    import retake._native as nv_

    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(rid)}: {json.dumps(v)}" for rid, v in sorted(_refusals(nv_).items())) + "\n}\n")
    print("recorded", len(ROWS), "refusals in", GOLDEN)

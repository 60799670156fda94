"""rtk_attention_decode_group, the parts that need no GPU: the two entries are declared with the header's signatures,
exported and bound; the workspace query equals the header's formula; the host-side refusals return the stated codes with no
device; the group kernel compiles for gfx950 without scratch; BranchGroup refuses what is not a set of forks of one parent.
The kernel is in tests/test_attention_group_gpu.py, the group of live branches in tests/test_branch_group_gpu.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtk_attention_decode_group_workspace_bytes", "rtk_attention_decode_group"]
T, STEP, TARGET_WG, OWN_KEYS = 32, 128, 512, 512


def _header():
    return open(os.path.join(ROOT, "include", "retake_hip.h")).read()


def test_entry_points_are_declared_exported_and_bound():
    import retake._native as nv
    import test_abi_cpu

    syms = test_abi_cpu._declared_symbols()
    lib = ctypes.CDLL(nv.LIB_PATH)
    for s in NEW:
        assert s in syms and hasattr(lib, s) and s in nv.EXPORTS, s
    assert nv.lib.rtk_version() == nv.ABI_VERSION


def test_bindings_match_the_header():
    """Argument by argument: the C types of the two prototypes and of struct rtk_decode_branch against the ctypes table."""
    import retake._native as nv

    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
             "rtk_stream_t": ctypes.c_void_p}

    def ctype(decl):
        decl = decl.strip()
        if "rtk_decode_branch*" in decl.replace(" *", "*"):
            return ctypes.POINTER(nv.DecodeBranch)
        if decl.startswith("const int*"):
            return ctypes.POINTER(ctypes.c_int)
        if "*" in decl:
            return ctypes.c_void_p
        return kinds[decl.split()[-2]]

    for name in NEW:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", text)
        res, args = nv._SIGNATURES[name]
        assert res is kinds[m.group(1)], name
        assert [ctype(a) for a in m.group(2).split(",")] == list(args), name
    body = re.search(r"typedef struct rtk_decode_branch \{(.*?)\} rtk_decode_branch;", text, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            base = stmt.rsplit("*", 1)[0] + "*" if "*" in stmt else stmt.split()[0]
            for nm in (stmt.rsplit("*", 1)[1] if "*" in stmt else stmt.split(None, 1)[1]).split(","):
                fields.append((nm.strip(), ctypes.c_void_p if "*" in base else {"int64_t": ctypes.c_int64, "int": ctypes.c_int32}[base]))
    assert fields == [(n, t) for n, t in nv.DecodeBranch._fields_]
    assert int(re.search(r"#define RTK_DECODE_GROUP_MAX (\d+)", text).group(1)) == nv.DECODE_GROUP_MAX == 8
    assert int(re.search(r"#define RTK_DECODE_GROUP_OWN_KEYS (\d+)", text).group(1)) == OWN_KEYS


def _formula(own, Hq, Hkv, L8, Ls):
    """include/retake_hip.h: the shared split by the rule of rtk_attention_decode over the padded shared keys, the own
    split every 512 keys."""
    up = lambda a, b: (a + b - 1) // b   # noqa: E731
    keys = up(L8, T) * T + up(Ls, T) * T
    ns = 0
    if keys:
        ns = max(1, min(up(TARGET_WG, Hkv), up(keys, STEP)))
        kps = up(up(keys, ns), STEP) * STEP
        ns = up(keys, kps)
    n_own = max(up(lk, OWN_KEYS) for lk in own)
    return (ns + n_own) * len(own) * Hq * (128 + 2) * 4


def _ws(nv, own, Hq, Hkv, L8, Ls, D=128, dtype=None):
    rows = (ctypes.c_int * len(own))(*own)
    return nv.lib.rtk_attention_decode_group_workspace_bytes(rows, len(own), Hq, Hkv, L8, Ls, D,
                                                             nv.RTK_BF16 if dtype is None else dtype)


def test_workspace_bytes_is_the_headers_formula():
    import retake._native as nv

    for own, (Hq, Hkv), L8, Ls in [((1,), (14, 2), 0, 0), ((1, 33, 130, 600), (14, 2), 45, 1056), ((64,) * 4, (28, 4), 0, 100352),
                                   ((64, 513), (28, 4), 100352, 0), ((5,) * 8, (8, 2), 64, 45), ((1024, 1025, 1), (4, 2), 1, 1),
                                   ((7,), (32, 1), 0, 200000)]:
        assert _ws(nv, own, Hq, Hkv, L8, Ls) == _formula(own, Hq, Hkv, L8, Ls) > 0, (own, Hq, Hkv, L8, Ls)
    # the shared split does not depend on the group: B branches cost B times one branch's partials
    assert _ws(nv, (64,) * 4, 28, 4, 0, 100352) == 4 * _ws(nv, (64,), 28, 4, 0, 100352)
    # outside the envelope: 0, with the reason
    err = nv.lib.rtk_last_error
    assert _ws(nv, (1,) * 5, 14, 2, 0, 64) == 0 and b"packed rows" in err()
    assert _ws(nv, (1,) * 9, 4, 2, 0, 64) == 0 and b"branches" in err()
    assert _ws(nv, (1,), 4, 2, 0, 64, dtype=nv.RTK_F32) == 0 and b"dtype" in err()
    assert _ws(nv, (1,), 4, 2, 0, 64, D=64) == 0 and b"head_dim" in err()
    assert _ws(nv, (1, 0), 4, 2, 0, 64) == 0
    assert _ws(nv, (1,), 4, 2, 0, -1) == 0 and b"Ls" in err()


def test_host_side_validation():
    """Every error before any launch, with no device in the machine."""
    import retake._native as nv

    dummy = (ctypes.c_char * 512)()
    p = (ctypes.addressof(dummy) + 15) & ~15
    err = nv.lib.rtk_last_error

    def c(B=2, q="p", ks="p", k8=None, Ls=64, L8=0, Lk=3, D=128, dtype=nv.RTK_BF16, Hq=4, Hkv=2, kv_sl=128, q_sh=128, out="p",
          scale=0.088):
        brs = (nv.DecodeBranch * B)()
        for br in brs:
            br.q, br.q_stride_h, br.k, br.v = (p if q == "p" else q), q_sh, p, p
            br.kv_stride_h, br.kv_stride_l, br.Lk = 8 * kv_sl, kv_sl, Lk
        ks = p if ks == "p" else ks
        return nv.lib.rtk_attention_decode_group(brs, B, ks, ks, Ls, 64 * 128, 128, k8, k8, k8, k8, L8, 8192, 64,
                                                 p if out == "p" else out, Hq, Hkv, D, dtype, scale, None, 0, None)

    assert nv.lib.rtk_attention_decode_group(None, 1, *([None] * 2), 0, 0, 0, *([None] * 4), 0, 0, 0, p, 4, 2, 128, nv.RTK_BF16,
                                             0.088, None, 0, None) == nv.RTK_EINVAL and b"NULL" in err()
    assert c(out=None) == nv.RTK_EINVAL and b"NULL" in err()
    assert c(B=0) == nv.RTK_EINVAL and b"n_branches" in err()
    assert c(q=None) == nv.RTK_EINVAL and b"branch 0" in err()
    assert c(Lk=0) == nv.RTK_EINVAL and b"Lk 0" in err()
    assert c(Hq=5) == nv.RTK_EINVAL and b"multiple" in err()
    assert c(Ls=-1) == nv.RTK_EINVAL and b"Ls" in err()
    assert c(L8=-1) == nv.RTK_EINVAL
    assert c(ks=None) == nv.RTK_EINVAL and b"shared" in err()
    assert c(L8=64) == nv.RTK_EINVAL and b"archive" in err()
    assert c(scale=0.0) == nv.RTK_EINVAL and b"scale" in err()
    assert c(B=9) == nv.RTK_EUNSUPPORTED and b"9 branches" in err()
    assert c(B=5, Hq=14) == nv.RTK_EUNSUPPORTED and b"packed rows" in err()
    assert c(dtype=nv.RTK_F32) == nv.RTK_EUNSUPPORTED and b"dtype" in err()
    assert c(D=64) == nv.RTK_EUNSUPPORTED and b"head_dim" in err()
    assert c(ks=p + 2) == nv.RTK_EUNSUPPORTED and b"shared" in err()
    assert c(q=p + 2) == nv.RTK_EUNSUPPORTED and b"layout" in err()
    assert c(kv_sl=132) == nv.RTK_EUNSUPPORTED and b"layout" in err()
    assert c(kv_sl=64) == nv.RTK_EUNSUPPORTED and b"layout" in err()
    assert c(q_sh=4) == nv.RTK_EUNSUPPORTED and b"layout" in err()
    assert c() == nv.RTK_EWORKSPACE and b"rtk_attention_decode_group_workspace_bytes" in err()
    assert c(B=4, Hq=14, Ls=0, ks=None) == nv.RTK_EWORKSPACE     # 28 packed rows, no shared rows: accepted as far as the workspace


def test_group_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    """The compiler's resource report of the file's kernels, built with the Makefile's own flags: no scratch, no spill
    in either column-group count of either dtype."""
    src = os.path.join(ROOT, "video-retake_amd", "csrc")
    mk = subprocess.run(["make", "-C", src, "-pn"], check=True, capture_output=True, text=True).stdout
    flags = re.search(r"^CXXFLAGS\s*:?=\s*(.*)$", mk, re.M).group(1).split()
    hipcc = re.search(r"^HIPCC\s*\??=\s*(\S+)$", mk, re.M).group(1)
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(src, "attention_decode.hip"), "-o", str(tmp_path / "attention_decode.elf")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = 0
    for b in blocks:
        if "attn_decode_group_d128_kernel" not in b.split()[0]:
            continue
        seen += 1
        get = lambda what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))   # noqa: E731
        print(b.split()[0], "VGPRs", get("VGPRs"), "LDS", get("LDS Size [bytes/block]"), "scratch", get("ScratchSize [bytes/lane]"))
        assert get("ScratchSize [bytes/lane]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, b
        assert get("Occupancy [waves/SIMD]") >= 2, b
    assert seen == 4


# ---------------------------------------------------------------------------------------------------
# BranchGroup: refusals on adopted (CPU) tensors
# ---------------------------------------------------------------------------------------------------
def _parent():
    import test_fork_cpu

    return test_fork_cpu._adopted(8)


def test_branch_group_takes_forks_of_one_parent_at_one_mark():
    from retake.branch_group import BranchGroup

    p, other = _parent(), _parent()
    m = p.mark()
    a, b = p.fork(m), p.fork(m)
    g = BranchGroup([a, b])
    assert len(g) == 2 and g[1] is b and g.members == [a, b] and g.get_seq_length(0) == 8
    assert g.group_attention_calls == g.group_attention_launches == 0
    with pytest.raises(ValueError, match="at least one"):
        BranchGroup([])
    with pytest.raises(ValueError, match="member 1 is not a branch"):
        BranchGroup([a, p])
    with pytest.raises(ValueError, match="member 2 was forked from another parent"):
        BranchGroup([a, b, other.fork()])
    with pytest.raises(ValueError, match="member 1 was forked from another parent or at another mark"):
        BranchGroup([a, p.fork(p.mark())])
    with pytest.raises(ValueError, match="member 1 is in the group twice"):
        BranchGroup([a, a])
    with pytest.raises(ValueError, match="one row per member"):
        g.attention(torch.zeros(3, 4, 1, 128), 0)
    with pytest.raises(ValueError, match="one new token per member"):
        g.decode_step(torch.zeros(2, 4, 2, 128), None, None, 0, None, None)

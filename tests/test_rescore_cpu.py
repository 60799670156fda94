"""The budget's re-scoring (video_budget_rescore / video_budget_observe_rows), the parts that need no GPU: the invariants of
the float64 restatement (tests/rescore_ref.py), what build_kvcache refuses, that the key off leaves nothing behind, the
argument errors rtk_pivotkv_rescore_batched raises on the host before anything is launched, and the new entry points' place
in the ABI."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch

import rescore_ref as rr

KEY, ROWS = "video_budget_rescore", "video_budget_observe_rows"
ENTRY_POINTS = ("rtk_pivotkv_rescore_workspace_bytes", "rtk_pivotkv_rescore_batched")


def _cfg(top=None, **kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top or {})
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


# ---------------------------------------------------------------------------------------------------
# the reference's own invariants
# ---------------------------------------------------------------------------------------------------
def _operands(seed, Hq, Hkv, Wc, n, D=32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Hq, Wc, D, generator=g) * 1.7, torch.randn(Hkv, n + 3, D, generator=g) * 1.7


@pytest.mark.parametrize("Hq,Hkv,Wc,n", [(4, 2, 8, 33), (28, 4, 3, 129), (8, 8, 5, 7), (16, 1, 4, 64)])
def test_reference_invariants(Hq, Hkv, Wc, n):
    q, k = _operands(1, Hq, Hkv, Wc, n)
    m = rr.mass(q, k, n)
    assert m.dtype == torch.float64 and m.shape == (n,)
    assert abs(m.sum().item() - Wc) < 1e-12 * Wc                     # every query row's probabilities sum to 1
    o = rr.obs(q, k, n)
    assert abs(o.mean().item() - 1.0) < 1e-12                        # what makes scores of different chunks comparable
    old = torch.rand(n + 3) * 2
    new = rr.rescored(old, q, k, n, 0.25)
    assert torch.equal(new[n:], old[n:].double())                    # rows >= n_old keep their arrival score
    assert abs(new[:n].mean().item() - (0.75 * old[:n].double().mean().item() + 0.25)) < 1e-12   # the mean moves to (1 - a) m + a
    assert torch.equal(rr.rescored(old, q, k, n, 1.0)[:n], o)       # alpha = 1 replaces
    assert torch.equal(rr.rescored(old, q, k, 0, 0.5), old.double())  # n_old = 0: nothing
    # rows >= n_old are never read
    k2 = k.clone()
    k2[:, n:] = float("nan")
    assert torch.equal(rr.mass(q, k2, n), m)


def test_one_old_row_observes_one():
    q, k = _operands(2, 4, 2, 8, 1)
    assert torch.equal(rr.obs(q, k, 1), torch.ones(1, dtype=torch.float64))
    assert rr.rescored(torch.tensor([0.25]), q, k, 1, 0.5).item() == 0.625


def test_a_peaked_case_puts_all_mass_on_one_row():
    Hq, Hkv, Wc, n, D = 4, 2, 8, 40, 32
    _, k = _operands(3, Hq, Hkv, Wc, n, D)
    j = 17
    q = torch.stack([4 * k[h // 2, j] for h in range(Hq)])[:, None, :].expand(Hq, Wc, D).contiguous()
    o = rr.obs(q, k, n)
    assert abs(o[j].item() - n) < 1e-9 * n and o.sum().item() == pytest.approx(n, rel=1e-12)
    assert float(torch.cat([o[:j], o[j + 1:]]).max()) < 1e-9


def test_seen_bookkeeping():
    s = rr.Seen()
    assert s.rescore(32) == 0 and s.n_old == 32                      # the first chunk does nothing
    assert s.rescore(64) == 32 and s.n_old == 64
    s.evict(48)
    assert s.rescore(80) == 48
    s.rewind(48)                                                     # a rewind caps it at the restored sc_len
    assert s.n_old == 48 and s.rescore(80) == 48
    s.rewind(100)
    assert s.n_old == 80


# ---------------------------------------------------------------------------------------------------
# build_kvcache
# ---------------------------------------------------------------------------------------------------
def test_key_off_leaves_nothing_behind():
    import retake.longvideo_cache as lc

    for top in ({}, {KEY: None}, {KEY: None, ROWS: 64}, {ROWS: "ignored without the key"},
                {"video_budget_rows": 48, KEY: None}):
        cache = lc.build_kvcache(_cfg(top))
        assert cache.video_budget_rescore is None and cache.budget_rescored == []
        assert "observe_queries" not in cache.memory_footprint()
        st = cache._store(0)
        assert st.oq is None and st.oq_rows == 0 and st.sc_seen == 0 and not st.oq_new
        assert not any("rescore" in name for name in cache._ws)
        with pytest.raises(ValueError, match=KEY):
            cache.observed_queries(0)


def test_key_on():
    import retake.longvideo_cache as lc

    cache = lc.build_kvcache(_cfg({"video_budget_rows": 48, KEY: 0.5}))
    assert cache.video_budget_rescore == 0.5 and cache.video_budget_observe_rows == 64
    assert cache.memory_footprint()["observe_queries"] == 0 and cache.observed_queries(0).numel() == 0
    cache = lc.build_kvcache(_cfg({"video_budget_rows": 48, "video_budget_slack": 8, KEY: 1, ROWS: 3}))
    assert cache.video_budget_rescore == 1.0 and cache.video_budget_observe_rows == 3
    # the options the budget runs beside keep working beside it, the position keys too
    for top, kw in (({"decode_attention": "packed"}, {}), ({}, {"score_rounding": "fast"}), ({}, {"overlap_streams": 2}),
                    ({}, {"flush_every_layers": 1}), ({}, {"pos_embed_reforge": False}),
                    ({"video_position_limit": 100, "video_position_gap": 4}, {})):
        top = dict(top, video_budget_rows=48, **{KEY: 0.25})
        assert lc.build_kvcache(_cfg(top, **kw)).video_budget_rescore == 0.25
    # a fork does not inherit the key (it needs no GPU to see: the branch is built from the same config)
    assert type(cache)(cache.config).video_budget_rescore is None


@pytest.mark.parametrize("top,names", [
    ({KEY: 0.5}, (KEY, "video_budget_rows")),
    ({KEY: 0.5, "video_window_rows": 48}, (KEY, "video_budget_rows", "video_window_rows")),
    ({KEY: 0.5, "video_budget_rows": 48, "kv_cache_dtype": "fp8_e4m3"}, (KEY, "kv_cache_dtype")),
    ({KEY: 0, "video_budget_rows": 48}, (KEY,)),
    ({KEY: 0.0, "video_budget_rows": 48}, (KEY,)),
    ({KEY: -0.5, "video_budget_rows": 48}, (KEY,)),
    ({KEY: 1.5, "video_budget_rows": 48}, (KEY,)),
    ({KEY: 2, "video_budget_rows": 48}, (KEY,)),
    ({KEY: True, "video_budget_rows": 48}, (KEY,)),
    ({KEY: "0.5", "video_budget_rows": 48}, (KEY,)),
    ({KEY: float("nan"), "video_budget_rows": 48}, (KEY,)),
    ({KEY: 0.5, ROWS: 0, "video_budget_rows": 48}, (ROWS,)),
    ({KEY: 0.5, ROWS: -1, "video_budget_rows": 48}, (ROWS,)),
    ({KEY: 0.5, ROWS: 8.0, "video_budget_rows": 48}, (ROWS,)),
    ({KEY: 0.5, ROWS: True, "video_budget_rows": 48}, (ROWS,)),
    ({KEY: 0.5, ROWS: None, "video_budget_rows": 48}, (ROWS,)),
], ids=["no_budget", "window", "fp8", "a0", "a0.0", "a-0.5", "a1.5", "a2", "abool", "astr", "anan", "W0", "W-1", "Wfloat",
        "Wbool", "Wnone"])
def test_refusals_name_their_keys(top, names):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top))
    for name in names:
        assert name in str(ei.value), (name, str(ei.value))


@pytest.mark.parametrize("top,kw,also", [
    ({"video_budget_rows": 48, "video_window_rows": 48}, {}, "video_window_rows"),
    ({"video_budget_rows": 48}, {"defer_rerotation": True}, "defer_rerotation"),
    ({"video_budget_rows": 48}, {"prompt_guided_scoring": True}, "prompt_guided_scoring"),
], ids=["window", "defer_rerotation", "prompt_guided_scoring"])
def test_what_the_budget_refuses_stays_refused(top, kw, also):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(dict(top, **{KEY: 0.5}), **kw))
    assert "video_budget_rows" in str(ei.value) and also in str(ei.value)


# ---------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------
FAKE = 0x10000   # never dereferenced


def _call(unit=None, n_units=1, Hq=28, Hkv=4, W=64, D=128, dt=None, alpha=0.5, qsh=64 * 128, qsl=128, scratch=FAKE,
          stride=1 << 22, **fields):
    import retake._native as nv

    u = nv.RescoreUnit(FAKE, FAKE, 2048 * 128, FAKE, 1000) if unit is None else unit
    for name, value in fields.items():
        setattr(u, name, value)
    return nv.lib.rtk_pivotkv_rescore_batched(C.byref(u), n_units, Hq, Hkv, W, D, nv.RTK_BF16 if dt is None else dt, alpha,
                                              qsh, qsl, scratch, stride, None)


def test_argument_errors_without_a_device():
    import retake._native as nv

    name = b"rtk_pivotkv_rescore_batched"
    need = nv.lib.rtk_pivotkv_rescore_workspace_bytes(28, 4, 64, 1000, 128, nv.RTK_BF16)
    assert need > 0 and need % 256 == 0
    bad = [dict(q=None), dict(k=None), dict(score=None), dict(scratch=None), dict(n=-1), dict(n=(1 << 24) + 1),
           dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=float("nan")), dict(W=0), dict(W=-3),
           dict(Hq=30), dict(Hq=0), dict(Hkv=0), dict(D=0),
           dict(qsl=127), dict(qsh=64), dict(k_stride_h=999 * 128),          # strides too small
           dict(qsl=132), dict(qsh=64 * 128 + 4), dict(k_stride_h=2048 * 128 + 4), dict(q=FAKE + 8), dict(k=FAKE + 2),
           dict(score=FAKE + 2),                                             # matrix path: 16-byte alignment; score: 4
           dict(scratch=FAKE + 128), dict(stride=need + 8), dict(stride=need - 256)]   # scratch misaligned / short
    for kw in bad:
        assert _call(**kw) == nv.RTK_EINVAL, kw
        assert nv.lib.rtk_last_error().startswith(name), kw
    assert _call(stride=need, n=1000 + nv.RESCORE_KEYS) == nv.RTK_EINVAL   # n beyond what the scratch was planned for
    assert _call(dt=nv.RTK_BF16_FAST) == nv.RTK_EUNSUPPORTED
    assert nv.lib.rtk_pivotkv_rescore_batched(None, 1, 28, 4, 64, 128, nv.RTK_BF16, 0.5, 8192, 128, FAKE, need, None) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_rescore_batched(None, -1, 28, 4, 64, 128, nv.RTK_BF16, 0.5, 8192, 128, FAKE, need, None) == nv.RTK_EINVAL
    # nothing to do: success, nothing launched (the stream is NULL and every pointer fake)
    assert nv.lib.rtk_pivotkv_rescore_batched(None, 0, 28, 4, 64, 128, nv.RTK_BF16, 0.5, 8192, 128, None, 0, None) == 0
    assert _call(n=0) == 0 and _call(n=0, q=None, k=None, score=None, stride=0) == 0
    # the generic path takes any alignment of the payload's own
    assert _call(dt=nv.RTK_F32, qsl=132, n=0) == 0
    with pytest.raises(ValueError, match=name.decode()):
        nv.check(_call(alpha=2.0), name.decode())


def test_workspace_bytes():
    import retake._native as nv

    f = nv.lib.rtk_pivotkv_rescore_workspace_bytes
    K = nv.RESCORE_KEYS
    assert K == 512
    # a function of the ranges: constant inside one, a step at its end
    assert f(28, 4, 64, 1, 128, nv.RTK_BF16) == f(28, 4, 64, K, 128, nv.RTK_BF16) < f(28, 4, 64, K + 1, 128, nv.RTK_BF16)
    al = lambda x: (x + 255) & ~255
    assert f(28, 4, 64, 100352, 128, nv.RTK_BF16) == al(4 * 448 * 4) + al(4 * 196 * 448 * 8)      # 14 blocks of 32 rows
    assert f(28, 4, 3, 129, 128, nv.RTK_F16) == al(4 * 32 * 4) + al(4 * 1 * 32 * 8)               # 21 rows pad to a block
    assert f(28, 4, 3, 129, 64, nv.RTK_BF16) == al(4 * 21 * 4) + al(4 * 1 * 21 * 8)               # the generic path does not pad
    assert f(28, 4, 64, 0, 128, nv.RTK_BF16) == al(4 * 448 * 4)
    for args in ((30, 4, 64, 10, 128, nv.RTK_BF16), (28, 4, 0, 10, 128, nv.RTK_BF16), (28, 4, 64, -1, 128, nv.RTK_BF16),
                 (28, 4, 64, 10, 128, nv.RTK_BF16_FAST), (28, 4, 64, (1 << 24) + 1, 128, nv.RTK_BF16)):
        assert f(*args) == 0, args


def test_the_shared_call_path_refuses_under_its_callers_name_before_anything_is_touched():
    """`rescore_groups` (the budget's and the focus's one way to the kernel): a shape the kernel does not serve raises with
    the caller's name, the rows and the room it was sized for - for any group, before the scratch policy is asked for a
    buffer and before a tensor of any entry is looked at (the entries here hold none)."""
    import retake._native as nv
    from retake._video_bound import rescore_groups

    def no_scratch(*_):
        raise AssertionError("a buffer was asked for")

    served, not_served = (0, 28, 4, 16, 128, nv.RTK_BF16), (0, 30, 4, 16, 128, nv.RTK_BF16)
    groups = {served: [(None, None, 0, None, 700)], not_served: [(None, None, 0, None, 5), (None, None, 0, None, 900)]}
    with pytest.raises(ValueError) as e:
        rescore_groups("PivotKVCache.focus", groups, 1.0, 64, no_scratch)
    assert str(e.value) == ("PivotKVCache.focus: rtk_pivotkv_rescore_batched does not serve Hq 30, Hkv 4, 16 query rows, "
                            "900 region rows, head_dim 128")
    with pytest.raises(ValueError) as e:
        rescore_groups("video_budget_rescore", groups, 0.5, 64, no_scratch, room=4096, sized_rows=64)
    assert str(e.value) == ("video_budget_rescore: rtk_pivotkv_rescore_batched does not serve Hq 30, Hkv 4, 64 query rows, "
                            "4096 region rows, head_dim 128")


def test_abi_header_exports_and_library_agree(tmp_path):
    import retake._native as nv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "retake_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in nv.EXPORTS and hasattr(nv.lib, name) and f" {name}(" in header
    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18              # additions only: no signature changed
    assert '"Budget re-scoring"' in header and f"Contents ({len(nv.EXPORTS)} entry points" in header
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rtk_rescore_unit));', '  printf("keys %d\\n", RTK_RESCORE_KEYS);']
    lines += [f'  printf("{n} %zu\\n", offsetof(rtk_rescore_unit, {n}));' for n, _ in nv.RescoreUnit._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(nv.RescoreUnit) == 40 and int(got["keys"]) == nv.RESCORE_KEYS
    for n, _ in nv.RescoreUnit._fields_:
        assert int(got[n]) == getattr(nv.RescoreUnit, n).offset, n

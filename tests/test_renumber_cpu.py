"""video_position_gap (the per-row renumbering of a bounded video region; this project's own rule - the reference has no
counterpart and answer quality is not evaluated), the parts that need no GPU: what build_kvcache accepts and refuses, the
entry point's place in the ABI, the argument errors rtk_pivotkv_renumber_batched raises on the host before any launch, and
the properties of the rule's restatement (tests/renumber_ref.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import rebase_ref as rr
import renumber_ref as nr

LIMIT, GAP = "video_position_limit", "video_position_gap"


def _cfg(top=None, **kw):
    ckw = {"compression_ratio": 0.5, "compression_method": "pivotkv", "pos_embed_reforge": True}
    ckw.update(kw)
    lv = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": ckw}
    lv.update(top or {})
    return types.SimpleNamespace(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs=lv)


def test_the_key_is_off_by_default_and_goes_with_either_bound():
    import retake.longvideo_cache as lc

    for top in ({}, {GAP: None}, {"video_window_rows": 48, LIMIT: 100}, {"video_budget_rows": 48, LIMIT: 0, GAP: None}):
        assert lc.build_kvcache(_cfg(top)).video_position_gap is None
    for bound in ("video_window_rows", "video_budget_rows"):
        for G in (1, 4, 1000):
            cache = lc.build_kvcache(_cfg({bound: 48, LIMIT: 100, GAP: G}))
            assert cache.video_position_gap == G and cache.video_position_limit == 100
            assert int(cache.position_offset(1)) == 0      # before any move: a zero


@pytest.mark.parametrize("top,kw,names", [
    ({GAP: 4}, {}, (LIMIT,)),
    ({GAP: 4, "video_budget_rows": 48}, {}, (LIMIT,)),
    ({GAP: 0, LIMIT: 100, "video_budget_rows": 48}, {}, (LIMIT,)),
    ({GAP: -3, LIMIT: 100, "video_window_rows": 48}, {}, (LIMIT,)),
    ({GAP: 4.0, LIMIT: 100, "video_budget_rows": 48}, {}, (LIMIT,)),
    ({GAP: "4", LIMIT: 100, "video_budget_rows": 48}, {}, (LIMIT,)),
    ({GAP: True, LIMIT: 100, "video_budget_rows": 48}, {}, (LIMIT,)),
], ids=["no_limit", "no_limit_budget", "G0", "G-3", "Gfloat", "Gstr", "Gtrue"])
def test_refusals_of_the_gap_name_both_keys(top, kw, names):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top, **kw))
    msg = str(ei.value)
    assert GAP in msg
    for name in names:
        assert name in msg, (name, msg)


@pytest.mark.parametrize("top,kw,names", [
    ({LIMIT: 100, GAP: 4}, {}, ("video_window_rows", "video_budget_rows")),
    ({LIMIT: 100, GAP: 4, "video_budget_rows": 48}, {"pos_embed_reforge": False}, ("pos_embed_reforge",)),
    ({LIMIT: 100, GAP: 4, "video_budget_rows": 48, "kv_cache_dtype": "fp8_e4m3"}, {}, ("kv_cache_dtype",)),
    ({LIMIT: 100, GAP: 4, "video_window_rows": 48}, {"native_rope": False}, ("native_rope",)),
    ({LIMIT: -1, GAP: 4, "video_window_rows": 48}, {}, ()),
], ids=["no_bound", "no_reforge", "fp8", "called_rope", "P-1"])
def test_every_refusal_of_the_limit_applies_unchanged(top, kw, names):
    import retake.longvideo_cache as lc

    with pytest.raises(ValueError) as ei:
        lc.build_kvcache(_cfg(top, **kw))
    msg = str(ei.value)
    assert LIMIT in msg
    for name in names:
        assert name in msg, (name, msg)


def test_abi_symbol_struct_and_kernel_ids():
    import retake._native as nv

    assert "rtk_pivotkv_renumber_batched" in nv.EXPORTS and hasattr(nv.lib, "rtk_pivotkv_renumber_batched")
    assert nv.lib.rtk_version() == nv.ABI_VERSION      # an addition: no signature changed
    assert C.sizeof(nv.RebaseUnit) == 64 and C.sizeof(nv.RenumberUnit) == 72
    assert [f[0] for f in nv.RenumberUnit._fields_] == [f[0] for f in nv.RebaseUnit._fields_] + ["row_delta"]
    ids = nv.profile_kernel_ids()
    n = nv.lib.rtk_profile_num_kernels()
    assert ids["renumber_scan"] == n - 2 and ids["renumber_apply"] == n - 1 and n <= 32      # appended; the mask has 32 bits
    assert ids["rebase_decide"] == n - 4 and ids["rebase_apply"] == n - 3                    # ... and nothing moved


def test_the_unit_matches_the_header(tmp_path):
    import os
    import subprocess

    import retake._native as nv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retake_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rtk_renumber_unit));', '  printf("tile %d\\n", RTK_RENUMBER_TILE);']
    lines += [f'  printf("{n} %zu\\n", offsetof(rtk_renumber_unit, {n}));' for n, _ in nv.RenumberUnit._fields_]
    lines += [f'  printf("rebase_{n} %zu\\n", offsetof(rtk_rebase_unit, {n}));' for n, _ in nv.RebaseUnit._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(nv.RenumberUnit) and int(got["tile"]) == nv.RENUMBER_TILE
    for n, _ in nv.RenumberUnit._fields_:
        assert int(got[n]) == getattr(nv.RenumberUnit, n).offset, n
    for n, _ in nv.RebaseUnit._fields_:      # the shared fields lie where rtk_rebase_unit has them
        assert got[n] == got["rebase_" + n], n


def test_argument_errors_without_a_device():
    """Every error is raised on the host before any launch: no device is touched (the pointers are never dereferenced)."""
    import retake._native as nv

    fake = 0x100000
    sec = (C.c_int * 3)(16, 24, 24)
    who = b"rtk_pivotkv_renumber_batched"

    def rc(D=128, dtype=nv.RTK_BF16, P=1, inv=fake, nsec=0, limit=0, gap=4, off=fake, delta=fake, n=1, **kw):
        u = nv.RenumberUnit(fake, 1024 * 128 * 2, 5, 100, fake, 1024, 105, 2, 0, fake)
        for name, value in kw.items():
            setattr(u, name, value)
        return nv.lib.rtk_pivotkv_renumber_batched(C.byref(u), n, D, dtype, P, inv, sec if nsec else None, nsec, limit, gap,
                                                   off, delta, None)

    # the re-base's argument errors ...
    for kw in ({"k": None}, {"ids": None}, {"inv": None}, {"off": None}, {"delta": None}, {"first": -1}, {"rows": -1},
               {"end": -1}, {"H": 0}, {"H": -2}, {"slot": -1}, {"k_stride_h": -16}, {"ids_stride": -1}, {"limit": -1},
               {"dtype": 2}, {"dtype": 9}, {"P": 2}, {"first": 106}, {"k_stride_h": 104 * 128 * 2},
               {"P": 3, "nsec": 3, "ids_stride": 100}, {"P": 3}, {"D": 0},
               # ... and the three of its own
               {"gap": 0}, {"gap": -1}, {"rows": 101}, {"rows": 6, "end": 10}, {"row_delta": None}, {"row_delta": fake + 4}):
        assert rc(**kw) == nv.RTK_EINVAL, kw
        assert nv.lib.rtk_last_error().startswith(who), kw
    for kw in ({"k": fake + 8}, {"k_stride_h": 1024 * 128 * 2 + 8}, {"D": 72}, {"D": 24}, {"D": 12, "dtype": nv.RTK_F32},
               {"D": 512}, {"ids": fake + 4}):
        assert rc(**kw) == nv.RTK_EUNSUPPORTED, kw
        assert nv.lib.rtk_last_error().startswith(who), kw
    assert rc(gap=0) == nv.RTK_EINVAL and b"gap" in nv.lib.rtk_last_error()
    assert rc(rows=101) == nv.RTK_EINVAL and b"K rows" in nv.lib.rtk_last_error()
    assert rc(row_delta=None) == nv.RTK_EINVAL and b"row_delta" in nv.lib.rtk_last_error()
    assert rc(P=3, nsec=3, D=64) == nv.RTK_EINVAL and b"mrope_section" in nv.lib.rtk_last_error()
    two = (nv.RenumberUnit * 2)(nv.RenumberUnit(fake, 1 << 20, 5, 100, fake, 1024, 105, 2, 3, fake),
                                nv.RenumberUnit(fake, 1 << 20, 5, 100, fake, 1024, 105, 2, 3, fake + 8192))
    assert nv.lib.rtk_pivotkv_renumber_batched(two, 2, 128, nv.RTK_BF16, 1, fake, None, 0, 0, 4, fake, fake, None) == nv.RTK_EINVAL
    assert b"slot" in nv.lib.rtk_last_error()
    assert nv.lib.rtk_pivotkv_renumber_batched(None, 1, 128, nv.RTK_BF16, 1, fake, None, 0, 0, 4, fake, fake, None) == nv.RTK_EINVAL
    assert nv.lib.rtk_pivotkv_renumber_batched(None, -1, 128, nv.RTK_BF16, 1, fake, None, 0, 0, 4, fake, fake, None) == nv.RTK_EINVAL
    with pytest.raises(NotImplementedError):
        nv.check(rc(D=72), "rtk_pivotkv_renumber_batched")
    # nothing to do: success, nothing launched
    assert nv.lib.rtk_pivotkv_renumber_batched(None, 0, 128, nv.RTK_BF16, 1, fake, None, 0, 0, 4, fake, fake, None) == 0


# ---------------------------------------------------------------------------------------------------
# the rule's restatement
# ---------------------------------------------------------------------------------------------------
def test_the_rule_in_integers():
    t = np.array([0, 1, 2, 3, 4, 50, 51, 60, 61, 61, 99])
    assert nr.excess(t, 5, 11, 4).tolist() == [45, 0, 5, 0, 0, 34]
    assert nr.deltas(t, 5, 11, 4).tolist() == [45, 45, 50, 50, 50, 84]
    d, total = nr.decide(t, 5, 11, 99, 4)
    assert total == 84 and (t[5:] - d).tolist() == [5, 6, 10, 11, 11, 15]
    assert nr.decide(t, 5, 11, 100, 4)[1] == 0 and not nr.decide(t, 5, 11, 100, 4)[0].any()   # the limit is not reached
    assert nr.decide(t, 5, 5, 0, 4)[1] == 0 and len(nr.excess(t, 5, 5, 4)) == 0                # an empty region
    assert nr.decide(t, 0, 5, 0, 1)[1] == 0                                                    # dense from 0: nothing to close
    assert nr.deltas(t + 7, 0, 5, 1).tolist() == [7] * 5                                       # nothing pinned: prev = -1
    assert nr.excess(t, 5, 11, 1).tolist() == [45, 0, 8, 0, 0, 37]
    # K rows stop short of the ids: the ids beyond are renumbered, the K rows beyond are not touched
    ids, K, d, total = nr.renumber(np.stack([t, t + 1000, t + 2000]), np.ones((2, 12, 16)), 5, 11, 4, 99, 4, np.ones(8), [2, 3, 3])
    assert total == 84 and ids[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 10, 11, 11, 15]
    assert np.array_equal(ids[1:], np.stack([t + 1000, t + 2000]))
    assert np.array_equal(K[:, :5], np.ones((2, 5, 16))) and np.array_equal(K[:, 9:], np.ones((2, 3, 16)))
    on = np.concatenate([rr.temporal_pairs(16, 3, [2, 3, 3])] * 2)
    assert np.array_equal(K[:, 5:9][..., ~on], np.ones((2, 4, 12))) and not np.any(K[:, 5:9][..., on] == 1.0)
    assert np.array_equal(K[:, 5], rr.rotate(np.ones((2, 16)), 45, np.ones(8), 3, [2, 3, 3]))
    assert np.array_equal(K[:, 7], rr.rotate(np.ones((2, 16)), 50, np.ones(8), 3, [2, 3, 3]))


def _random_ids(rng, n, first, big=1000):
    """Non-decreasing ids: `first` dense pinned ids, then steps of 0 (rows of one frame), 1, or a hole."""
    step = rng.choice([0, 0, 0, 1, 1, 2, 3, 7, big], size=n)
    step[:first] = 1
    return np.cumsum(step).astype(np.int64) - 1


def test_a_gap_at_or_above_every_inner_gap_is_the_rebase():
    rng = np.random.default_rng(11)
    for trial in range(50):
        first = int(rng.integers(0, 6))
        n = first + int(rng.integers(1, 40))
        t = _random_ids(rng, n, first)
        t[first:] += int(rng.integers(0, 3)) * int(rng.integers(1, 500))      # the gap behind the pinned rows: 0 or open
        G = max(1, int(np.diff(t[first:]).max(initial=0)))
        for limit in (0, int(t[-1]), int(t[-1]) + 1):
            d, total = nr.decide(t, first, n, limit, G)
            want = rr.decide(t, first, n, limit)
            assert total == want and d.tolist() == [want] * (n - first), (trial, limit)
            assert nr.decide(t, first, n, limit, G + 5)[1] == want


def test_the_cap_composes_under_dropping_rows():
    """min(min(x, G) + min(y, G), G) = min(x + y, G) for x, y >= 0: dropping a row later merges two gaps, and renumbering
    before and after the drop gives what renumbering the survivors' unbounded ids gives - a closed form."""
    rng = np.random.default_rng(12)
    for trial in range(50):
        first = int(rng.integers(0, 4))
        n = first + int(rng.integers(3, 30))
        G = int(rng.choice([1, 2, 4, 16]))
        t = _random_ids(rng, n, first)
        d, total = nr.decide(t, first, n, 0, G)
        once = t.copy()
        once[first:] -= d
        keep = np.ones(n, dtype=bool)
        keep[first + rng.choice(n - first - 1, size=int(rng.integers(1, n - first)), replace=False)] = False   # (the last row stays)
        t2, once2 = t[keep], once[keep]
        m = len(t2)
        a = once2.copy()
        a[first:] -= nr.decide(once2, first, m, 0, G)[0]          # renumbered, rows dropped, renumbered again
        b = t2.copy()
        b[first:] -= nr.decide(t2, first, m, 0, G)[0]             # the survivors' unbounded ids renumbered once
        assert np.array_equal(a, b), trial
        # the closed form: the first region id follows the pinned ones, every later step is min(unbounded step, G)
        prev = int(t2[first - 1]) if first else -1
        want = np.concatenate([[min(int(t2[first]), prev + 1)], np.minimum(np.diff(t2[first:]), G)]).cumsum()
        assert np.array_equal(b[first:], want), trial


def test_the_span_bound_and_the_monotone_delta():
    rng = np.random.default_rng(13)
    for trial in range(50):
        first = int(rng.integers(0, 4))
        n = first + int(rng.integers(1, 60))
        G = int(rng.choice([1, 3, 4]))
        t = _random_ids(rng, n, first, big=100_000)
        d, total = nr.decide(t, first, n, 0, G)
        assert np.all(d >= 0) and np.all(np.diff(d) >= 0) and total == (int(d[-1]) if len(d) else 0)
        new = t[first:] - d
        prev = int(t[first - 1]) if first else -1
        assert int(new[0]) <= prev + 1 and int(new[-1]) - int(new[0]) <= (n - first - 1) * G
        assert int(new[-1]) <= prev + 1 + (n - first - 1) * G      # at most 1 + (n - 1) G ids behind the pinned rows


def test_negative_gaps_are_preserved():
    t = np.array([0, 1, 2, 40, 41, 30, 31, 90, 80, 200])
    for G in (1, 4):
        e = nr.excess(t, 3, 10, G)
        assert e[2] == 0 and e[5] == 0                           # 41 -> 30 and 90 -> 80: never "repaired"
        d, total = nr.decide(t, 3, 10, 0, G)
        new = t[3:] - d
        assert new[2] - new[1] == -11 and new[5] - new[4] == -10
        assert np.all(np.diff(d) >= 0) and total == int(d[-1]) > 0
    # an M-RoPE text overlap in front of the region: the first excess is 0, not negative
    assert nr.excess(np.array([0, 1, 2, 2, 2, 9]), 3, 6, 4).tolist() == [0, 0, 3]

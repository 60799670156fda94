"""Prompt-guided PivotKV without a GPU: the invariants of the float64 restatement (tests/prompt_score_ref.py), what
build_kvcache refuses together with prompt_guided_scoring, the hooks' bookkeeping and the host side of the new entry point."""
import types

import pytest
import torch

import prompt_score_ref as ref


def cfg(**extra):
    top = {k: extra.pop(k) for k in ("attention_kernel", "kv_cache_dtype") if k in extra}
    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    kw.update(extra)
    return types.SimpleNamespace(hidden_size=4 * 128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                 longvideo_kwargs={"kvcache_compression": True, "kvcache_compression_kwargs": kw, **top})


@pytest.mark.parametrize("Hq,Hkv,D,Lv,Lp", [(4, 2, 16, 37, 1), (6, 2, 8, 50, 5), (4, 4, 16, 33, 12)])
def test_restatement_scores_are_a_distribution_over_the_video_keys(Hq, Hkv, D, Lv, Lp):
    q, k = ref.operands(1, Hq, Hkv, Lv + Lp, D, torch.float32)
    s = ref.scores(q, k, Lp)
    assert s.shape == (Lv,) and s.dtype == torch.float64
    assert abs(s.sum().item() - 1.0) < 1e-12          # every row's softmax sums to 1 over the video keys
    assert (s > 0).all() and (s < 1).all()            # ... so the mask override's 1.0 ranks first
    # prompt keys and video queries are never read
    q2, k2 = q.clone(), k.clone()
    q2[:, :Lv] = 7.0
    k2[:, Lv:] = -3.0
    assert torch.equal(ref.scores(q2, k2, Lp), s)
    # by hand: one loop per head and prompt row
    G = Hq // Hkv
    want = torch.zeros(Lv, dtype=torch.float64)
    for h in range(Hq):
        for i in range(Lv, Lv + Lp):
            logit = (k[h // G, :Lv].double() @ q[h, i].double()) / D ** 0.5
            want += torch.softmax(logit, 0) / (Lp * G * Hkv)
    assert (s - want).abs().max().item() < 1e-15


def test_restatement_selection_and_ids():
    s = torch.tensor([0.1, 0.4, 0.4, 0.05, 0.3, 0.2, 0.4, 0.01], dtype=torch.float64)
    assert ref.keep_len(0.25, 8) == 2 and ref.keep_len(0.01, 8) == 1 and ref.keep_len(0.25, 7) == 1
    assert ref.select(s, 2).tolist() == [1, 2]                       # ties: lowest index first
    assert ref.select(s, 4).tolist() == [1, 2, 4, 6]
    mask = torch.tensor([0, 0, 0, 1, 0, 0, 0, 1, 1, 1], dtype=torch.bool)   # (entries past Lv belong to prompt rows: unread)
    assert ref.select(s, 3, mask).tolist() == [1, 3, 7]              # key patches first, then by score
    assert ref.threshold_band(s, 4, 0.05).tolist() == [False, False, False, False, True, False, False, False]
    assert ref.threshold_band(s, 4, 0.11).tolist() == [False, True, True, False, True, True, True, False]
    assert ref.threshold_band(s, 3, 0.0, mask).tolist() == [False, True, True, False, False, False, True, False]
    ids = torch.stack([torch.tensor([10, 10, 11, 11, 12, 12, 13, 13, 14, 15]), torch.arange(10), torch.arange(10) + 3])
    kidx = torch.tensor([1, 4, 6])
    assert torch.equal(ref.new_ids(ids, kidx, 8, False), ids[:, kidx])
    got = ref.new_ids(ids, kidx, 8, True)
    # tmin = 10; float32(t - 10) * float32(3 / 8) truncated: 0 -> 0, 2 -> 0, 3 -> 1
    assert got[0].tolist() == [10, 10, 11] and torch.equal(got[1:], ids[1:, kidx])


def test_key_defaults_off_and_hooks_record_the_prompt():
    import retake.longvideo_cache as lc

    off = lc.build_kvcache(cfg())
    assert off.prompt_guided_scoring is False
    off.before_forward(prompt_length=17)
    assert off._prompt_len == 0 and off._prompt_rows(657) == 0       # the reference's `pass`
    # the reference's own switch does not turn the rule on
    assert lc.build_kvcache(cfg(prompt_guided_compression=True)).prompt_guided_scoring is False
    on = lc.build_kvcache(cfg(prompt_guided_scoring=True))
    on.before_forward(prompt_length=17)
    assert on._prompt_rows(657) == 17 and on._prompt_rows(17) == 0 and on._prompt_rows(10) == 0   # 0 < Lp < L only
    on.after_forward()
    assert on._prompt_len == 0
    on.before_forward(prompt_length=None)
    assert on._prompt_rows(657) == 0
    on.before_forward()
    assert on._prompt_rows(657) == 0


@pytest.mark.parametrize("other", [{"score_rounding": "reference"}, {"score_rounding": "fast"},
                                   {"kv_cache_dtype": "fp8_e4m3", "attention_kernel": "hip"}, {"defer_rerotation": True},
                                   {"overlap_streams": 2}, {"flush_every_layers": 4}, {"native_rope": False}])
def test_build_kvcache_refuses_what_the_mode_does_not_serve(other):
    import retake.longvideo_cache as lc

    assert lc.build_kvcache(cfg(**dict(other))) is not None           # fine without the key
    with pytest.raises(ValueError) as e:
        lc.build_kvcache(cfg(prompt_guided_scoring=True, **dict(other)))
    name = next(k for k in other if k != "attention_kernel")
    assert "prompt_guided_scoring" in str(e.value) and name in str(e.value)


def test_entry_point_is_exported_and_checks_its_arguments():
    import retake._native as nv

    assert nv.lib.rtk_version() == nv.ABI_VERSION == 18
    assert "rtk_pivotkv_score_prompt_batched" in nv.EXPORTS and "rtk_pivotkv_score_prompt_workspace_bytes" in nv.EXPORTS
    wsb = nv.lib.rtk_pivotkv_score_prompt_workspace_bytes
    # 16-bit, head_dim 128: one lse per packed row, the G * Lp rows of a KV group padded to 32-row blocks
    assert wsb(28, 4, 201, 1, 128, nv.RTK_BF16) == 4 * 32 * 4              # G * Lp = 7 rows: ONE block per group
    assert wsb(28, 4, 6336, 64, 128, nv.RTK_F16 | nv.RTK_SCORE_MANY_UNITS) == 4 * 14 * 32 * 4
    assert wsb(4, 2, 657, 17, 128, nv.RTK_F32) == 512                      # generic: Hq * Lp floats, 256-byte granules
    assert wsb(6, 2, 338, 5, 64, nv.RTK_BF16) == 256
    assert wsb(4, 2, 17, 17, 128, nv.RTK_F32) == 0 and wsb(4, 3, 100, 5, 128, nv.RTK_F32) == 0
    call = nv.lib.rtk_pivotkv_score_prompt_batched
    fake = 1 << 20   # never dereferenced: every call below is refused before anything is launched
    base = dict(ws=fake, ws_stride=1 << 24, k=None, k_stride=0, score=fake, score_stride=657, scratch=fake,
                scratch_stride=512, n=1, Hq=4, Hkv=2, L=657, Lp=17, D=128, dt=nv.RTK_F32)

    def rc(**kw):
        a = dict(base, **kw)
        return call(a["ws"], a["ws_stride"], a["k"], a["k_stride"], a["score"], a["score_stride"], a["scratch"],
                    a["scratch_stride"], a["n"], a["Hq"], a["Hkv"], a["L"], a["Lp"], a["D"], a["dt"], None, 0, 0, None)

    assert rc(Lp=657) == nv.RTK_EINVAL and rc(Lp=0) == nv.RTK_EINVAL
    assert rc(n=29) == nv.RTK_EINVAL and rc(n=0) == nv.RTK_EINVAL
    assert rc(Hkv=3) == nv.RTK_EINVAL and rc(score=None) == nv.RTK_EINVAL and rc(ws=fake + 16) == nv.RTK_EINVAL
    assert rc(n=2, scratch_stride=256) == nv.RTK_EINVAL and rc(n=2, score_stride=100) == nv.RTK_EINVAL
    for dt in (nv.RTK_BF16_REFROUND, nv.RTK_BF16_FAST, nv.RTK_F16_REFROUND):
        assert rc(dt=dt) == nv.RTK_EUNSUPPORTED

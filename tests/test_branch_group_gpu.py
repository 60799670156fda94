"""BranchGroup on the GPU: forks of one prefilled cache decode a token each through `group.decode_step` - one attention
launch per layer - against TWIN forks of the same parent that take the same steps one at a time through append_pre_rope +
attention (the drivers of tests/test_fork_gpu.py / tests/test_rewind_gpu.py).  The rows, ids and lengths a step leaves are
the twin's bit for bit (it is the same append kernel on the same operands); the attention outputs are held to float64 over
the dense key_cache / value_cache the branch offers, at the bar of tests/test_attention_gpu.py: max(2 E, half an output ulp),
E the eager expression's error on the same tensors.  The group kernel's bits are not the per-branch kernel's (the fp32 sums
are grouped differently), so the twin's float64 error is printed beside the group's, not compared with it.

Shapes: 2 layers, Hq 4 / Hkv 2, D 128; parent TEXT 64 + two chunks of L 512 (320 rows at video_end; fp8 rows: 64 + 256
archived); three branches with questions of 9, 5 and 12 rows; two decode steps.  Five branches at Hq 14 / Hkv 2 (35 packed
rows: two launches) on a text-only parent."""
import types

import pytest
import torch

import attention_ref as ar
import glue_stubs as gs
import synth
import test_fork_gpu as tfg
import test_rewind_gpu as trg
from test_rewind_gpu import LAYERS, D, _same, _state

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
ASKS = ((20, 9), (30, 5), (40, 12))    # (seed, question rows) per branch
STEPS = 2


def dev():
    return torch.device("cuda:0")


def _asked(parent, asks=ASKS):
    """Forks of `parent` at video_end, each with its question prefilled."""
    out = []
    for seed, n in asks:
        d = parent.branch(parent.cache.video_end)
        d.question(seed, n, decode=0)
        out.append(d)
    return out


def _group_inputs(drivers, asks, step, l):
    """The batch a patched model would hand a layer: row b = member b's projections of its step-th decode token (the
    tensors the twin's `step(seed + 1 + step, 1)` feeds) and its position ids."""
    qkv = [trg._qkv(1000 * (seed + 1 + step) + l, 1, d.dtype) for d, (seed, _) in zip(drivers, asks)]
    return tuple(torch.cat([x[i] for x in qkv], dim=0) for i in range(3))


def _bar(q, k, v, what, got, twin=None):
    ref = ar.attention_fp64(q, k, v)
    e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
    bar = max(2.0 * e, ar.half_ulp(q.dtype, ref.abs().max().item()))
    err = (got.double() - ref).abs().max().item()
    terr = float("nan") if twin is None else (twin.double() - ref).abs().max().item()
    print(f"fp64[branch group {what}]: group {err:.3e}  one at a time {terr:.3e}  eager E {e:.3e}  bar {bar:.3e}")
    assert torch.isfinite(got.float()).all() and err <= bar, (what, err, bar)


@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_decode_steps_against_twins(fp8, ids):
    from retake.branch_group import BranchGroup

    p = tfg._make("pre_rope", ids, BF16, 512, 64, fp8)
    members, twins = _asked(p), _asked(p)
    group = BranchGroup([d.cache for d in members])
    assert len(group) == 3 and group[2] is members[2].cache and group.members == [d.cache for d in members]
    assert group.get_seq_length(0) == 320 + 12 and members[0].cache.archive_len(0) == (256 if fp8 else 0)
    for step in range(STEPS):
        pos = [d._text_ids(1) for d in members]
        pos = torch.cat(pos, dim=1 if ids == "mrope" else 0)
        for d, (seed, _) in zip(twins, ASKS):
            d.step(seed + 1 + step, 1)
        for l in range(LAYERS):
            q, k, v = _group_inputs(members, ASKS, step, l)
            out = group.decode_step(q, k, v, l, pos.clone(), p.rot, p.sec)
            assert out.shape == (3, 1, trg.Hq, D) and out.dtype == BF16
            for b, (d, t) in enumerate(zip(members, twins)):
                tq, tk, tv, to = t.log[-LAYERS + l]
                what = ("fp8" if fp8 else "16bit", ids, "step", step, "layer", l, "member", b)
                _same(q[b:b + 1], tq, (what, "rotated q"))
                st = d.cache._layers[l]
                _same(st.k[:, :, :st.length], tk, (what, "own K"))       # (a branch's views are its own rows)
                _same(st.v[:, :, :st.length], tv, (what, "own V"))
                _bar(q[b:b + 1], d.cache.key_cache[l], d.cache.value_cache[l], what, out[b:b + 1], to)
        for b, (d, t) in enumerate(zip(members, twins)):
            tfg._same_observables(d.cache, _state(t.cache), ("after step", step, "member", b))
        assert group.get_seq_length(1) == 320 + 12 + step + 1
    assert group.group_attention_launches == group.group_attention_calls == LAYERS * STEPS
    assert all(d.cache.attention_calls == LAYERS for d in members)       # the question's prefill alone
    # per member: mark / rewind stay the member's own, and the group goes on
    m = members[1].cache.mark()
    q, k, v = _group_inputs(members, ASKS, STEPS, 0)
    pos = torch.cat([d._text_ids(1) for d in members], dim=1 if ids == "mrope" else 0)
    group.decode_step(q, k, v, 0, pos, p.rot, p.sec)
    members[1].cache.rewind(m)
    assert members[1].cache._layers[0].length == 5 + STEPS and members[0].cache._layers[0].length == 9 + STEPS + 1


# ---------------------------------------------------------------------------------------------------
# five branches at G = 7: two launches, the outputs of groups of four and of one
# ---------------------------------------------------------------------------------------------------
def _g7_parent(rows=70):
    import retake.longvideo_cache as lc

    kw = {"compression_ratio": 0.25, "compression_method": "pivotkv", "pos_embed_reforge": True}
    cfg = types.SimpleNamespace(hidden_size=14 * D, num_hidden_layers=LAYERS, num_attention_heads=14, num_key_value_heads=2,
                                longvideo_kwargs={"kvcache_compression": True, "attention_kernel": "hip",
                                                  "kvcache_compression_kwargs": kw})
    cache = lc.build_kvcache(cfg)
    cache.kvcache_compression = False
    rot = synth.RotaryStub(synth.inv_freq(D), trg.A, device=dev())
    _g7_append(cache, rot, 1, rows, 0)
    return cache, rot


def _g7_qkv(seed, n):
    return tuple(torch.from_numpy(x).to(dev()).to(BF16) for x in synth.qkv_chunk(seed, 14, 2, n, D))


def _g7_append(cache, rot, seed, n, t0):
    pos = torch.arange(t0, t0 + n, device=dev()).view(1, 1, n).expand(3, 1, n).contiguous()
    for l in range(LAYERS):
        q, k, v = _g7_qkv(100 * seed + l, n)
        assert cache.append_pre_rope(q, k, v, l, pos.clone(), rot, trg.SEC) is not None


def test_five_branches_at_g7_take_two_launches():
    from retake.branch_group import BranchGroup

    parent, rot = _g7_parent()
    mark = parent.mark()
    brs = [parent.fork(mark) for _ in range(5)]
    for b, br in enumerate(brs):
        _g7_append(br, rot, 10 + b, 3 + 2 * b, 70)
    group = BranchGroup(brs)
    pos = torch.tensor([73 + 2 * b for b in range(5)], device=dev()).view(1, 5, 1).expand(3, 5, 1).contiguous()
    for l in range(LAYERS):
        q, k, v = (torch.cat([_g7_qkv(100 * (20 + b) + l, 1)[i] for b in range(5)], dim=0) for i in range(3))
        out = group.decode_step(q, k, v, l, pos.clone(), rot, trg.SEC)
        assert out.shape == (5, 1, 14, D)
        assert group.group_attention_launches == 2 * (l + 1) and group.group_attention_calls == l + 1
        four, one = BranchGroup(brs[:4]), BranchGroup(brs[4:])
        _same(out[:4], four.attention(q[:4], l), ("groups of four and one", l))
        _same(out[4:], one.attention(q[4:], l), ("groups of four and one", l))
        assert four.group_attention_launches == one.group_attention_launches == 1
        for b, br in enumerate(brs):
            assert br._layers[l].length == 3 + 2 * b + 1
            _bar(q[b:b + 1], br.key_cache[l], br.value_cache[l], ("G7", "layer", l, "member", b), out[b:b + 1])


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    from retake.branch_group import BranchGroup, group_attention_forward

    cfg = ("pre_rope", "mrope", BF16, 512, 64)
    p = tfg.Driver(*cfg).prefill(chunks=1)
    m0 = p.cache.mark()
    p.step(3, 512, video=True)
    ve = p.cache.video_end
    other = tfg._make(*cfg)
    a, b = p.branch(ve), p.branch(ve)
    with pytest.raises(ValueError, match="member 1 was forked from another parent"):
        BranchGroup([a.cache, other.branch(other.cache.video_end).cache])
    with pytest.raises(ValueError, match="member 2 was forked from another parent or at another mark"):
        BranchGroup([a.cache, b.cache, p.cache.fork(p.cache.mark())])
    with pytest.raises(ValueError, match="member 1 is not a branch"):
        BranchGroup([a.cache, p.cache])
    group = BranchGroup([a.cache, b.cache])
    # q_len 2, and a batch of another size, through the patches' helper: before anything is touched
    layer = gs.StubAttention(0, 512, 4, 2, (16, 24, 24), trg.A, seed=3).to_device(dev()).to(BF16).eval()
    pos = torch.full((3, 2, 2), 100, dtype=torch.int64, device=dev())
    before = _state(a.cache)
    with pytest.raises(ValueError, match="one new token per branch"):
        group_attention_forward(layer, torch.zeros((2, 2, 512), dtype=BF16, device=dev()), pos, group, trg.SEC)
    with pytest.raises(ValueError, match="one new token per branch"):
        group_attention_forward(layer, torch.zeros((3, 1, 512), dtype=BF16, device=dev()), pos[:, :, :1], group, trg.SEC)
    tfg._same_observables(a.cache, before, "refused steps")
    # a parent rewound below the fork point: the constructor and every step raise what the branch raises
    p.cache.rewind(m0)
    with pytest.raises(ValueError, match="invalidated"):
        BranchGroup([a.cache, b.cache])
    q, k, v = (torch.cat([x, x], dim=0) for x in trg._qkv(5000, 1, BF16))
    with pytest.raises(ValueError, match="invalidated"):
        group.decode_step(q.clone(), k, v, 0, pos[:, :, :1].clone(), a.rot, a.sec)
    with pytest.raises(ValueError, match="invalidated"):
        group.attention(q, 0)
    assert group.group_attention_launches == 0 and a.cache._layers[0].length == 0


# ---------------------------------------------------------------------------------------------------
# the route through the attention patches (stub modules)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", ["qwen_eager", "qwen_sdpa", "qwen_fa2", "llava"])
def test_patches_take_the_group_route(patch):
    """past_key_value = group, hidden states [3, 1, hidden]: the patch returns o_proj of the group's decode step - the
    projections, `decode_step` and o_proj done by hand on a twin group give the same bits, rows and ids."""
    import retake.llava_onevision as lo
    import retake.qwen2_vl as qv
    from retake.branch_group import BranchGroup

    llava = patch == "llava"
    ids = "plain" if llava else "mrope"
    p = tfg._make("pre_rope", ids, BF16, 512, 64)
    members, twins = _asked(p), _asked(p)
    group, tgroup = BranchGroup([d.cache for d in members]), BranchGroup([d.cache for d in twins])
    layers = [gs.StubAttention(l, 512, 4, 2, None if llava else (16, 24, 24), trg.A, seed=5).to_device(dev()).to(BF16).eval()
              for l in range(LAYERS)]
    x = torch.randn((3, 1, 512), generator=torch.Generator().manual_seed(7)).to(dev()).to(BF16)
    pos = torch.cat([d._text_ids(1) for d in members], dim=0 if llava else 1)
    fwd = {"qwen_eager": qv.retake_Qwen2VLAttention_forward, "qwen_sdpa": qv.retake_Qwen2VLSdpaAttention_forward,
           "qwen_fa2": qv.retake_Qwen2VLFlashAttention2_forward, "llava": lo.retake_Qwen2Attention_forward}[patch]
    with torch.no_grad():
        for l, layer in enumerate(layers):
            if llava:
                got = fwd(layer, x, None, None, past_key_value=group, position_ids=pos.clone())[0]
            else:
                res = fwd(layer, x, None, pos.clone(), group, False, True, None)
                got = res[0]
                assert res[1] is None and res[2] is group
            q = layer.q_proj(x).view(3, 1, 4, D).transpose(1, 2)
            k = layer.k_proj(x).view(3, 1, 2, D).transpose(1, 2)
            v = layer.v_proj(x).view(3, 1, 2, D).transpose(1, 2)
            out = tgroup.decode_step(q, k, v, l, pos.clone(), layer.rotary_emb, None if llava else trg.SEC,
                                     scaling=layer.scaling if llava else None, shift_ids_in_place=not llava)
            _same(got, layer.o_proj(out.reshape(3, 1, -1)), (patch, "layer", l))
            assert got.shape == (3, 1, 512) and torch.isfinite(got.float()).all()
    assert group.group_attention_launches == LAYERS
    for d, t in zip(members, twins):
        tfg._same_observables(d.cache, _state(t.cache), patch)
        assert d.cache._layers[0].length == t.cache._layers[0].length
    with torch.no_grad(), pytest.raises(ValueError, match="one new token per branch"):
        if llava:
            fwd(layers[0], torch.cat([x, x], dim=1), None, None, past_key_value=group, position_ids=pos.repeat(1, 2))
        else:
            fwd(layers[0], torch.cat([x, x], dim=1), None, pos.repeat(1, 1, 2), group, False, True, None)

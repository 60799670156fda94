"""Prompt-guided PivotKV (kvcache_compression_kwargs["prompt_guided_scoring"]) on the GPU: the thin score kernels
(rtk_pivotkv_score_prompt_batched) and the cache that runs them, against the float64 restatement tests/prompt_score_ref.py.

Bars (the project's score bars for the fp32 score arithmetic, applied to Lp * score - a column sum of Lp probabilities, where
the bars were set on sums of L of them): 5e-6 for fp32 operands, 2e-5 for 16-bit operands against the exact score of the
same operands.  A kept set may differ from the float64 top-k only in tokens whose float64 score lies within bar / Lp of the
float64 threshold, at most 1 % of keep of them; the seeds were chosen on the CPU so that the fp32 cases have no such token.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import prompt_score_ref as ref
import rope_ref
import synth

pytestmark = pytest.mark.gpu

A = synth.YARN_FACTOR4_ATTENTION_SCALING
RATIO = 0.25
BAR = {torch.float32: 5e-6, torch.bfloat16: 2e-5, torch.float16: 2e-5}


def dev():
    return torch.device("cuda:0")


def al256(n):
    return (n + 255) & ~255


def run_kernel(qs, ks, Lp, q_tensors=None, packed=False):
    """rtk_pivotkv_score_prompt_batched on n units (q~ [Hq, L, D], k~ [Hkv, L, D] device tensors of one shape): one call,
    -> [n, L] fp32 scores (entries >= Lv keep their NaN filler).  packed: q~ / k~ are copied into score workspaces laid out
    as the prepare kernels leave them; else k~ by pointer and the queries through `q_tensors` ([Hq, L, D] views of any
    head / row strides, read in place)."""
    import retake._native as nv

    n = len(qs)
    Hq, L, D = qs[0].shape
    Hkv = ks[0].shape[0]
    dt = nv.dtype_code(qs[0])
    es = qs[0].element_size()
    score = torch.full((n, L), float("nan"), dtype=torch.float32, device=dev())
    sb = nv.lib.rtk_pivotkv_score_prompt_workspace_bytes(Hq, Hkv, L, Lp, D, dt)
    assert sb > 0 and sb % 256 == 0
    scratch = torch.empty(n * sb + 256, dtype=torch.uint8, device=dev())
    scratch_p = al256(scratch.data_ptr())
    keep_alive = [scratch]
    if packed:
        stride = al256(nv.lib.rtk_pivotkv_score_workspace_bytes(Hq, Hkv, L, D, dt))
        k_off = al256(Hq * L * D * es)
        ws = torch.zeros(n * stride + 256, dtype=torch.uint8, device=dev())
        base = al256(ws.data_ptr()) - ws.data_ptr()
        for u in range(n):
            o = base + u * stride
            ws[o:o + Hq * L * D * es].copy_(qs[u].contiguous().view(torch.uint8).reshape(-1))
            ws[o + k_off:o + k_off + Hkv * L * D * es].copy_(ks[u].contiguous().view(torch.uint8).reshape(-1))
        args = (C.c_void_p(ws.data_ptr() + base), stride, None, 0)
        qarg = (None, 0, 0)
        keep_alive.append(ws)
    else:
        kk = torch.stack([k.contiguous() for k in ks])
        qt = q_tensors if q_tensors is not None else [q.contiguous() for q in qs]
        assert all(t.stride() == qt[0].stride() and t.stride(2) == 1 for t in qt)
        args = (None, 0, nv.ptr(kk), Hkv * L * D * es)
        qarg = ((C.c_void_p * n)(*[t.data_ptr() for t in qt]), qt[0].stride(0), qt[0].stride(1))
        keep_alive += [kk, qt]
    nv.check(nv.lib.rtk_pivotkv_score_prompt_batched(*args, nv.ptr(score), L, C.c_void_p(scratch_p), sb, n, Hq, Hkv, L, Lp, D,
                                                     dt, *qarg, nv.stream()), "rtk_pivotkv_score_prompt_batched")
    torch.cuda.synchronize()
    del keep_alive
    return score


def device_select(score, Lv, keep):
    """The library's selection (rtk_pivotkv_select) over the Lv video columns of a score row -> kept indices, ascending."""
    import retake._native as nv

    s = score[:Lv].clone()
    keep_idx = torch.empty(keep, dtype=torch.int64, device=dev())
    rank = torch.empty(Lv, dtype=torch.int32, device=dev())
    nb = nv.lib.rtk_pivotkv_select_workspace_bytes(Lv)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev())
    nv.check(nv.lib.rtk_pivotkv_select(nv.ptr(s), None, Lv, keep, None, 0, 0, nv.ptr(keep_idx), nv.ptr(rank), None, 0,
                                       C.c_void_p(al256(ws.data_ptr())), nb, nv.stream()), "rtk_pivotkv_select")
    torch.cuda.synchronize()
    return keep_idx


def check_scores(name, got, q, k, Lp, dtype):
    """Bar on Lp * score against float64, untouched tail, kept set against the float64 top-k.  Prints the measured maxima."""
    L = q.shape[1]
    Lv = L - Lp
    bar = BAR[dtype]
    want = ref.scores(q, k, Lp)
    err = (got[:Lv].double() - want).abs().max().item() * Lp
    assert torch.isnan(got[Lv:]).all(), "entries >= Lv were written"
    assert (got[:Lv] < 1).all() and (got[:Lv] > 0).all()
    keep = ref.keep_len(RATIO, Lv)
    band = ref.threshold_band(want, keep, bar / Lp)
    allowed = keep // 100 if dtype != torch.float32 else 0
    near = int(band.sum().item()) - 1          # (the threshold token itself is always in the band)
    assert near <= allowed, f"{name}: {near} tokens within bar / Lp of the float64 threshold: choose another seed"
    kept64 = set(ref.select(want, keep).tolist())
    kept = set(device_select(got, Lv, keep).tolist())
    diff = kept64 ^ kept
    print(f"prompt_score {name}: max |Lp*(score - float64)| = {err:.3e} (bar {bar:.0e}), kept set differs in {len(diff)} of "
          f"{keep} (tokens near the threshold: {near})")
    assert err < bar
    assert all(band[j] for j in diff) and len(diff) <= allowed
    return err


KERNEL_CASES = [   # dtype, Hq, Hkv, D, Lv, Lp, seed (chosen on the CPU: see the module docstring)
    (torch.bfloat16, 28, 4, 128, 200, 1, 2),
    (torch.bfloat16, 28, 4, 128, 640, 17, 4),
    (torch.float16, 4, 2, 128, 1000, 64, 1),
    (torch.bfloat16, 28, 4, 128, 2304, 130, 1),
    (torch.float32, 4, 2, 128, 640, 17, 1),
    (torch.float32, 6, 2, 64, 333, 5, 1),
]


@pytest.mark.parametrize("dtype,Hq,Hkv,D,Lv,Lp,seed", KERNEL_CASES)
def test_kernel_against_float64(dtype, Hq, Hkv, D, Lv, Lp, seed):
    q, k = (t.to(dev()) for t in ref.operands(seed, Hq, Hkv, Lv + Lp, D, dtype))
    got = run_kernel([q], [k], Lp)[0]
    again = run_kernel([q], [k], Lp)[0]
    assert torch.equal(got[:Lv], again[:Lv]), "two runs differ"
    check_scores(f"{str(dtype)[6:]} {Hq}/{Hkv} D={D} Lv={Lv} Lp={Lp}", got, q, k, Lp, dtype)


def test_kernel_three_units_one_launch():
    """Three bf16 units in one call: from packed workspaces (q~ at offset 0, k~ behind it), and with k~ by pointer and the
    queries read where they lie through strides - unit 1's queries are a tensor of their own in the projection layout
    [L, Hq, D] (head stride D, row stride Hq * D), like the pre-RoPE queries the prologue route scores in place."""
    dtype, Hq, Hkv, D, Lv, Lp = torch.bfloat16, 28, 4, 128, 640, 17
    L = Lv + Lp
    ops = [tuple(t.to(dev()) for t in ref.operands(seed, Hq, Hkv, L, D, dtype)) for seed in (4, 9, 11)]
    qs, ks = [o[0] for o in ops], [o[1] for o in ops]
    packed = run_kernel(qs, ks, Lp, packed=True)
    both = torch.empty((2, L, Hq, D), dtype=dtype, device=dev())
    own = torch.empty((L, Hq, D), dtype=dtype, device=dev())
    views = [both[0].transpose(0, 1), own.transpose(0, 1), both[1].transpose(0, 1)]
    for v, q in zip(views, qs):
        v.copy_(q)
    strided = run_kernel(qs, ks, Lp, q_tensors=views)
    assert torch.equal(packed[:, :Lv], strided[:, :Lv]), "packed and in-place queries give different bits"
    assert torch.equal(strided[:, :Lv], run_kernel(qs, ks, Lp, q_tensors=views)[:, :Lv]), "two runs differ"
    for u in range(3):
        assert torch.isnan(packed[u, Lv:]).all()
        want = ref.scores(qs[u], ks[u], Lp)
        err = (strided[u, :Lv].double() - want).abs().max().item() * Lp
        print(f"prompt_score batched unit {u}: max |Lp*(score - float64)| = {err:.3e} (bar {BAR[dtype]:.0e})")
        assert err < BAR[dtype]
        assert torch.equal(strided[u, :Lv], run_kernel([qs[u]], [ks[u]], Lp)[0, :Lv]), "a unit's bits depend on its neighbours"


# ------------------------------------------------------------------------------------------------------------------
# the cache
# ------------------------------------------------------------------------------------------------------------------
SEC = [16, 24, 24]
TEXT, CHUNKS = 17, ((640, 17), (640, 17), (144, 17))
LAYERS = 2
# synth.qkv_chunk seeds of the (chunk, layer) units, chosen on the CPU: with these no float64 score (of the pre-RoPE
# operands, mask of chunk 1 applied) lies within 4 * bar / Lp of the threshold, so the kept sets have to be the float64
# top-k exactly - also after the fp32 un-rotation round trip, which moves a score by ~1e-8
UNIT_SEEDS = {torch.float32: ((100, 110), (200, 210), (300, 310)), torch.bfloat16: ((107, 111), (200, 211), (300, 310))}


def cfg(Hq, Hkv, D, reforge, **extra):
    kw = {"compression_ratio": RATIO, "compression_method": "pivotkv", "pos_embed_reforge": reforge}
    top = {k: extra.pop(k) for k in ("attention_kernel",) if k in extra}
    kw.update(extra)
    return types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq, num_key_value_heads=Hkv,
                                 longvideo_kwargs={"kvcache_compression": True, "kvcache_compression_kwargs": kw, **top})


def chunk_ids(c, Lv, Lp, ids):
    """The chunk's ids before the continuity shift: video rows, then the prompt's text rows (one id on every axis)."""
    if ids == "mrope":
        v = synth.mrope_position_ids(3 + 11 * c, Lv // 64, 8, 8, hw0=2) if Lv % 64 == 0 else \
            synth.mrope_position_ids(3 + 11 * c, Lv // 16, 4, 4, hw0=2)
        p = np.broadcast_to(np.arange(Lp, dtype=np.int64) + v.max() + 1, (3, 1, Lp))
        return torch.from_numpy(np.concatenate([v, p], axis=-1)).to(dev())
    return (torch.arange(Lv + Lp, device=dev()) + 50 + 1000 * c).view(1, Lv + Lp)


def unit_operands(cache, layer):
    """(q~ [Hq, L, D], k~ [Hkv, L, D]) of the layer's pending unit as the prepare / prologue kernels left them for the
    score passes: queries kept in place or the packed copy at offset 0 of the slot's workspace; k~ in the slot's
    un-rotated rows (reforge) or packed behind q~."""
    b = cache._batch
    sl = b.slot(layer)
    Hq, Hkv, L, D, es = b.Hq, b.Hkv, b.L, b.D, b.esize
    ws = b.score_ws[(b.score_ws_base - b.score_ws.data_ptr()) + sl * b.ws_stride:]
    q = b.q_keep[sl][0] if b.q_keep[sl] is not None else ws[:Hq * L * D * es].view(b.dtype).view(Hq, L, D)
    k = b.k_unrot[sl] if b.reforge else ws[al256(Hq * L * D * es):][:Hkv * L * D * es].view(b.dtype).view(Hkv, L, D)
    return q.clone(), k.clone()


CACHE_CASES = [   # dtype, Hq, Hkv, ids ("mrope" [3,1,L] / "plain" [1,L] with reforge, None: reforge off), route, extra options
    (torch.float32, 4, 2, "mrope", "update", {}),
    (torch.float32, 4, 2, "plain", "update", {}),
    (torch.float32, 4, 2, None, "update", {}),
    (torch.float32, 4, 2, "mrope", "pre_rope", {}),
    (torch.float32, 4, 2, "plain", "pre_rope", {}),
    (torch.bfloat16, 28, 4, None, "update", {}),
    (torch.bfloat16, 28, 4, "mrope", "pre_rope", {"prologue_operands": "pre_rope"}),   # queries scored where they lie
]


@pytest.mark.parametrize("dtype,Hq,Hkv,ids,route,extra", CACHE_CASES)
def test_cache_prompt_guided(dtype, Hq, Hkv, ids, route, extra):
    """A 17-token text prefix, two chunks of 640 video + 17 prompt rows, a tail chunk of 144 + 17, two layers: lengths,
    ids, kept V / K rows, continuity, the mask override and the diagnostics against the restatement run on the operands the
    prepare / prologue kernels produced."""
    import retake.longvideo_cache as lc

    D = 128
    reforge = ids is not None
    P = {"mrope": 3, "plain": 1, None: 0}[ids]
    sec = SEC if ids == "mrope" else None
    inv = synth.inv_freq(D)
    rot = synth.RotaryStub(inv, A, device=dev())
    cache = lc.build_kvcache(cfg(Hq, Hkv, D, reforge, prompt_guided_scoring=True, **extra))
    bar = BAR[dtype]
    g = torch.Generator(device=dev()).manual_seed(5)

    def rand(h, n):   # the projection layout: [1, n, h*D] memory, [1, h, n, D] view
        return (1.7 * torch.randn((1, n, h, D), generator=g, device=dev())).to(dtype).transpose(1, 2)

    def projection(x):   # [1, h, n, D] fp32 numpy -> the same layout
        return torch.from_numpy(x).to(dev()).to(dtype).transpose(1, 2).contiguous().transpose(1, 2)

    # text prefix, compression off
    cache.kvcache_compression = False
    tpos = torch.arange(TEXT, device=dev()).view(1, TEXT)
    tpos = tpos.expand(3, TEXT).reshape(3, 1, TEXT).contiguous() if ids == "mrope" else tpos
    want_ids = [tpos.reshape(max(P, 1), TEXT).clone() for _ in range(LAYERS)]
    want_k, want_v, k_bound = [[] for _ in range(LAYERS)], [[] for _ in range(LAYERS)], [[] for _ in range(LAYERS)]
    for l in range(LAYERS):
        kt, vt = rand(Hkv, TEXT), rand(Hkv, TEXT)
        cache.update(kt, vt, l, {"position_ids": tpos.clone()} if reforge else {})
        want_k[l].append(kt[0].float().cpu())
        want_v[l].append(vt[0])
        k_bound[l].append(torch.zeros((Hkv, TEXT, D)))
    cache.kvcache_compression = True
    total = TEXT
    for c, (Lv, Lp) in enumerate(CHUNKS):
        L = Lv + Lp
        keep = ref.keep_len(RATIO, Lv)
        pos = chunk_ids(c, Lv, Lp, ids) if reforge else None
        mask = None
        if c == 1:   # key patches: fewer than keep, so every one of them has to be kept
            mask = torch.from_numpy(np.random.default_rng(3).uniform(size=Lv) < 0.1).to(dev())
            assert 0 < int(mask.sum()) <= keep
        cache.keypatches_mask_chunk = mask
        cache.before_forward(prompt_length=Lp)
        units = []
        for l in range(LAYERS):
            q0, k0, v0 = (projection(x) for x in synth.qkv_chunk(UNIT_SEEDS[dtype][c][l], Hq, Hkv, L, D))
            prev = cache.get_prev_temporal_idx(l) if reforge else -1
            assert int(prev) == int(want_ids[l][0, -1]) or not reforge, "continuity does not start from the last kept id"
            P0 = cache.get_seq_length(l)
            assert P0 == total
            out = None
            if route == "pre_rope":
                out = cache.update_pre_rope(q0, k0, v0, l, pos, rot, sec, shift_ids_in_place=ids == "mrope")
                assert (out is not None) == (L >= 512), "the prologue route serves chunks of 512 rows and more"
            if out is not None:
                _, K, V = out
            else:
                p_l = pos
                if reforge:
                    p_l = cache.shift_temporal_ids_(pos if ids == "mrope" else pos.clone(), l)
                    q = synth.rope_forward(q0.float(), p_l, rot, sec).to(dtype)
                    k = synth.rope_forward(k0.float(), p_l, rot, sec).to(dtype)
                else:
                    q, k = q0, k0
                kw = {"query_states": q, "rotary_emb": rot, "mrope_section": sec}
                if reforge:
                    kw["position_ids"] = p_l
                K, V = cache.update(k, v0, l, kw)
            # what the layer's attention sees is unchanged: [prefix | all L rows]
            assert K.shape[2] == V.shape[2] == P0 + L and torch.equal(V[:, :, P0:], v0)
            assert cache.get_seq_length(l) == P0 + keep
            b = cache._batch
            assert b.prompt == Lp and b.keep == keep
            qt, kt = unit_operands(cache, l)
            chunk_pos = b.pos_old[b.slot(l)].clone() if reforge else None
            if reforge:   # the shifted ids start one past the last kept id of the previous chunk
                assert int(chunk_pos[0, 0]) == int(want_ids[l][0, -1]) + 1
            units.append((qt, kt, chunk_pos, K[0, :, P0:].clone(), v0[0].clone()))
        n_ev = list(cache.num_evicted_tokens)
        last_scores, last_keep = cache.last_scores.clone(), cache.last_keep_indices.clone()   # (flushes)
        cache.after_forward()
        assert cache._prompt_len == 0
        assert last_scores.shape == (Lv,) and last_keep.shape == (keep,) and int(last_keep.max()) < Lv
        for l, (qt, kt, chunk_pos, k_rows, v_rows) in enumerate(units):
            s64 = ref.scores(qt, kt, Lp)
            near = int(ref.threshold_band(s64, keep, bar / Lp, mask).sum().item()) - 1
            assert near <= 0, f"chunk {c} layer {l}: {near} tokens within bar / Lp of the float64 threshold: choose another seed"
            kidx = ref.select(s64, keep, mask)
            if mask is not None:
                assert set(torch.nonzero(mask).flatten().tolist()) <= set(kidx.tolist())
            if l == LAYERS - 1:
                shown = s64.clone()   # last_scores is the score row after the selection's in-place mask override (as ever)
                if mask is not None:
                    shown[mask] = 1.0
                err = (last_scores.double() - shown).abs().max().item() * Lp
                print(f"prompt_score cache {str(dtype)[6:]} {ids} {route} chunk {c}: max |Lp*(score - float64)| = {err:.3e}")
                assert err < bar and torch.equal(last_keep, kidx)
            want_v[l].append(v_rows[:, kidx])
            if reforge:
                nid = ref.new_ids(chunk_pos, kidx, Lv, True)
                want_ids[l] = torch.cat([want_ids[l], nid], dim=1)
                # kept K = k~ re-rotated at the new ids (tests/rope_ref.py): float64 truth at the kernels' fp32 angles
                ang = rope_ref.angles(nid.cpu().numpy(), inv, D, sec)
                truth, mag = rope_ref.rotate_truth(kt[:, kidx].cpu(), ang, A)
                want_k[l].append(torch.from_numpy(truth).float())
                k_bound[l].append(torch.from_numpy(rope_ref.rotate_bound(dtype, mag)).float())
            else:
                want_k[l].append(k_rows[:, kidx].float().cpu())
                k_bound[l].append(torch.zeros((Hkv, keep, D)))
        total += keep
        assert cache.num_evicted_tokens == n_ev
    cache.keypatches_mask_chunk = None
    assert total == TEXT + sum(ref.keep_len(RATIO, lv) for lv, _ in CHUNKS)
    for l in range(LAYERS):
        assert cache.get_seq_length(l) == total
        assert cache.num_evicted_tokens[l] == sum(lv + lp - ref.keep_len(RATIO, lv) for lv, lp in CHUNKS)
        assert torch.equal(cache.value_cache[l][0], torch.cat(want_v[l], dim=1)), "V rows are not bit-exact gathers"
        got_k, wk, bound = cache.key_cache[l][0].float().cpu(), torch.cat(want_k[l], dim=1), torch.cat(k_bound[l], dim=1)
        if not reforge:
            assert torch.equal(got_k, wk), "K rows are not bit-exact gathers"
        else:
            kerr = (got_k - wk).abs()
            if dtype == torch.float32:
                assert kerr.max().item() <= 1e-5, f"kept K off by {kerr.max().item():.3e}"
            assert (kerr <= bound + 1e-30)[:, TEXT:].all() and torch.equal(got_k[:, :TEXT], wk[:, :TEXT])
            pc = cache.position_cache[l]
            assert pc.shape[-1] == total and torch.equal(pc.reshape(P, total), want_ids[l])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_native_attention_sees_the_whole_chunk(dtype):
    """attention_kernel="hip": during a prompt-guided chunk the native attention over [prefix | L rows] returns the bits
    it returns with the key off."""
    import retake.longvideo_cache as lc

    Hq, Hkv, D, (Lv, Lp) = 28, 4, 128, CHUNKS[0]
    L = Lv + Lp
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    g = torch.Generator(device=dev()).manual_seed(8)
    t = {n: (1.7 * torch.randn((1, L if n != "kt" and n != "vt" else TEXT, h, D), generator=g, device=dev())).to(dtype).transpose(1, 2)
         for n, h in (("q", Hq), ("k", Hkv), ("v", Hkv), ("kt", Hkv), ("vt", Hkv))}
    outs = []
    for on in (True, False):
        cache = lc.build_kvcache(cfg(Hq, Hkv, D, True, attention_kernel="hip", prompt_guided_scoring=on))
        cache.kvcache_compression = False
        tpos = torch.arange(TEXT, device=dev()).expand(3, TEXT).reshape(3, 1, TEXT).contiguous()
        cache.update(t["kt"], t["vt"], 0, {"position_ids": tpos})
        cache.kvcache_compression = True
        pos = chunk_ids(0, Lv, Lp, "mrope")
        cache.before_forward(prompt_length=Lp)
        cache.shift_temporal_ids_(pos, 0)
        q = synth.rope_forward(t["q"].float(), pos, rot, SEC).to(dtype)
        k = synth.rope_forward(t["k"].float(), pos, rot, SEC).to(dtype)
        K, V = cache.update(k, t["v"], 0, {"query_states": q, "position_ids": pos, "rotary_emb": rot, "mrope_section": SEC})
        assert K.shape[2] == TEXT + L
        out = cache.attention(q, K, V, layer_idx=0)
        assert out is not None and cache.attention_calls == 1
        outs.append(out.clone())
        cache.after_forward()
        assert cache.get_seq_length(0) == TEXT + ref.keep_len(RATIO, Lv if on else L)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("key", [None, False])
def test_off_means_off(key):
    """With prompt_guided_scoring absent or False, before_forward(prompt_length=17) changes nothing: the cache is
    bit-identical to the same run without the hook call (passes with and without the feature)."""
    import retake.longvideo_cache as lc

    Hq, Hkv, D, L, dtype = 28, 4, 128, 657, torch.bfloat16
    rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
    extra = {} if key is None else {"prompt_guided_scoring": key}
    caches = []
    for hook in (True, False):
        cache = lc.build_kvcache(cfg(Hq, Hkv, D, True, **extra))
        g = torch.Generator(device=dev()).manual_seed(21)
        for c in range(2):
            pos = chunk_ids(c, 640, 17, "mrope")
            if hook:
                cache.before_forward(prompt_length=17)
            for l in range(LAYERS):
                q0, k0, v0 = ((1.7 * torch.randn((1, L, h, D), generator=g, device=dev())).to(dtype).transpose(1, 2)
                              for h in (Hq, Hkv, Hkv))
                cache.shift_temporal_ids_(pos, l)
                q = synth.rope_forward(q0.float(), pos, rot, SEC).to(dtype)
                k = synth.rope_forward(k0.float(), pos, rot, SEC).to(dtype)
                cache.update(k, v0, l, {"query_states": q, "position_ids": pos, "rotary_emb": rot, "mrope_section": SEC})
            cache.after_forward()
        caches.append(cache)
    a, b = caches
    keep = int(RATIO * L)
    for l in range(LAYERS):
        assert a.get_seq_length(l) == b.get_seq_length(l) == 2 * keep
        assert torch.equal(a.key_cache[l], b.key_cache[l]) and torch.equal(a.value_cache[l], b.value_cache[l])
        assert torch.equal(a.position_cache[l], b.position_cache[l])
    assert a.num_evicted_tokens == b.num_evicted_tokens
    assert torch.equal(a.last_scores, b.last_scores) and torch.equal(a.last_keep_indices, b.last_keep_indices)

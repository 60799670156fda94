"""PivotKVCache.mark / rewind / crop on the GPU: every case is a TWIN comparison, bit for bit, against the existing code path
run on a fresh cache - never against the code under test.

Cache A: prefill (5 text rows, two video chunks), mark, question 1 (7 rows) + 3 decode steps, rewind, question 2 (9 rows) + 3
decode steps.  Cache B, fresh: the same prefill, question 2 + its decode steps.  Equal afterwards: key_cache / value_cache /
position_cache of every layer, num_evicted_tokens, get_seq_length, get_prev_temporal_idx, the K / V views every call of the
second question returned and its attention outputs (attention_kernel="hip").

Shapes: 2 layers, Hq 4, Hkv 2, D 128, ratio 0.25; L 512 (the one-call rtk_pivotkv_update / update_pre_rope route) and L 64
(stage by stage, the one-workgroup selection).  Inputs from tests/synth.py."""
import functools
import gc
import types

import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

LAYERS, Hq, Hkv, D, RATIO = 2, 4, 2, 128, 0.25
SEC = [16, 24, 24]
A = synth.YARN_FACTOR4_ATTENTION_SCALING
TEXT, Q1, Q2, DECODE, LP = 5, 7, 9, 3, 16


def dev():
    return torch.device("cuda:0")


def _cfg(reforge=True, fp8=False, **extra):
    kw = {"compression_ratio": RATIO, "compression_method": "pivotkv", "pos_embed_reforge": reforge}
    kw.update(extra)
    top = {"kvcache_compression": True, "attention_kernel": "hip", "kvcache_compression_kwargs": kw}
    if fp8:
        top["kv_cache_dtype"] = "fp8_e4m3"
    return types.SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=LAYERS, num_attention_heads=Hq,
                                 num_key_value_heads=Hkv, longvideo_kwargs=top)


@functools.lru_cache(maxsize=None)
def _qkv(seed, n, dtype):
    """Pre-RoPE projections of one (step, layer) in the projection layout ([1, n, h * D] memory, [1, h, n, D] view); made
    once and shared by every cache and case - nothing writes them (the callers clone what a kernel rotates in place)."""
    return tuple(torch.from_numpy(x).to(dev()).to(dtype).transpose(1, 2).contiguous().transpose(1, 2)
                 for x in synth.qkv_chunk(seed, Hq, Hkv, n, D))


def _bits(t):
    if t.dtype in (torch.float32,):
        return t.contiguous().view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16)
    return t


def _same(x, y, what):
    if isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor):
        assert isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor), what
        assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
        assert torch.equal(_bits(x), _bits(y)), what
    else:
        assert x == y, (what, x, y)


def _state(cache):
    """Every observable of the twin rule, cloned."""
    out = {"num_evicted": list(cache.num_evicted_tokens), "layers": len(cache),
           "pos": [p.clone() if isinstance(p, torch.Tensor) else p for p in cache.position_cache]}
    for l in range(len(cache)):
        k, v = cache.key_cache[l], cache.value_cache[l]
        out[f"k{l}"] = k.clone() if isinstance(k, torch.Tensor) else k
        out[f"v{l}"] = v.clone() if isinstance(v, torch.Tensor) else v
        out[f"len{l}"] = cache.get_seq_length(l)
        prev = cache.get_prev_temporal_idx(l)
        out[f"prev{l}"] = int(prev)
        out[f"len8_{l}"] = cache.archive_len(l)
        if cache.archive_len(l):
            for name, t in zip(("k8", "v8", "ks8", "vs8"), cache.archive(l)):
                out[f"{name}_{l}"] = t.clone()
    return out


def _same_state(a, b, what=""):
    a, b = (x if isinstance(x, dict) else _state(x) for x in (a, b))
    assert a.keys() == b.keys(), (what, sorted(a.keys() ^ b.keys()))
    for key in a:
        if isinstance(a[key], list) and key == "pos":
            assert len(a[key]) == len(b[key]), (what, key)
            for i, (x, y) in enumerate(zip(a[key], b[key])):
                _same(x, y, (what, key, i))
        else:
            _same(a[key], b[key], (what, key))


def _same_log(a, b, what=""):
    assert len(a) == len(b) and len(a) > 0, what
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for j, (s, t) in enumerate(zip(x, y)):
            _same(s, t, (what, "call", i, ("q", "K", "V", "attention")[j]))


class _Driver:
    """One cache and the calls the attention patches make on it, layer by layer.  protocol "update": the reference's - ids
    shifted by the continuity rule, q / k rotated, `update` on the rotated tensors (text through its else-branch);
    "pre_rope": update_pre_rope for chunks, append_pre_rope for text and decode, and the op-by-op route wherever those decline
    (chunks below 512 rows, no reforging) - as the patches do."""

    def __init__(self, protocol, ids, dtype, L, reforge=True, fp8=False, prompt=0, **extra):
        import retake.longvideo_cache as lc

        if prompt:
            extra["prompt_guided_scoring"] = True
        reserve = {"reserve_tokens": extra.pop("reserve_tokens")} if "reserve_tokens" in extra else {}
        self.cache = lc.build_kvcache(_cfg(reforge, fp8, **extra), **reserve)
        self.protocol, self.mrope, self.dtype, self.L, self.prompt = protocol, ids == "mrope", dtype, L, prompt
        self.sec = SEC if self.mrope else None
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())
        self.t_next = 0
        self.log = []

    def _text_ids(self, n, t0=None):
        t0 = self.t_next if t0 is None else t0
        p = torch.arange(t0, t0 + n, device=dev()).view(1, 1, n)
        self.t_next = t0 + n
        return p.expand(3, 1, n).contiguous() if self.mrope else p[0].contiguous()

    def _video_ids(self, Lv, Lp):
        g = Lv // 64
        p = torch.from_numpy(synth.mrope_position_ids(self.t_next, g, 8, 8, hw0=self.t_next)).to(dev())
        if Lp:   # the appended prompt: text ids that follow the chunk (forge_input_chunks)
            p = torch.cat([p, torch.arange(self.t_next + g, self.t_next + g + Lp, device=dev()).view(1, 1, Lp).expand(3, 1, Lp)], dim=2)
        self.t_next += g
        return p.contiguous() if self.mrope else p[0].contiguous()

    def _feed(self, l, q, k, v, pos, video):
        cache = self.cache
        cache.kvcache_compression = video
        pos = pos.clone()
        out = None
        if self.protocol == "pre_rope":
            out = (cache.update_pre_rope if video else cache.append_pre_rope)(q.clone(), k, v, l, pos, self.rot, self.sec)
        if out is not None:
            return out
        cache.shift_temporal_ids_(pos, l)   # (no reforge: no shift, no ids kept)
        qr = synth.rope_forward(q.float(), pos, self.rot, self.sec).to(q.dtype)
        kr = synth.rope_forward(k.float(), pos, self.rot, self.sec).to(q.dtype)
        kw = {"query_states": qr, "position_ids": pos, "rotary_emb": self.rot, "mrope_section": self.sec}
        kk, vv = cache.update(kr, v, l, kw)
        return qr, kk, vv

    def step(self, seed, n, video=False, t0=None, after_forward=True, layers=range(LAYERS)):
        """One forward of n rows through the layers; the log gets (rotated q, K view, V view, attention output) clones."""
        cache = self.cache
        lp = self.prompt if video else 0
        pos = self._video_ids(n, lp) if video else self._text_ids(n, t0)
        if video and lp:
            cache.before_forward(prompt_length=lp)
        for l in layers:
            q, k, v = _qkv(1000 * seed + l, n + lp, self.dtype)
            qr, kk, vv = self._feed(l, q, k, v, pos, video)
            out = cache.attention(qr, kk, vv, layer_idx=l)
            assert out is not None
            self.log.append((qr.clone(), kk.clone(), vv.clone(), out.clone()))
        if video and after_forward:
            cache.after_forward()
        cache.kvcache_compression = False

    def prefill(self, chunks=2):
        self.step(1, TEXT)
        for c in range(chunks):
            self.step(2 + c, self.L, video=True)
        return self

    def question(self, seed, n, decode=DECODE):
        """n question rows + `decode` single-row steps, ids continuing from the end of the video; returns that part of the log."""
        at = len(self.log)
        t0 = TEXT + 2 * (self.L // 64)
        self.step(seed, n, t0=t0)
        for i in range(decode):
            self.step(seed + 1 + i, 1)
        return self.log[at:]


def _twin_run(protocol, ids, dtype, L, use_video_end=False, **kw):
    a = _Driver(protocol, ids, dtype, L, **kw).prefill()
    m = a.cache.mark()
    ve = a.cache.video_end
    assert ve is not None and ve.layers == m.layers and ve.serial < m.serial
    after_video = _state(a.cache)
    a.question(10, Q1)
    assert a.cache.get_seq_length(0) == after_video["len0"] + Q1 + DECODE
    assert a.cache.rewind(ve if use_video_end else m) is None
    _same_state(a.cache, after_video, "after rewind")
    log_a = a.question(20, Q2)
    b = _Driver(protocol, ids, dtype, L, **kw).prefill()
    _same_state(b.cache, after_video, "fresh prefill")
    log_b = b.question(20, Q2)
    _same_log(log_a, log_b, (protocol, ids, dtype, L))
    _same_state(a.cache, b.cache, "after question 2")
    return a, b


# ---------------------------------------------------------------------------------------------------
# 1. the twin run
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [512, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("protocol", ["update", "pre_rope"])
def test_twin_run(protocol, ids, dtype, L):
    a, _ = _twin_run(protocol, ids, dtype, L, use_video_end=protocol == "update")
    keep = int(RATIO * L)
    assert a.cache.get_seq_length(0) == TEXT + 2 * keep + Q2 + DECODE
    assert a.cache.num_evicted_tokens == [2 * (L - keep)] * LAYERS


def test_twin_run_without_reforge():
    _twin_run("update", "mrope", torch.bfloat16, 512, reforge=False)


# ---------------------------------------------------------------------------------------------------
# 2. video after a rewind
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,protocol", [(512, "pre_rope"), (64, "update")])
def test_video_after_rewind(L, protocol):
    """A: chunk 1, mark, question, rewind, chunk 2.  B: chunk 1, chunk 2."""
    a = _Driver(protocol, "mrope", torch.bfloat16, L).prefill(chunks=1)
    m = a.cache.mark()
    t = a.t_next
    a.question(10, Q1)
    a.cache.rewind(m)
    a.t_next = t
    at = len(a.log)
    a.step(3, L, video=True)
    b = _Driver(protocol, "mrope", torch.bfloat16, L).prefill(chunks=2)
    _same(a.cache.last_keep_indices, b.cache.last_keep_indices, "last_keep_indices")
    _same_log(a.log[at:], b.log[-LAYERS:], "chunk 2")
    _same_state(a.cache, b.cache, "after chunk 2")
    assert a.cache.video_end.layers == b.cache.video_end.layers


# ---------------------------------------------------------------------------------------------------
# 3. fp8 rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [512, 64])
def test_twin_run_fp8(L):
    a, b = _twin_run("pre_rope", "mrope", torch.bfloat16, L, fp8=True)
    keep = int(RATIO * L)
    assert a.cache.archive_len(0) == 2 * keep and a.cache._layers[0].length == TEXT + Q2 + DECODE


def test_fp8_rewind_between_chunks():
    """A mark between the two chunks, rewound to after both: archive_len and the archive views match a fresh cache that saw
    one chunk, and so does the attention over them."""
    L = 512
    a = _Driver("pre_rope", "mrope", torch.bfloat16, L, fp8=True).prefill(chunks=1)
    m = a.cache.mark()
    t = a.t_next
    a.step(3, L, video=True)
    assert a.cache.archive_len(0) == 2 * int(RATIO * L)
    a.cache.rewind(m)
    a.t_next = t
    b = _Driver("pre_rope", "mrope", torch.bfloat16, L, fp8=True).prefill(chunks=1)
    assert a.cache.archive_len(0) == b.cache.archive_len(0) == int(RATIO * L)
    _same_state(a.cache, b.cache, "one chunk")
    assert a.cache.video_end is not None and a.cache.video_end.layers == m.layers
    log_a = a.question(20, Q2)
    b.t_next = t
    log_b = b.question(20, Q2)
    _same_log(log_a, log_b, "attention over the archive")
    _same_state(a.cache, b.cache, "after the question")


# ---------------------------------------------------------------------------------------------------
# 4. prompt-guided scoring
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,protocol", [(512, "pre_rope"), (512, "update"), (64, "update")])
def test_twin_run_prompt_guided(L, protocol):
    a, _ = _twin_run(protocol, "mrope", torch.float32, L, prompt=LP)
    keep = int(RATIO * L)
    assert a.cache.get_seq_length(0) == TEXT + 2 * keep + Q2 + DECODE
    assert a.cache.num_evicted_tokens == [2 * (L + LP - keep)] * LAYERS


# ---------------------------------------------------------------------------------------------------
# 5. a mark between update and after_forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,protocol", [(512, "pre_rope"), (64, "update")])
def test_mark_before_after_forward_equals_mark_after(L, protocol):
    a = _Driver(protocol, "mrope", torch.bfloat16, L)
    a.step(1, TEXT)
    a.step(2, L, video=True, after_forward=False)
    assert a.cache._batch.pending == list(range(LAYERS))
    m1 = a.cache.mark()
    a.cache.after_forward()
    m2 = a.cache.mark()
    ve = a.cache.video_end
    for name in ("epoch", "layers", "n_layers", "pos_layers", "n_evicted", "seen_tokens"):
        assert getattr(m1, name) == getattr(m2, name) == getattr(ve, name), name
    assert m1.layers[0].length == TEXT + int(RATIO * L) and m1.layers[0].num_evicted == L - int(RATIO * L)
    assert m1.serial < ve.serial < m2.serial and m1.cache is a.cache and m1.resume_position_ids is None


# ---------------------------------------------------------------------------------------------------
# 6. crop
# ---------------------------------------------------------------------------------------------------
def test_crop():
    L = 512
    a = _Driver("pre_rope", "mrope", torch.bfloat16, L).prefill()
    b = _Driver("pre_rope", "mrope", torch.bfloat16, L).prefill()
    for d in (a, b):
        d.question(10, Q1, decode=0)
    m = b.cache.mark()
    for d in (a, b):
        for i in range(DECODE):
            d.step(30 + i, 1)
    before = _state(a.cache)
    a.cache.crop(10 ** 9)                       # at or above the current length: nothing happens
    a.cache.crop(before["len0"])
    _same_state(a.cache, before, "no-op crops")
    with pytest.raises(ValueError, match="compressed"):     # into the compressed video
        a.cache.crop(TEXT + int(RATIO * L) + 3)
    with pytest.raises(ValueError, match="compressed"):
        a.cache.crop(-(Q1 + DECODE + 1))
    _same_state(a.cache, before, "refused crops")
    a.cache.crop(-DECODE)
    b.cache.rewind(m)
    _same_state(a.cache, b.cache, "crop(-3) against rewind")
    assert a.cache.get_seq_length(0) == before["len0"] - DECODE
    # down to the boundary itself, by length; the cache goes on working and equals a cache that never saw the question
    a.cache.crop(TEXT + 2 * int(RATIO * L))
    c = _Driver("pre_rope", "mrope", torch.bfloat16, L).prefill()
    _same_state(a.cache, c.cache, "crop to the video's end")
    _same_log(a.question(20, Q2), c.question(20, Q2), "question after the crop")
    _same_state(a.cache, c.cache, "after the question")


# ---------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------
def test_refused_marks_change_nothing():
    L = 64
    a = _Driver("update", "mrope", torch.float32, L).prefill()
    other = _Driver("update", "mrope", torch.float32, L).prefill()
    m1 = a.cache.mark()
    a.question(10, Q1, decode=1)
    m2 = a.cache.mark()
    a.step(40, 1)
    before = _state(a.cache)
    with pytest.raises(ValueError, match="another cache"):
        a.cache.rewind(other.cache.mark())
    with pytest.raises(ValueError):
        a.cache.rewind(None)
    _same_state(a.cache, before, "a mark of another cache")
    a.cache.rewind(m1)
    after = _state(a.cache)
    with pytest.raises(ValueError, match="invalidated"):       # m2's rows have been given up
        a.cache.rewind(m2)
    _same_state(a.cache, after, "an invalidated mark")
    a.cache.rewind(m1)                                         # m1 itself stays good, and so does a later mark
    a.question(20, Q2, decode=0)
    m3 = a.cache.mark()
    a.step(41, 1)
    a.cache.rewind(m3)
    assert a.cache.get_seq_length(0) == after["len0"] + Q2
    # a mark from before the buffers were replaced
    m4 = a.cache.mark()
    ks, vs = ([view[l].clone() for l in range(LAYERS)] for view in (a.cache.key_cache, a.cache.value_cache))
    a.cache.key_cache = ks
    a.cache.value_cache = vs
    before = _state(a.cache)
    with pytest.raises(ValueError, match="replaced"):
        a.cache.rewind(m4)
    _same_state(a.cache, before, "a mark from before key_cache was assigned")
    m5 = a.cache.mark()
    a.cache.position_cache = a.cache.position_cache
    with pytest.raises(ValueError, match="replaced"):
        a.cache.rewind(m5)
    with pytest.raises(ValueError, match="replaced"):          # video_end is such a mark too now
        a.cache.rewind(a.cache.video_end)


# ---------------------------------------------------------------------------------------------------
# 8. nothing is allocated
# ---------------------------------------------------------------------------------------------------
def test_rewind_allocates_nothing():
    L = 512
    a = _Driver("pre_rope", "mrope", torch.bfloat16, L, reserve_tokens=2048).prefill()
    assert a.cache.reserve_tokens == 2048
    for seed, n in [(10, Q1), (20, Q1)] + [(s0 + 1 + i, 1) for s0 in (10, 20) for i in range(DECODE)]:
        for l in range(LAYERS):   # (the shared inputs of both questions exist before anything is measured)
            _qkv(1000 * seed + l, n, torch.bfloat16)

    def pointers():
        return [(st.k.data_ptr(), st.v.data_ptr(), st.pos.data_ptr(), st.k.shape, st.pos.shape) for st in a.cache._layers]

    m = a.cache.mark()
    p0 = pointers()
    a.log.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a.question(10, Q1)
    a.log.clear()
    gc.collect()
    torch.cuda.synchronize()
    peak1, held1 = torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()
    a.cache.rewind(m)
    assert pointers() == p0 and torch.cuda.memory_allocated() == held1
    a.question(20, Q1)                           # a different question of the same length
    a.log.clear()
    gc.collect()
    torch.cuda.synchronize()
    assert pointers() == p0
    assert torch.cuda.max_memory_allocated() == peak1 and torch.cuda.memory_allocated() == held1
    # the fp8 archive stays where it is, too
    f = _Driver("pre_rope", "mrope", torch.bfloat16, L, fp8=True).prefill()
    arch = [tuple(t.data_ptr() for t in (st.k8, st.v8, st.ks8, st.vs8)) for st in f.cache._layers]
    m = f.cache.mark()
    f.question(10, Q1)
    f.cache.rewind(m)
    assert arch == [tuple(t.data_ptr() for t in (st.k8, st.v8, st.ks8, st.vs8)) for st in f.cache._layers]


# ---------------------------------------------------------------------------------------------------
# 9. glue: the resume ids of a chunked prefill
# ---------------------------------------------------------------------------------------------------
class _CacheDrivingLM:
    """glue_stubs.StubLanguageModel whose call also does to the cache what the patched attention layers do: every layer
    shifts the ids it was handed IN PLACE by the continuity rule (qwen2_vl.py:68-73) and updates the cache with rows of that
    many tokens (synthetic projections: the glue is what is tested)."""

    def __init__(self, stub, mrope):
        self.stub, self.mrope, self.n_calls = stub, mrope, 0
        self.rot = synth.RotaryStub(synth.inv_freq(D), A, device=dev())

    @property
    def calls(self):
        return self.stub.calls

    def embed_tokens(self, ids):
        return self.stub.embed_tokens(ids)

    def __call__(self, **kw):
        out = self.stub(**kw)                    # records clones of what the forward handed over
        cache, pos = kw["past_key_values"], kw["position_ids"]
        n = pos.shape[-1]
        sec = SEC if self.mrope else None
        self.n_calls += 1
        for l in range(LAYERS):
            q, k, v = _qkv(7000 + 10 * self.n_calls + l, n, torch.float32)
            cache.shift_temporal_ids_(pos, l)
            qr = synth.rope_forward(q, pos, self.rot, sec)
            kr = synth.rope_forward(k, pos, self.rot, sec)
            cache.update(kr, v, l, {"query_states": qr, "position_ids": pos, "rotary_emb": self.rot, "mrope_section": sec})
        return out


def _glue_cfg(cfg):
    llm = cfg.text_config if hasattr(cfg, "text_config") else cfg
    llm.hidden_size, llm.num_attention_heads, llm.num_key_value_heads, llm.num_hidden_layers = Hq * D, Hq, Hkv, LAYERS
    return cfg


@pytest.mark.parametrize("model", ["qwen2vl", "llava"])
def test_glue_resume_position_ids(model):
    import glue_stubs as gs
    import retake._prefill as pf

    n_post = 7
    if model == "qwen2vl":
        import retake.qwen2_vl as mod

        # (visual ratio 1: no frame is dropped, so the reference's segmentation - made before the drop - fits the ids)
        cfg = _glue_cfg(gs.qwen_config(ratio=1.0, kv_ratio=0.5, chunk_frames=16))
        me = gs.make_qwen_model(mod, cfg)
        kw = gs.qwen_inputs(grid_t=32, n_post=n_post, device=dev())      # 32 frames x 4 tokens: two chunks of 64
        me.model = lm = _CacheDrivingLM(me.model, True)
        out = mod.retake_Qwen2VLForConditionalGeneration_forward(me, return_dict=False, **kw)
    else:
        import retake.llava_onevision as mod

        cfg = _glue_cfg(gs.llava_config(ratio=1.0, kv_ratio=0.5, chunk_frames=12))
        # (the reference's LLaVA token splice drops the newline slot from the ids even at ratio 1: segments and ids only
        # line up with the visual compression off)
        cfg.longvideo_kwargs["visual_compression"] = False
        kw, bank = gs.llava_inputs(T=16, n_post=n_post, device=dev())      # 16 frames x 4 tokens + the newline slot: chunks of 48 and 17
        me = gs.make_llava_model(mod, cfg, bank.to(dev()))
        me.image_newline = me.image_newline.to(dev())
        me.language_model = lm = _CacheDrivingLM(me.language_model, False)
        me.get_input_embeddings = lambda: lm.embed_tokens
        out = mod.retake_LlavaOnevisionForConditionalGeneration_forward(me, return_dict=False, **kw)
    cache = out[1]
    calls = lm.calls
    assert len(calls) >= 3 and calls[-2]["kvcache_compression"] and not calls[-1]["kvcache_compression"]
    trailing = calls[-1]["position_ids"]         # the ids the forward gave the trailing text rows, before any shift
    assert trailing.shape[-1] == n_post
    mark = cache.video_end
    assert mark is not None and mark.resume_position_ids is not None
    assert mark.resume_position_ids.dtype == torch.int64 and mark.resume_position_ids.device.type == "cpu"
    P = 3 if model == "qwen2vl" else 1
    assert torch.equal(mark.resume_position_ids, trailing[..., 0].reshape(P))
    for n in (1, 4, n_post):
        got = pf.followup_position_ids(mark, n, dev())
        assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == trailing[..., :n].shape
        assert torch.equal(got.cpu(), trailing[..., :n])
    # the mark is the end of the video: rewinding drops the trailing text rows, and only those
    n_all = cache.get_seq_length(0)
    cache.rewind(mark)
    assert cache.get_seq_length(0) == n_all - n_post and cache.kvcache_compression is False

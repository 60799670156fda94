"""PivotKVCache.fork on the GPU: TWIN comparisons in the style of tests/test_rewind_gpu.py (whose driver this file reuses) -
a branch answers a question, a fresh cache with the same prefill answers the same question, and the two are compared; never
the code under test with itself.

Shapes: 2 layers, Hq 4, Hkv 2, D 128, ratio 0.25; L 512 and L 64; M-RoPE and plain ids; both entry protocols.
  aligned    TEXT 64 + two chunks of L 512: 320 16-bit rows at `video_end` (fp8 rows: 64 16-bit + 256 archived) - whole key
             tiles of both attention kernels, so EVERYTHING is bit-equal: own K / V rows, ids, lengths, every attention output
  unaligned  TEXT 5 (261 rows), or L 64 (96 rows: no multiple of the chunk kernel's 64): stored rows and ids bit-equal, the
             attention outputs within the 16-bit kernel's own bar of float64 (tests/test_attention_gpu.py: max(2 E, half an
             output ulp), E the eager expression's error on the same tensors)."""
import copy
import functools
import gc

import pytest
import torch

import attention_ref as ar
import test_rewind_gpu as trg
from test_rewind_gpu import DECODE, LAYERS, Hkv, D, RATIO, _same, _state

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
QN = 9    # rows of the question


class Driver(trg._Driver):
    """test_rewind_gpu's driver with the length of the leading text as a parameter, and branches."""

    def __init__(self, protocol, ids, dtype, L, text, packed=False, **kw):
        super().__init__(protocol, ids, dtype, L, **kw)
        self.text = text
        if packed:
            self.cache.decode_attention = "packed"

    def prefill(self, chunks=2):
        self.step(1, self.text)
        for c in range(chunks):
            self.step(2 + c, self.L, video=True)
        return self

    def t_video_end(self):
        return self.text + 2 * (self.L // 64)

    def question(self, seed, n, decode=DECODE):
        at = len(self.log)
        self.step(seed, n, t0=self.t_video_end())
        for i in range(decode):
            self.step(seed + 1 + i, 1)
        return self.log[at:]

    def branch(self, mark=None, **kw):
        d = copy.copy(self)
        d.cache, d.log = self.cache.fork(mark, **kw), []
        return d


def _make(protocol="pre_rope", ids="mrope", dtype=BF16, L=512, text=64, fp8=False, packed=False):
    return Driver(protocol, ids, dtype, L, text, packed=packed, fp8=fp8).prefill()


@functools.lru_cache(maxsize=None)
def _twin(seed, n, *cfg):
    """A fresh cache with the same prefill answering question (seed, n) alone: its log and final state, made once per
    configuration and shared (nothing writes them)."""
    d = _make(*cfg)
    at_video_end = _state(d.cache)
    log = d.question(seed, n)
    return log, _state(d.cache), at_video_end


def _same_observables(br, twin_state, what):
    """Every observable of the twin rule that a branch answers for the whole sequence."""
    s = _state(br)
    assert s.keys() == twin_state.keys(), what
    for key, want in twin_state.items():
        if key == "pos":
            assert len(s[key]) == len(want)
            for x, y in zip(s[key], want):
                _same(x, y, (what, key))
        else:
            _same(s[key], want, (what, key))


def _same_answers(blog, tlog, base, bitwise, what):
    """A branch's calls against the twin's: the rotated queries and the stored own rows bit for bit (the twin's views hold
    the `base` shared 16-bit rows first); the attention outputs bit for bit, or both within the kernel's bar of float64."""
    assert len(blog) == len(tlog) > 0, what
    for i, ((q, k, v, o), (tq, tk, tv, to)) in enumerate(zip(blog, tlog)):
        _same(q, tq, (what, i, "q"))
        _same(k, tk[:, :, base:], (what, i, "K"))
        _same(v, tv[:, :, base:], (what, i, "V"))
        if bitwise:
            _same(o, to, (what, i, "attention"))
            continue
        ref = ar.attention_fp64(tq, tk, tv)
        e = (ar.attention_eager_reference(tq, tk, tv).double() - ref).abs().max().item()
        bar = max(2.0 * e, ar.half_ulp(q.dtype, ref.abs().max().item()))
        err, twin = ((x.double() - ref).abs().max().item() for x in (o, to))
        print(f"fp64[fork {what} call {i}]: branch {err:.3e}  twin {twin:.3e}  eager E {e:.3e}  bar {bar:.3e}")
        assert err <= bar, (what, i, err, bar)


def _fork_and_ask(cfg, seed=20, n=QN, bitwise=True, **fork_kw):
    p = _make(*cfg)
    br = p.branch(p.cache.video_end, **fork_kw)
    tlog, tstate, at_ve = _twin(seed, n, *cfg)
    assert br.cache.forked_from is p.cache.video_end
    _same_observables(br.cache, at_ve, "at the fork")
    base = br.cache.shared_len(0)
    blog = br.question(seed, n)
    _same_answers(blog, tlog, base, bitwise, cfg)
    _same_observables(br.cache, tstate, "after the question")
    return p, br


# ---------------------------------------------------------------------------------------------------
# 1. the aligned twin: everything bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["mrope", "plain"])
@pytest.mark.parametrize("protocol", ["update", "pre_rope"])
def test_aligned_twin(protocol, ids):
    p, br = _fork_and_ask((protocol, ids, BF16, 512, 64))
    keep = int(RATIO * 512)
    assert br.cache.shared_len(0) == 64 + 2 * keep == 320 and br.cache._layers[0].length == QN + DECODE
    assert br.cache.get_seq_length(0) == 320 + QN + DECODE and p.cache.get_seq_length(0) == 320
    assert br.cache.num_evicted_tokens == [2 * (512 - keep)] * LAYERS
    assert br.cache.attention_calls == LAYERS * (1 + DECODE)


def test_aligned_twin_fp8_rows():
    p, br = _fork_and_ask(("pre_rope", "mrope", BF16, 512, 64, True))
    assert br.cache.archive_len(0) == 256 and br.cache.shared_len(0) == 64 and br.cache.kv_cache_dtype == "fp8_e4m3"
    assert br.cache.archive(0)[0].untyped_storage().data_ptr() == p.cache.archive(0)[0].untyped_storage().data_ptr()


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_aligned_twin_packed_decode(fp8):
    _, br = _fork_and_ask(("pre_rope", "mrope", BF16, 512, 64, fp8, True))
    assert br.cache.decode_attention_calls == LAYERS * DECODE     # the decode steps (R = 2); the question (R = 18) is the chunk kernel's


def test_aligned_twin_fp16():
    _fork_and_ask(("pre_rope", "mrope", F16, 512, 64))


# ---------------------------------------------------------------------------------------------------
# 2. the unaligned twins: rows and ids bit for bit, attention within the kernel's bar of float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol,ids,L,text", [("pre_rope", "mrope", 512, 5), ("update", "plain", 512, 5),
                                                 ("update", "mrope", 64, 64), ("pre_rope", "plain", 64, 5)])
def test_unaligned_twin(protocol, ids, L, text):
    _, br = _fork_and_ask((protocol, ids, BF16, L, text), bitwise=False)
    assert br.cache.shared_len(0) == text + 2 * int(RATIO * L)


# ---------------------------------------------------------------------------------------------------
# 3. two branches and the parent, all live, interleaved layer by layer
# ---------------------------------------------------------------------------------------------------
def test_two_branches_and_the_parent_interleaved():
    cfg = ("pre_rope", "mrope", BF16, 512, 64)
    p = _make(*cfg)
    ve = p.cache.video_end
    at_ve = _state(p.cache)
    b1, b2 = p.branch(ve, reserve_tokens=64), p.branch(ve)
    asks = [(b1, 20, 9), (b2, 30, 7), (p, 40, 11)]
    t0 = p.t_video_end()
    for step in range(1 + DECODE):
        for l in range(LAYERS):
            for d, seed, n in asks:
                if step == 0:
                    d.step(seed, n, t0=t0, layers=[l])
                else:
                    d.step(seed + step, 1, t0=t0 + n + step - 1, layers=[l])
    for d, seed, n in asks:
        tlog, tstate, _ = _twin(seed, n, *cfg)
        _same_answers(d.log[-LAYERS * (1 + DECODE):], tlog, d.cache.shared_len(0), True, ("interleaved", seed))
        _same_observables(d.cache, tstate, ("interleaved", seed))
    # the parent at video_end is what it was
    p.cache.rewind(ve)
    _same_observables(p.cache, at_ve, "the parent, rewound to video_end")
    _same_observables(b1.cache, _twin(20, 9, *cfg)[1], "branch 1 afterwards")


# ---------------------------------------------------------------------------------------------------
# 4. mark / rewind / crop on a branch
# ---------------------------------------------------------------------------------------------------
def test_branch_mark_rewind_crop():
    cfg = ("pre_rope", "mrope", BF16, 512, 64)
    p = _make(*cfg)
    br = p.branch(p.cache.video_end)
    m = br.cache.mark()
    br.question(10, 7)
    assert br.cache.get_seq_length(0) == 320 + 7 + DECODE
    br.cache.rewind(m)
    assert br.cache.get_seq_length(0) == 320
    tlog, tstate, _ = _twin(20, QN, *cfg)
    _same_answers(br.question(20, QN), tlog, 320, True, "second question after a rewind")
    _same_observables(br.cache, tstate, "second question after a rewind")
    before = _state(br.cache)
    with pytest.raises(ValueError, match="compressed"):
        br.cache.crop(319)
    with pytest.raises(ValueError, match="compressed"):
        br.cache.crop(-(QN + DECODE + 1))
    _same_observables(br.cache, before, "refused crops")
    br.cache.crop(-DECODE)
    assert br.cache.get_seq_length(0) == 320 + QN and br.cache._layers[0].length == QN
    br.cache.crop(320)                             # down to the fork point itself, and on with another question
    _same_answers(br.question(20, QN), tlog, 320, True, "question after a crop to the fork point")


# ---------------------------------------------------------------------------------------------------
# 5. invalidation
# ---------------------------------------------------------------------------------------------------
def test_invalidation():
    cfg = ("pre_rope", "mrope", BF16, 512, 64)
    p = Driver(*cfg).prefill(chunks=1)
    m0 = p.cache.mark()
    p.step(3, 512, video=True)
    ve = p.cache.video_end
    br, gone = p.branch(ve), p.branch(ve)
    # the parent answers a question of its own and rewinds to the fork point itself: the branch still answers bit-equal
    p.question(40, 11)
    p.cache.rewind(ve)
    tlog, tstate, _ = _twin(20, QN, *cfg)
    _same_answers(br.question(20, QN), tlog, 320, True, "after the parent rewound to the fork point")
    _same_observables(br.cache, tstate, "after the parent rewound to the fork point")
    # ... to a mark BEFORE the fork point: the shared rows are given up
    p.cache.rewind(m0)
    q, k, v = trg._qkv(5000, 1, BF16)
    pos = torch.full((3, 1, 1), 100, dtype=torch.int64, device=trg.dev())
    for b in (br, gone):
        n = b.cache.get_seq_length(0)
        with pytest.raises(ValueError, match="invalidated"):
            b.cache.append_pre_rope(q.clone(), k, v, 0, pos.clone(), b.rot, b.sec)
        with pytest.raises(ValueError, match="invalidated"):
            b.cache.attention(q, k, v, layer_idx=0)
        assert b.cache.get_seq_length(0) == n


def test_released_parent_keeps_the_branch_valid():
    cfg = ("pre_rope", "mrope", BF16, 512, 64)
    p = _make(*cfg)
    br = p.branch(p.cache.video_end)
    mark = br.cache.forked_from
    del p
    gc.collect()
    assert mark.cache is None
    tlog, tstate, _ = _twin(20, QN, *cfg)
    _same_answers(br.question(20, QN), tlog, 320, True, "parent released")
    _same_observables(br.cache, tstate, "parent released")


# ---------------------------------------------------------------------------------------------------
# 6. memory: a fork costs its ids and its reserve, not the rows
# ---------------------------------------------------------------------------------------------------
def test_fork_memory():
    p = _make("pre_rope", "mrope", BF16, 512, 64)
    kv_bytes = sum(t.numel() * t.element_size() for st in p.cache._layers for t in (st.k, st.v))
    gc.collect()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    br = p.cache.fork(p.cache.video_end, reserve_tokens=64)
    delta = torch.cuda.memory_allocated() - held
    # by construction: [3, 320 + 64] ids and 64 rows of K and V per layer (the allocator rounds each up to 512 bytes)
    assert 0 < delta <= LAYERS * (3 * 8 * (320 + 64) + 2 * Hkv * 64 * D * 2 + 3 * 512)
    assert delta < 0.10 * kv_bytes, (delta, kv_bytes)        # a cap, not a measurement
    for l in range(LAYERS):
        ks, vs = br.shared(l)
        pst = p.cache._layers[l]
        assert ks.untyped_storage().data_ptr() == pst.k.untyped_storage().data_ptr() and ks.data_ptr() == pst.k.data_ptr()
        assert vs.untyped_storage().data_ptr() == pst.v.untyped_storage().data_ptr() and ks.shape == (1, Hkv, 320, D)
        assert br._layers[l].k.shape == (1, Hkv, 64, D)

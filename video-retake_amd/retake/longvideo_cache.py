"""PivotKV cache on MI355X.  Same surface as the reference's retake/longvideo_cache.py.

`PivotKVCache.update` (reference :217-323) keeps its signature, its `cache_kwargs` protocol (pops
`position_ids`, `query_states`, `rotary_emb`, `mrope_section`) and its return value (the UNCOMPRESSED
keys/values of the layer); everything it computes runs as HIP kernels behind the C ABI (include/retake_hip.h):
    rtk_pivotkv_update    one call per update: fused prepare (rotary tables + un-rotate q / k + append k / v, :238,
                          :248-259) - or, from the pre-RoPE projections, the whole attention prologue
                          (`update_pre_rope`: continuity shift + tables + RoPE + append + scoring operands)
    rtk_pivotkv_flush     one call per chunk, all pending layers: the two score passes (:260-268), finalize +
                          mask override + top-k + id gather / rescale (:269-295), and ONE in-place compaction launch
                          (kept K re-rotated at the new ids, kept V compacted inside the tail, ids; :278-318)
    rtk_pivotkv_append_rope   text prefill / decode segments (`append_pre_rope`; the else-branch :319-321)
The stage-by-stage entry points (rtk_pivotkv_prepare / _score_stages / _select / _evict_batched ...) serve the shapes
the one-call path does not: small chunks, fp32 passes, rotary modules that must be called, worker streams.

Memory layout (differs from the reference on purpose): each layer owns ONE pre-allocated
[1, Hkv, capacity, D] key and value buffer and one [P, capacity] position-id buffer.  `update` appends
the chunk at the tail (that view is what it returns to the layer's attention), prepares the scoring operands in the
layer's slot of a per-chunk batch and returns.  The eviction itself - scoring, selection, gather of the kept
rows, re-rotation of the kept keys at their new ids, compaction over the head of the tail, position
bookkeeping - is deferred until the view has been consumed and then flushed for ALL pending layers at
once (`after_forward`, which the reference calls after every video chunk; or the next `update` of a
pending layer; or any access to `key_cache` / `value_cache` / `position_cache`; or, with `flush_every_layers: N`, every N
layers).  This removes the reference's two O(cache) torch.cat rebuilds per (layer, chunk) and turns 28 launch-bound
evictions into one bandwidth-bound launch.  `memory_footprint()` says what all of it costs in bytes.

Where the rest lives (the names are re-exported here, and the other modules of the package import them from here):
    _rope_torch       repeat_kv, rotate_half, apply_rotary_pos_emb, apply_multimodal_rotary_pos_emb
    _hf_cache         DynamicCache: which class PivotKVCache subclasses, and why
    _cache_state      what a layer and a slot of the batch own (_LayerStore, _Batch, ...), the list views, CacheMark
    native_attention  chunk_attention, native_attention (causal offset from the HF mask), the fp8 row helpers
    _video_bound      the bounded video region: the sliding window and the video budget, planned and committed by one mechanism
    _focus            the question-focused decode cache: watch_question / focus, the rows a question's queries choose
    _sparse_decode    the page-sparse decode route: sparse_decode(cache) / dense_decode(cache), per-page key bounds beside
                      the rows (functions that take the cache; `attention` asks it while armed)
    _flush            the deferred eviction of a chunk: _flush, its one-call and stage-by-stage routes, what they call
    _update_stages    `update` stage by stage (_update_general): every shape the one-call hot path here does not serve
    _marks            restore points and branches: mark / rewind / crop / fork, never run during a prefill
"""
from __future__ import annotations

import ctypes as C
import sys
import weakref
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import (_flush as _fl, _focus, _marks, _native as nv, _sparse_decode, _update_stages as _us,   # (`_flush` is the method)
               _video_bound)
from ._cache_state import (CacheMark, _Batch, _CacheView, _LayerMark, _LayerStore, _Rotary, _Side, _Update,  # noqa: F401
                           _inv_stamp, _on_device, _version_of)
from ._hf_cache import DynamicCache, _hf_dynamic_cache_is_legacy, _ListDynamicCache  # noqa: F401
from ._rope_torch import _rotate, apply_multimodal_rotary_pos_emb, apply_rotary_pos_emb, repeat_kv, rotate_half  # noqa: F401
from .native_attention import (ATTENTION_KERNELS, KV_CACHE_DTYPES, chunk_attention, fp8_dequantize_rows,  # noqa: F401
                               fp8_quantize_rows, native_attention, wide_dispatch)

_WARNED = set()


def _warn_once(msg: str):
    if msg not in _WARNED:
        _WARNED.add(msg)
        print(msg, file=sys.stderr)


__all__ = ["repeat_kv", "rotate_half", "apply_multimodal_rotary_pos_emb", "apply_rotary_pos_emb", "PivotKVCache",
           "CacheMark", "build_kvcache", "DynamicCache"]


def _fill_io(io, q, qs, k, ks, v, vs, pos):
    """The operands of a rtk_update_io block (qs, ks, vs: the tensors' .stride()); the callers check them, each by its rules."""
    io.q, io.q_stride_h, io.q_stride_l = q.data_ptr(), qs[1], qs[2]
    io.k, io.k_stride_h, io.k_stride_l = k.data_ptr(), ks[1], ks[2]
    io.v, io.v_stride_h, io.v_stride_l = v.data_ptr(), vs[1], vs[2]
    io.pos, io.pos_stride = pos.data_ptr(), pos.stride(0)


class PivotKVCache(DynamicCache):
    """Drop-in for the reference's PivotKVCache (longvideo_cache.py:119-323)."""

    # mark / rewind (not in the reference).  Class-level defaults: the base class's __init__ already goes through the setters
    _epoch = 0                    # bumped wherever a layer's buffers are replaced or rewritten wholesale
    _mark_serial = 0              # marks taken so far
    _dead_marks = ()              # (lo, hi] serial ranges a rewind / crop has invalidated, lo ascending
    _flushes = 0                  # identity of the most recent compressed flush whose rows the cache holds
    _compressed_in_forward = False
    last_compressed_mark = None   # the mark `after_forward` took after the most recent forward that compressed a chunk
    # fork (not in the reference)
    forked_from = None            # a branch: the parent's mark it was forked at (PivotKVCache.fork)
    _fork_dead = None             # ... and why it is no longer valid, once the parent has given up the shared rows
    _branches = None              # a parent: weak set of its branches
    # question focus (not in the reference; _focus)
    _watch = None                 # armed by watch_question: the capture's buffers (None: off, nothing is copied)
    focused_from = None           # a focused cache (PivotKVCache.focus): the parent's `video_end` it was focused at
    def __init__(self, config, reserve_tokens: Optional[int] = None, reserve_archive_tokens: Optional[int] = None) -> None:
        """reserve_tokens (not in the reference): tokens per layer this cache is expected to hold at most - compressed
        prompt + one uncompressed chunk + generation.  The first allocation of a layer takes that size, which saves the
        geometric regrowth copies (~0.4 % of a 2048-frame prefill) and half the memory; without it buffers double.
        reserve_archive_tokens: the same for the fp8 archive of the kept video rows (kv_cache_dtype="fp8_e4m3"), whose
        rows then do not count towards reserve_tokens."""
        self.reserve_tokens = int(reserve_tokens) if reserve_tokens else 0
        self.reserve_archive_tokens = int(reserve_archive_tokens) if reserve_archive_tokens else 0
        self._layers: List[_LayerStore] = []
        self._batch: Optional[_Batch] = None
        self._last_slot = None
        self._pos_layers = 0          # len(position_cache) of the reference (skipped layers are padded with [])
        self._kview = _CacheView(self, "k")
        self._vview = _CacheView(self, "v")
        super().__init__()
        self._layers = []  # drop whatever the base class appended through the views
        self.config = config
        llm_config = config.text_config if hasattr(config, "text_config") else config  # LLaVA-OneVision / Qwen2-VL
        self.hidden_size = llm_config.hidden_size
        self.num_hidden_layers = llm_config.num_hidden_layers
        self.num_heads = llm_config.num_attention_heads
        self.head_dim = self.hidden_size // self.num_heads
        self.num_key_value_heads = llm_config.num_key_value_heads
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads

        kv_compression_kwargs = config.longvideo_kwargs["kvcache_compression_kwargs"]
        self.kvcache_compression = True
        self.kv_compression_kwargs = kv_compression_kwargs
        self.compression_ratio = kv_compression_kwargs["compression_ratio"]  # captured at construction (P0b)
        self.compression_method = kv_compression_kwargs["compression_method"]
        self.pos_embed_reforge = kv_compression_kwargs.get("pos_embed_reforge", False)
        # cos/sin of the position ids are computed inside the HIP kernels from rotary_emb.inv_freq / attention_scaling
        # whenever the rotary module is of the static inv_freq * position kind (HF's default / linear / YaRN / llama3
        # rope types, which is every shipped config: configs/*.yaml patch YaRN, monkeypatch.py:24-48) - correctly
        # rounded sin / cos, within one fp32 ulp of the module's, kept keys inside the 1e-5 bar.  Any other module
        # (dynamic / longrope types, no inv_freq) is CALLED, exactly as the reference does (:249, :298).
        # native_rope: False forces the call for every module (the bit-faithful opt-out).
        self.native_rope = bool(kv_compression_kwargs.get("native_rope", True))
        self._rotaries: Dict[int, Tuple[Any, Optional[_Rotary], Any]] = {}
        self._aio = nv.UpdateIO()   # argument block of append_pre_rope
        # MI355X build option for 16-bit models: "fp32" (default) scores with exact bf16 / fp16 products, fp32 accumulation,
        # softmax and sums; "reference" reproduces the reference's own bf16 (fp16 on a float16 model) roundings of the
        # logits, probabilities, per-head sums and means (longvideo_cache.py:264-270) - coarser, but what the reference
        # computes; "fast" (bf16 only) is the two-instruction softmax on the fp16 matrix path
        self.score_rounding = str(kv_compression_kwargs.get("score_rounding", "fp32"))
        if self.score_rounding not in ("fp32", "reference", "fast"):
            raise ValueError(f"score_rounding must be 'fp32', 'reference' or 'fast', got {self.score_rounding!r}")
        # MI355X build option: run scoring / selection of each update on one of N worker HIP streams.  Only
        # the tail append stays on the caller's stream (it is all the layer's attention needs); the flush
        # waits for the workers' events.  Independent updates then overlap on the GPU.
        self.overlap_streams = int(kv_compression_kwargs.get("overlap_streams", 0))
        # the reference overwrites the score of every key-patch token with 1.0 (:272-274): the batched pass 2 does not
        # compute those columns.  Same kept set, same scores after the override; False restores the full pass (tests / A/B)
        self.skip_masked_columns = bool(kv_compression_kwargs.get("skip_masked_columns", True))
        # compression_ratio 1 (what `dynamic_compression_ratio` sets for every prompt within max_input_length,
        # qwen2_vl.py:553-554): keep == chunk length, so topk(k = L) followed by the ascending sort (:276-277) is the
        # identity whatever the scores are, and the id rescale (:288-292) multiplies by 1.0.  The scoring passes and the
        # selection are not run then - the K round trip through the un-rotated frame and the bookkeeping still are.
        # True restores them (tests, `last_scores`)
        self.score_when_keeping_all = bool(kv_compression_kwargs.get("score_when_keeping_all", False))
        # MI355X build option (retake/sharded.py sets it): the kept keys stay UN-rotated in the cache and their ids
        # provisional; the owner rotates them once, at their final ids (rtk_rope_rotate_rows), when the temporal offset
        # of its block is known.  key_cache then holds un-rotated rows until that call.
        self.defer_rerotation = bool(kv_compression_kwargs.get("defer_rerotation", False))
        # MI355X build option: what the attention prologue (update_pre_rope) hands to the score passes and the re-rotation.
        #   "reference" (default)  q~ / k~ = the reference's own operands: the un-rotation of the rotated rows, with the
        #                          model dtype's rounding per torch op (longvideo_cache.py:76-78, :248-259).  On a bf16 model
        #                          that round trip moves the exact score of a token by up to ~2e-2 (6 bf16 ulps; measured,
        #                          tests/golden/gen_golden.py --only pivotkv_prerope_bf16) - it is part of what the reference
        #                          computes, so scores, kept sets and kept keys follow it bit for bit;
        #   "pre_rope"             q~ := q0, k~ := k0 (equal up to that rounding; more accurate, not the
        #                          reference's bits) - no copy of the queries (they are scored where they lie).
        self.prologue_operands = str(kv_compression_kwargs.get("prologue_operands", "reference"))
        if self.prologue_operands not in ("reference", "pre_rope"):
            raise ValueError(f"prologue_operands must be 'reference' or 'pre_rope', got {self.prologue_operands!r}")
        # MI355X build option (tests / A-B): False makes the prologue route pack a copy of the queries for the score passes
        # even when they could be read where they lie (prologue_operands="pre_rope" only)
        self.score_queries_in_place = bool(kv_compression_kwargs.get("score_queries_in_place", True))
        # MI355X build option (tests / A-B): False makes rtk_pivotkv_flush stage the rows whose source lies inside the
        # destination range and place them with a second launch, instead of the one in-place compaction launch
        self.in_place_compaction = bool(kv_compression_kwargs.get("in_place_compaction", True))
        # MI355X build option (tests / A-B): False sends every update and flush through the stage-by-stage route
        # instead of the one-call entry points rtk_pivotkv_update / rtk_pivotkv_flush - same kernels, same results
        self.one_call_update = bool(kv_compression_kwargs.get("one_call_update", True))
        # MI355X build option: bound the scratch of the deferred eviction.  0 (default): one flush per chunk for ALL layers -
        # every layer's q~ / k~ / partials wait in their own slot until `after_forward` (scratch = layers x ~(Hq + Hkv) L D
        # elements: 1.4 GB at L = 6272, 28 layers, bf16).  N > 0: the batch has N slots (slot = layer mod N) and is flushed
        # whenever the next layer's slot is taken, i.e. every N layers - scratch / launches-per-chunk trade N/layers : layers/N
        self.flush_every_layers = int(kv_compression_kwargs.get("flush_every_layers", 0))
        # MI355X build option: on the reference's protocol (`update` on rotated tensors) the launch that un-rotates and
        # appends layer l's chunk can also apply layer l + 1's continuity shift (qwen2_vl.py:68-73) to the caller's ids, so
        # that `shift_temporal_ids_` of the attention patch launches once per chunk instead of once per layer.  It WRITES
        # the caller's `position_ids` - which the reference's `update` never does - so it is OPT-IN per call: only a caller
        # that passes cache_kwargs["shift_next_position_ids"] = True gets it (the Qwen2-VL patch does: it shares one ids
        # tensor between the layers and shifts it in place itself; the LLaVA patch, which shifts a private clone per layer,
        # does not).  This key is the kill switch: False = every layer's shift is its own launch, whatever the caller says.
        self.shift_next_in_update = bool(kv_compression_kwargs.get("shift_next_in_update", True))
        self._preshifted = None       # (ids tensor, its version, layer, stream) an update launch has already shifted for
        # MI355X build option (not in the reference, which leaves `prompt_guided_compression` unfinished: its before_forward
        # ignores prompt_length): True makes a chunk that follows before_forward(prompt_length=Lp), 0 < Lp < L, a
        # PROMPT-GUIDED unit - its last Lp rows are the appended prompt, the Lv = L - Lp video keys are scored by the prompt's
        # queries alone (softmax over the video keys, no mask, mean over rows / heads / groups: every score < 1), the
        # selection keeps max(1, int(ratio * Lv)) of the VIDEO rows and the prompt rows are not cached.  What the layer's
        # attention sees is unchanged.  False (default): nothing changes anywhere, prompt_length is ignored as in the reference
        self.prompt_guided_scoring = bool(kv_compression_kwargs.get("prompt_guided_scoring", False))
        self._prompt_len = 0          # prompt rows of the chunk in flight (before_forward .. after_forward), 0 = none
        if self.flush_every_layers < 0:
            raise ValueError("flush_every_layers must be >= 0")
        self._sides: List[_Side] = []
        self._side_rr = 0
        self.num_evicted_tokens: List[int] = []
        self.keypatches_mask_chunk = None
        self._ws: Dict[str, torch.Tensor] = {}
        self._warned = False
        # MI355X build option, a top-level key of longvideo_kwargs (build_kvcache reads it): "hip" makes the attention
        # patches call `attention` below instead of torch / flash_attn; None (default) leaves them exactly as they are
        self.attention_kernel = None
        # MI355X build option, a top-level key of longvideo_kwargs (build_kvcache reads it): "fp8_e4m3" keeps the kept rows of
        # compressed video chunks as e4m3 codes + one power-of-two scale per (kv head, row) in a per-layer ARCHIVE beside the
        # 16-bit buffers (include/retake_hip.h "FP8 rows of the compressed cache").  The 16-bit buffers go on holding what is
        # not a kept video row - text, the in-flight chunk, decode rows; a flush quantises the kept rows into the archive
        # and leaves the 16-bit length where it was.  Lossy, not in the reference; needs attention_kernel="hip".
        self.kv_cache_dtype = None
        self.attention_calls = 0      # native attention launches so far (tests count them)
        # MI355X build option, a top-level key of longvideo_kwargs (build_kvcache reads it): "packed" makes `attention` try
        # the GQA-packed few-row kernel first (chunk_attention(packed_gqa=True)); None (default): exactly as without it
        self.decode_attention = None
        self.decode_attention_calls = 0   # ... of which took the packed kernel
        # MI355X build option, a top-level key of longvideo_kwargs (build_kvcache reads it): "packed" makes `attention` try
        # the wide packed kernel (chunk_attention(packed_wide=True): up to 64 packed rows - the verification step of
        # assisted generation, a few-token continuation) where the packed one declines, at the geometries where it measured
        # faster than the chunk kernel (native_attention.wide_dispatch); needs decode_attention="packed".  None (default):
        # exactly as without it
        self.multi_token_attention = None
        self.wide_attention_calls = 0     # ... of which took the wide packed kernel
        # MI355X build options, top-level keys of longvideo_kwargs (build_kvcache reads them; NOT in the reference, which
        # processes a finished video), for streams that do not end: a bound on a layer's VIDEO REGION - everything behind its
        # pinned rows (_LayerStore.pinned); with fp8 rows the archive.  video_window_rows = W bounds it by age: when
        # `after_forward` finds more than W + video_window_slack rows there it drops the oldest, down to W.  video_budget_rows
        # = B bounds it by SCORE (a rule of this project's own - answer quality is not evaluated): down to the newest row and
        # the B - 1 best-scored others; then a chunk that keeps all of its rows is scored all the same
        # (score_when_keeping_all).  Both act ONLY in `after_forward`: a caller that never calls it gets neither.  The slack
        # trades memory for fewer moves: a move rewrites the whole region whatever it drops.  None (default): off, nothing
        # changes, no score buffer exists.  The mechanism, and what each policy does: _video_bound.
        self.video_window_rows, self.video_window_slack = None, 0
        self.video_budget_rows, self.video_budget_slack = None, 0
        # video_budget_rescore = alpha in (0, 1], needs video_budget_rows (again NOT in the reference and a rule of this
        # project's own - answer quality is not evaluated): in `after_forward`, in front of the eviction, the stored scores of
        # the region's OLD rows are blended with what the last video_budget_observe_rows (default 64) rotated query rows of
        # the chunk that has just gone through see of them (_video_bound.rescore_budget).  None (default): off, nothing
        # changes, bit for bit - no query buffer exists and nothing is launched
        self.video_budget_rescore, self.video_budget_observe_rows = None, 64
        self.budget_rescored: List[int] = []  # per layer: re-scorings so far
        # archive_rescore = True, needs kv_cache_dtype (NOT in the reference; scores taken on e4m3 keys are another rule than
        # scores taken on 16-bit keys, and what that does to answer quality is not evaluated): video_budget_rescore and
        # `focus` score the archive's key rows as they lie - K = dtype(float(code) * scale), dequantised where the kernel
        # loads a key (rtk_pivotkv_rescore_fp8k_batched).  False (default): both refuse a cache with kv_cache_dtype, as ever
        self.archive_rescore = False
        # MI355X build option, a top-level key of longvideo_kwargs (build_kvcache reads it; NOT in the reference, a rule of
        # this project's own - answer quality is not evaluated): video_position_limit = P, an int >= 0, needs a window or a
        # budget.  A move drops rows but leaves every surviving id where it was, so the ids of a stream that does not end grow
        # without bound.  With the key on, an `after_forward` that has just moved a layer's rows looks - on the device - at
        # the layer's temporal ids: if the region's last id has reached P and its first id lies more than one past the
        # pinned rows' last, the region's ids are shifted down to follow the pinned rows and its keys re-rotated by the same
        # delta in place (_video_bound.rebase_positions).  P = 0 re-bases at every move: ids then equal "position in cache",
        # and every row of the region is re-rounded to the storage dtype once per move (half an ulp each time, DESIGN.md
        # §5) - a higher P trades id range for fewer roundings.  None (default): off, nothing changes, bit for bit.
        self.video_position_limit = None
        # video_position_gap = G, an int >= 1, needs video_position_limit (again NOT in the reference and a rule of this
        # project's own - answer quality is not evaluated): the delta becomes one per ROW.  Besides the gap behind the pinned
        # rows, every inner id gap above G closes to G (gaps <= G stay, 0 and negative ones included) and each key is
        # re-rotated by its own row's delta (_video_bound.rebase_positions).  Under the budget an old survivor keeps the
        # region's first id low, so without this key the uniform delta stays 0 and the last id grows unbounded.  A
        # renumbered region of n rows spans at most 1 + (n - 1) G ids: P must exceed pinned + (rows + slack + a chunk's
        # kept rows) G, or every move triggers and re-rounds nearly every row.  None (default): the uniform re-base.
        self.video_position_gap = None
        self._position_offsets: Dict[Any, torch.Tensor] = {}   # per device: int64 [layers], the cumulative deltas
        self.window_dropped: List[int] = []   # per layer: rows the window has dropped so far (also counted as evicted)
        self.budget_dropped: List[int] = []   # ... and the budget
        self._attn_ws: Dict[Any, torch.Tensor] = {}
        # page-sparse decode (not in the reference, a rule of this project's own - answer quality is not evaluated): the
        # functions of retake/_sparse_decode.py take the cache - sparse_decode(cache, keep_rows) arms, dense_decode(cache)
        # disarms.  They are NOT bound as methods: the class keeps exactly the names it had, and the state lives here
        self._sparse = None               # the page index while armed (None: off, `attention` is exactly as without it)
        self.sparse_attention_calls = 0   # attention calls that took rtk_attention_decode_sparse (an fp8 cache: _sparse_fp8kv; wide=True: _sparse_wide)
        self.page_summary_calls = 0       # rtk_pivotkv_page_summary_batched (_fp8k_batched) calls so far (one per device and arming)

    def attention(self, query_states, key_states, value_states, *, scaling=None, query_offset=None, layer_idx=None):
        """The chunk's attention over the views `update` / `update_pre_rope` / `append_pre_rope` returned, in one HIP
        launch (see chunk_attention).  [1, Lq, Hq, D], or None when the library declines the shape.
        kv_cache_dtype="fp8_e4m3": `layer_idx` names the layer whose archive precedes those views; query_offset counts
        over archive + views; a shape the library declines raises NotImplementedError (no other route reads the archive)."""
        archive = shared = None
        if self._sparse is not None:   # _sparse_decode.sparse_decode armed: the page-sparse call where it serves, else the routes below
            out = _sparse_decode.route(self, query_states, key_states, value_states, scaling, query_offset, layer_idx)
            if out is not None:
                self.attention_calls += 1
                return out
        if self.kv_cache_dtype is not None:
            if layer_idx is None:
                raise ValueError("PivotKVCache.attention needs layer_idx when kv_cache_dtype is set")
            archive = self.archive(layer_idx)
        if self.forked_from is not None:   # a branch: key_states / value_states are its own rows, the parent's precede them
            self._branch_check()
            if layer_idx is None:
                raise ValueError("PivotKVCache.attention needs layer_idx on a branch (PivotKVCache.fork)")
            shared = self.shared(layer_idx)
        route = []
        out = chunk_attention(query_states, key_states, value_states, scaling=scaling, workspace=self._attn_ws,
                              query_offset=query_offset, archive=archive, packed_gqa=self.decode_attention == "packed",
                              route=route, shared=shared,
                              packed_wide=self.multi_token_attention == "packed"
                              and wide_dispatch(query_states.shape[1], key_states.shape[1], query_states.shape[2]))
        if out is not None:
            self.attention_calls += 1
            self.decode_attention_calls += route == ["packed"]
            self.wide_attention_calls += route == ["wide"]
        elif self.forked_from is not None:
            raise NotImplementedError("a branch (PivotKVCache.fork): the native chunk attention refuses this shape "
                                      f"({nv.lib.rtk_last_error().decode(errors='replace')}) and no other route reads the "
                                      "parent's rows")
        elif self.kv_cache_dtype is not None:
            raise NotImplementedError(f"kv_cache_dtype={self.kv_cache_dtype!r}: the native chunk attention refuses this shape "
                                      f"({nv.lib.rtk_last_error().decode(errors='replace')}) and no other route reads the fp8 rows")
        return out

    # ---- the fp8 archive (kv_cache_dtype="fp8_e4m3") -----------------------------------------------
    def archive_len(self, layer_idx) -> int:
        """Archived (fp8) rows of the layer; a pending chunk's kept rows are not among them until its flush."""
        if layer_idx is None or layer_idx >= len(self._layers):
            return 0
        return self._layers[layer_idx].len8

    def archive(self, layer_idx):
        """(k8, v8, k_scale, v_scale) views of the layer's archived rows - codes uint8 [1, Hkv, len8, D], scales fp32
        [1, Hkv, len8] - or None while nothing is archived."""
        n = self.archive_len(layer_idx)
        if not n:
            return None
        st = self._layers[layer_idx]
        return st.k8[:, :, :n], st.v8[:, :, :n], st.ks8[:, :, :n], st.vs8[:, :, :n]

    def _archive_reserve(self, st: _LayerStore, more: int, Hkv: int, D: int, device):
        need = st.len8 + more
        if st.k8 is not None and st.k8.shape[2] >= need:
            return
        cap = max(need, 2 * (st.k8.shape[2] if st.k8 is not None else 0), self.reserve_archive_tokens or 1024,
                  self._region_room(st, 0, more))
        new = [torch.empty((1, Hkv, cap, D), dtype=torch.uint8, device=device) for _ in range(2)] + \
              [torch.empty((1, Hkv, cap), dtype=torch.float32, device=device) for _ in range(2)]
        if st.len8:
            for t, old in zip(new, (st.k8, st.v8, st.ks8, st.vs8)):
                t[:, :, :st.len8].copy_(old[:, :, :st.len8])
        st.k8, st.v8, st.ks8, st.vs8 = new

    def _dense(self, st: _LayerStore, which: str):
        """key_cache[l] / value_cache[l] with archived rows: a dense DEQUANTISED COPY (a diagnostic, not a view) in the order
        [16-bit rows before the first archive write | archive | remaining 16-bit rows].  That is sequence order - row for
        row the order of position_cache[l] - for a prompt with ONE run of video chunks.  With text between two videos the
        second video's kept rows still join the archive, i.e. they come BEFORE the text rows that preceded them in the
        sequence, while position_cache[l] stays in sequence order: the two then no longer line up row for row (attention
        is unaffected: every archived row is visible to every later query)."""
        buf, codes, scales = (st.k, st.k8, st.ks8) if which == "k" else (st.v, st.v8, st.vs8)
        if st.base:   # a branch: the 16-bit rows are [the parent's rows it shares | its own]
            self._branch_check()
            buf = torch.cat([st.sk if which == "k" else st.sv, buf[:, :, :st.length]], dim=2)
        Hkv, D, n8, n16 = buf.shape[1], buf.shape[3], st.len8, st.base + st.length
        if not n8:
            return buf
        at = st.archive_at
        out = torch.empty((1, Hkv, n16 + n8, D), dtype=buf.dtype, device=buf.device)
        out[:, :, :at].copy_(buf[:, :, :at])
        out[:, :, at + n8:].copy_(buf[:, :, at:n16])
        fp8_dequantize_rows(codes[:, :, :n8], scales[:, :, :n8], buf.dtype, out[:, :, at:at + n8])
        return out

    def _fp8_refuse(self, dtype, D, reforge, rot, has_ids=True):
        """What kv_cache_dtype="fp8_e4m3" does not serve, raised by the first compressed update before anything is launched."""
        if self.kv_cache_dtype is None:
            return
        if reforge and not has_ids:
            raise NotImplementedError(f"kv_cache_dtype={self.kv_cache_dtype!r} with pos_embed_reforge needs the chunk's "
                                      "position ids: the archive kernel re-rotates the kept keys at their new ids")
        if dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"kv_cache_dtype={self.kv_cache_dtype!r} needs a bfloat16 or float16 model, got {dtype}")
        if D != 128:
            raise NotImplementedError(f"kv_cache_dtype={self.kv_cache_dtype!r} needs head_dim 128, got {D}")
        if reforge and rot is None:
            raise NotImplementedError(f"kv_cache_dtype={self.kv_cache_dtype!r} with pos_embed_reforge needs a rotary module of "
                                      "the static inv_freq * position kind (native RoPE): the archive kernel re-rotates the "
                                      "kept keys itself")

    # ---- diagnostics of the most recent compressed update (the selection may still be deferred: flush first) ----
    @property
    def last_scores(self):
        """Scores of the most recent compressed update; None if it kept its whole chunk without scoring it."""
        b, l = self._last_slot
        self._flush()
        if b.keep_all:
            return None
        return b.score[l, :b.Lv] if b.prompt else b.score[l]

    @property
    def last_keep_indices(self):
        b, l = self._last_slot
        self._flush()
        return b.keep_idx[l]

    def memory_footprint(self) -> Dict[str, int]:
        """Device bytes this cache holds right now, by what they are for (not in the reference; bench.py's `memory` block and
        tests/test_memory_gpu.py read it).  The reference's cache is the compressed rows only (longvideo_cache.py:313-318) -
        its transients (the [Hq, L, L] fp32 softmax and its casts, two torch.cat copies of the layer) come and go inside
        every update; here the transients are pre-allocated once per chunk geometry and reused:
          cache_rows        K / V / id rows of the committed tokens (what the reference's lists hold)
          cache_headroom    the rest of the pre-allocated K / V / id buffers: room for the in-flight chunk (the uncompressed
                            tail update() returns to the layer's attention) and for generation, or unused growth
          k_unrotated       per-slot copy of the chunk's un-rotated keys (re-rotated into the cache by the flush)
          score_operands    per-slot q~ (and the fast mode's fp16 k~) + row statistics of the deferred score passes
          score_partials    per-slot column partials, final scores, live-key lists
          selection         kept indices, ids of the pending chunk (old / new), selection scratch, compaction tickets
          staging           kept-row staging of the two-launch eviction (in_place_compaction=False / no reforge)
          deferred_queries  pre-RoPE queries kept alive for a flush that scores them where they lie (prologue_operands="pre_rope")
          worker_scratch    per-update scratch of the stage-by-stage route / worker streams
          attention_workspace  key-split partials of the native chunk attention (attention_kernel="hip"; few-row shapes only)
          row_scores        the fp32 score buffers of the video regions - the key exists only with video_budget_rows on
          observe_queries   the layers' last rotated query rows - the key exists only with video_budget_rescore on (the
                            re-scoring's scratch counts as worker_scratch)
          focus_queries     the layers' watched query rows - the key exists only while watch_question is armed
          page_summaries    the per-page key bounds of the page-sparse decode, and
          sparse_workspace  the per-layer workspaces of its calls (bounds, page lists, partials) - the keys exist only
                            while sparse_decode is armed."""
        def nbytes(t):
            return 0 if t is None else t.numel() * t.element_size()

        out = dict.fromkeys(("cache_rows", "cache_headroom", "k_unrotated", "score_operands", "score_partials", "selection",
                             "staging", "deferred_queries", "worker_scratch", "attention_workspace"), 0)
        for st in self._layers:
            if st.k is not None:
                row = 2 * st.k.shape[1] * st.k.shape[3] * st.k.element_size()
                out["cache_rows"] += row * st.length
                out["cache_headroom"] += nbytes(st.k) + nbytes(st.v) - row * st.length
            if st.k8 is not None:   # fp8 archive: D codes + one fp32 scale per (kv head, row), K and V
                row8 = 2 * st.k8.shape[1] * (st.k8.shape[3] + 4)
                out["cache_rows"] += row8 * st.len8
                out["cache_headroom"] += nbytes(st.k8) + nbytes(st.v8) + nbytes(st.ks8) + nbytes(st.vs8) - row8 * st.len8
            if st.pos is not None:
                out["cache_rows"] += 8 * st.pos.shape[0] * st.pos_len
                out["cache_headroom"] += nbytes(st.pos) - 8 * st.pos.shape[0] * st.pos_len
        b = self._batch
        if b is not None:
            out["k_unrotated"] = nbytes(b.k_unrot)
            out["score_operands"] = nbytes(b.score_ws)
            out["score_partials"] = nbytes(b.partials) + nbytes(b.score) + nbytes(b.key_index) + nbytes(b.prompt_ws)
            out["selection"] = (nbytes(b.keep_idx) + nbytes(b.pos_new) + nbytes(b.pos_old) + nbytes(b.sel_ws) + nbytes(b.pos_video)
                                + nbytes(b.compact_sync) + nbytes(b.cos_new) + nbytes(b.sin_new))
            out["staging"] = nbytes(b.v_stage) + nbytes(b.k_stage)
            seen = set()
            for t in b.q_keep:
                if t is not None and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    out["deferred_queries"] += nbytes(t)
        if self.video_budget_rows is not None:
            out["row_scores"] = sum(nbytes(st.sc) for st in self._layers)
        if self.video_budget_rescore is not None:
            out["observe_queries"] = sum(nbytes(st.oq) for st in self._layers)
        if self._watch is not None:
            out["focus_queries"] = _focus.watched_bytes(self)
        if self._sparse is not None:
            out.update(_sparse_decode.sparse_bytes(self))
        out["worker_scratch"] = sum(nbytes(t) for t in self._ws.values()) + sum(nbytes(t) for sd in self._sides for t in sd.ws.values())
        out["attention_workspace"] = sum(nbytes(t) for t in self._attn_ws.values())
        out["total"] = sum(out.values())
        return out

    # ---- mark / rewind / crop, and fork: a branch reads the parent's rows where they lie: functions of _marks, bound as methods
    video_end = property(_marks.video_end)
    _take_mark, mark, set_resume_position_ids = _marks._take_mark, _marks.mark, _marks.set_resume_position_ids
    _mark_is_dead, _kill_marks_after, _check_mark = _marks._mark_is_dead, _marks._kill_marks_after, _marks._check_mark
    rewind, _after_rewind, _crop_floor, crop = _marks.rewind, _marks._after_rewind, _marks._crop_floor, _marks.crop
    shared_len, shared, fork, _branch_check = _marks.shared_len, _marks.shared, _marks.fork, _marks._branch_check
    _branch_refuse_write, _branch_update_check = _marks._branch_refuse_write, _marks._branch_update_check

    # ---- list views --------------------------------------------------------------------------
    @property
    def key_cache(self):
        return self._kview

    @key_cache.setter
    def key_cache(self, value):  # the base class assigns [] in __init__
        self._branch_refuse_write()
        self._flush()
        self._epoch += 1
        self._layers = []
        for v in value:
            self._kview.append(v)

    @property
    def value_cache(self):
        return self._vview

    @value_cache.setter
    def value_cache(self, value):
        self._branch_refuse_write()
        self._epoch += 1
        for i, v in enumerate(value):
            if i >= len(self._layers):
                self._layers.append(_LayerStore())
            if not (isinstance(v, list) and len(v) == 0):
                self._adopt(i, "v", v)

    def _adopt(self, i: int, which: str, value):
        self._branch_refuse_write()
        if getattr(self, "kv_cache_dtype", None) is not None:
            raise NotImplementedError(f"kv_cache_dtype={self.kv_cache_dtype!r}: key_cache / value_cache are dequantised copies "
                                      "of [16-bit rows | archive]; assigning through them is not supported")
        st = self._layers[i]
        if st.pending:
            self._flush()
        self._epoch += 1
        st.pinned = -1   # (video_window_rows: a layer replaced wholesale pins what it holds at its next compressed chunk)
        st.sc_len = st.sc_seen = 0    # (video_budget_rows: ... and its region starts afresh there)
        if isinstance(value, list) and len(value) == 0:
            st.k = st.v = None
            st.length = 0
            return
        if which == "k":
            st.k = value
            st.length = value.shape[2]
        else:
            st.v = value

    def get_seq_length(self, layer_idx: int = 0) -> int:
        if len(self._layers) <= layer_idx or self._layers[layer_idx].k is None:
            return 0
        st = self._layers[layer_idx]
        return st.base + st.length + st.len8 + (st.pending_keep if st.pending else 0)

    def __len__(self):
        return len(self._layers)

    def __getitem__(self, layer_idx):
        return self.key_cache[layer_idx], self.value_cache[layer_idx]

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    # ---- position ids of the cached tokens (reference :143, :179-215) -----------------------------
    def _pos_view(self, st: _LayerStore):
        v = st.pos[:, :st.pos_len]
        return v.unsqueeze(1) if st.pos_ndim == 3 else v

    @property
    def position_cache(self):
        """Per-layer position ids of the cached tokens (reference :143): a list of [3, 1, n] / [1, n] views
        of the layers' id buffers, [] for skipped layers.  Reading it flushes deferred work."""
        self._flush()
        out = []
        for i in range(self._pos_layers):
            st = self._layers[i] if i < len(self._layers) else None
            out.append([] if st is None or st.pos is None else self._pos_view(st))
        return out

    @position_cache.setter
    def position_cache(self, value):
        self._branch_refuse_write()
        self._flush()
        self._epoch += 1
        self._pos_layers = len(value)
        for i, t in enumerate(value):
            st = self._store(i)
            if isinstance(t, list) and len(t) == 0:
                st.pos, st.pos_len, st.pos_ndim = None, 0, 0
            else:
                st.pos_ndim = t.ndim
                st.pos = t.reshape(t.shape[0], t.shape[-1]).contiguous()
                st.pos_len = t.shape[-1]

    def _pos_reserve(self, st: _LayerStore, P: int, ndim: int, more: int, device):
        need = st.pos_len + more
        if st.pos is not None and st.pos.shape[1] >= need:
            return
        first = st.archive_at if self.kv_cache_dtype is not None else st.pinned
        first = first if first >= 0 else st.pos_len
        cap = max(need, 2 * (st.pos.shape[1] if st.pos is not None else 0), 4096, self.reserve_tokens + self.reserve_archive_tokens,
                  self._region_room(st, first, more))
        buf = torch.empty((P, cap), dtype=torch.int64, device=device)
        if st.pos is not None and st.pos_len:
            buf[:, :st.pos_len].copy_(st.pos[:, :st.pos_len])
        st.pos, st.pos_ndim = buf, ndim

    # ---- hooks (reference :146-150): after_forward is where deferred compaction is flushed -------
    def before_forward(self, **kwargs):
        if self.prompt_guided_scoring:   # (off: the reference's `pass`)
            n = kwargs.get("prompt_length")
            self._prompt_len = int(n) if n is not None and int(n) > 0 else 0

    def after_forward(self, **kwargs):
        """The reference's hook after every forward of a video chunk (:146-150): the deferred eviction of the chunk is
        flushed, the sliding window (video_window_rows) or the video budget (video_budget_rows) - which act here and
        nowhere else: a caller that never calls after_forward gets neither - drops what exceeds it, and
        `video_end` is taken."""
        self._flush()
        self._prompt_len = 0
        if self._compressed_in_forward:   # the work is flushed: a few tuples per chunk
            self._compressed_in_forward = False
            if self.video_window_rows is not None:
                _video_bound.slide_window(self)
            elif self.video_budget_rows is not None:
                if self.video_budget_rescore is not None:
                    _video_bound.rescore_budget(self)
                _video_bound.evict_budget(self)
            if not self.defer_rerotation:
                self.last_compressed_mark = self._take_mark(True)

    def _prompt_rows(self, L: int) -> int:
        """Prompt rows of a chunk of L rows arriving now: the recorded prompt_length if 0 < Lp < L, else 0 (an ordinary chunk)."""
        n = self._prompt_len
        return n if 0 < n < L else 0

    # ---- the bounded video region (video_window_rows / video_budget_rows): functions of _video_bound, bound as methods
    _region_room, _keep_scores, row_scores = _video_bound.region_room, _video_bound.keep_scores, _video_bound.row_scores
    position_offset, observed_queries = _video_bound.position_offset, _video_bound.observed_queries

    # ---- the question-focused decode cache: functions of _focus, bound as methods
    watch_question, unwatch_question, watched_queries = _focus.watch_question, _focus.unwatch_question, _focus.watched_queries
    focus, focus_scores, focus_kept = _focus.focus, _focus.focus_scores, _focus.focus_kept

    # ---- bookkeeping lists (reference :152-215) ------------------------------------------------
    def update_num_evicted_tokens(self, num_tokens: int, layer_idx: int):
        """num_evicted_tokens[layer] += num_tokens, padding skipped layers with 0 (longvideo_cache.py:152-177)."""
        if len(self.num_evicted_tokens) <= layer_idx:
            self.num_evicted_tokens.extend([0] * (layer_idx - len(self.num_evicted_tokens)))
            self.num_evicted_tokens.append(num_tokens)
        else:
            self.num_evicted_tokens[layer_idx] += num_tokens
        return self.num_evicted_tokens[layer_idx]

    def update_position_ids(self, position_ids: torch.Tensor, layer_idx: int):
        """position_cache[layer] = cat(prev, position_ids, dim=-1), padding skipped layers with []
        (longvideo_cache.py:179-209).  The ids are appended to the layer's pre-allocated id buffer."""
        st = self._store(layer_idx)
        if st.pending:
            self._flush()
        n = position_ids.shape[-1]
        P = position_ids.shape[0]
        self._pos_reserve(st, P, position_ids.ndim, n, position_ids.device)
        st.pos[:, st.pos_len:st.pos_len + n].copy_(position_ids.reshape(P, n))
        st.pos_len += n
        self._pos_layers = max(self._pos_layers, layer_idx + 1)
        return self._pos_view(st)

    def get_prev_temporal_idx(self, layer_idx: int):
        """Last temporal id stored for the layer, -1 if none (longvideo_cache.py:211-215)."""
        if layer_idx >= self._pos_layers and not (len(self._layers) > layer_idx and self._layers[layer_idx].pending):
            return -1
        st = self._layers[layer_idx]
        if st.pending:
            self._flush()  # the ids of the previous chunk are still in the batch
        if layer_idx >= self._pos_layers or st.pos is None or st.pos_len == 0:
            return -1
        return st.pos[0, st.pos_len - 1]

    def _shift_latch_check(self):
        """The in-launch id shift (RTK_UPDATE_SHIFT_NEXT) bounds its wait; a wait that ran out shifted NOTHING and latched a
        host-visible word.  Every entry point looks at it (one read of pinned host memory, no device sync) before it
        trusts ids a launch was supposed to have shifted - same policy as p2p.check(): a bounded wait that gives up is an
        error, never a silent continuation."""
        b = self._batch
        if b is not None and b.shift_latch is not None and b.shift_latch[0]:
            self._shift_failed(b)

    def _shift_failed(self, b: "_Batch"):
        n = int(b.shift_latch[0])
        self._preshifted = None
        self.shift_next_in_update = False     # this cache goes back to one shift launch per layer
        try:   # put the words back (the failed launches left residue in the counters, the latch stops every later watcher)
            torch.cuda.synchronize(b.device)
            b.shift_ticket.zero_()
            torch.cuda.synchronize(b.device)
        except Exception:  # noqa: BLE001  (the error below is the one to report)
            pass
        b.shift_latch[0] = 0
        b.shift_stream = None
        raise RuntimeError(
            f"PivotKVCache: the in-launch position-id shift of {n} update launch(es) ran out of its bounded wait and shifted "
            "nothing (the arrival counters were not zero at launch: were update launches of one cache issued on two streams "
            "at once?).  The layers after the first such launch ran on UNSHIFTED temporal ids: the cache contents of the "
            "current video are invalid - rebuild the cache.  The feature is now off for this cache (one rtk_position_shift "
            "launch per layer).")

    def check(self):
        """Synchronise the cache's device and raise if a bounded device-side wait of this cache has run out (the in-launch
        id shift).  The entry points look at the latch on every call without synchronising; call this after the last
        update of a run when nothing else of the cache is called before its contents are used."""
        b = self._batch
        if b is not None and b.device.type == "cuda":
            torch.cuda.synchronize(b.device)
        self._shift_latch_check()

    def shift_temporal_ids_(self, position_ids: torch.Tensor, layer_idx: int):
        """The attention patch's continuity fix (qwen2_vl.py:68-73, llava_onevision.py:68-72) on the device:
        position_ids[0, 0, :] (or [0, :]) += prev + 1 - its first element, in place, where prev is the last
        temporal id cached for the layer.  Same result as the reference's compare-then-shift, without the
        host round trip of the comparison."""
        if not self.pos_embed_reforge:
            return position_ids
        return self._shift_row(position_ids, layer_idx)

    def _shift_row(self, position_ids: torch.Tensor, layer_idx: int):
        if not position_ids.is_cuda:
            nv.require_device(position_ids)
        if position_ids.dtype is not torch.int64 or position_ids.stride(-1) != 1:
            row = position_ids[0, 0] if position_ids.ndim == 3 else position_ids[0]
            prev = self.get_prev_temporal_idx(layer_idx)
            row += prev + 1 - row[0].clone()
            return position_ids
        self._shift_latch_check()   # (before the memo below is trusted)
        done, self._preshifted = self._preshifted, None
        idx = position_ids.get_device()
        if done is not None and done[0]() is position_ids and done[1] is not None and done[1] == _version_of(position_ids) \
                and done[2] == layer_idx and nv.current_device() == idx and done[3] == nv.raw_stream(idx):
            return position_ids   # the previous layer's update launch has shifted this very tensor for this layer
        prev_ptr = None
        if len(self._layers) > layer_idx:
            c = self._layers[layer_idx].c
            if c.pending:
                self._flush()
            if layer_idx < self._pos_layers and c.pos and c.pos_len:
                prev_ptr = c.pos + 8 * (c.pos_len - 1)
        # the temporal row ([0, 0, :] of [3, 1, n] ids, [0, :] of [1, n] ids) starts at the tensor's first element
        nv.check(_on_device(idx, nv.lib.rtk_position_shift, position_ids.data_ptr(), position_ids.shape[-1], prev_ptr,
                            nv.raw_stream(idx)), "rtk_position_shift")
        return position_ids

    # ---- storage -------------------------------------------------------------------------------
    def _store(self, layer_idx: int) -> _LayerStore:
        while len(self._layers) <= layer_idx:
            self._layers.append(_LayerStore())
        return self._layers[layer_idx]

    def reserve(self, layer_idx: int, tokens: int, like: torch.Tensor):
        """Make room for `tokens` more rows after the committed length of the layer."""
        st = self._store(layer_idx)
        need = st.length + tokens
        if st.k is not None and st.k.shape[2] >= need and st.k.is_contiguous() and st.v.is_contiguous() \
                and st.v.shape[2] == st.k.shape[2]:
            return st
        first = st.pinned if st.pinned >= 0 else st.length
        room = 0 if self.kv_cache_dtype is not None else self._region_room(st, first, tokens)
        cap = max(need, 2 * (st.k.shape[2] if st.k is not None else 0), 1024, self.reserve_tokens, room)
        shape = (1, like.shape[1], cap, like.shape[3])
        nk = torch.empty(shape, dtype=like.dtype, device=like.device)
        nvv = torch.empty(shape, dtype=like.dtype, device=like.device)
        if st.k is not None and st.length:
            nk[:, :, :st.length].copy_(st.k[:, :, :st.length])
            nvv[:, :, :st.length].copy_(st.v[:, :, :st.length])
        st.k, st.v = nk, nvv
        return st

    def _buf(self, name: str, shape, dtype, device, ws: Optional[dict] = None) -> torch.Tensor:
        ws = self._ws if ws is None else ws
        t = ws.get(name)
        n = 1
        for s in shape:
            n *= s
        if t is None or t.numel() < n or t.dtype != dtype or t.device != device:
            t = torch.empty(max(n, 1), dtype=dtype, device=device)
            ws[name] = t
        return t[:n].view(*shape)

    _STATIC_ROPE_TYPES = ("default", "linear", "yarn", "llama3", "mrope")

    def _rotary(self, rotary_emb_fn, device) -> Optional[_Rotary]:
        """The native-RoPE view of a rotary module, or None when the module has to be called (reference :249, :298).
        Memoised per module object; modules with equal inv_freq / attention_scaling (HF: one per layer) share one
        entry, so a chunk's layers stay in one batch."""
        hit = self._rotaries.get(id(rotary_emb_fn))
        if hit is not None and hit[0] is rotary_emb_fn and (hit[1] is None or hit[1].device == device) \
                and hit[2] == _inv_stamp(rotary_emb_fn):
            return hit[1]
        entry = None
        inv = getattr(rotary_emb_fn, "inv_freq", None)
        if (self.native_rope and isinstance(inv, torch.Tensor) and hasattr(rotary_emb_fn, "attention_scaling")
                and getattr(rotary_emb_fn, "rope_type", "default") in self._STATIC_ROPE_TYPES):
            inv = inv.detach().to(device=device, dtype=torch.float32).contiguous()
            scaling = float(rotary_emb_fn.attention_scaling)
            for _, other, _ in self._rotaries.values():
                if (other is not None and other.device == device and other.scaling == scaling
                        and other.inv.shape == inv.shape and torch.equal(other.inv, inv)):
                    entry = other
                    break
            if entry is None:
                entry = _Rotary(inv, scaling, device)
        # (the strong reference pins the id; the stamp notices a module whose inv_freq was replaced or written in place)
        self._rotaries[id(rotary_emb_fn)] = (rotary_emb_fn, entry, _inv_stamp(rotary_emb_fn))
        return entry

    def _rope_tables(self, cos_t, sin_t, rotary_emb_fn, x_like, pos2d, pos_ld, ndim, sec, n, D):
        """fp32 [n, D] cos/sin tables of the ids pos2d [P, n] (row stride pos_ld), section-merged
        (reference :249 / :298 + :68-74; `sec`: the batch's M-RoPE sections array or None), into cos_t / sin_t."""
        dev = x_like.device
        P = pos2d.shape[0]
        nsec = len(sec) if sec is not None else 0
        s = nv.stream()
        rot = self._rotary(rotary_emb_fn, dev)
        if rot is not None:
            nv.check(nv.lib.rtk_rope_table(nv.ptr(pos2d), pos_ld, P, n, nv.ptr(rot.inv), D, rot.scaling, sec, nsec,
                                           nv.round_mode(x_like.dtype), nv.ptr(cos_t), nv.ptr(sin_t), s),
                     "rtk_rope_table")
            return
        ids = pos2d.unsqueeze(1) if ndim == 3 else pos2d
        cos, sin = rotary_emb_fn(x_like, ids)  # third-party module, exactly as the reference calls it
        cos = cos.reshape(P, n, D)
        sin = sin.reshape(P, n, D)
        if not cos.is_contiguous():
            cos = cos.contiguous()
        if not sin.is_contiguous():
            sin = sin.contiguous()
        nv.check(nv.lib.rtk_rope_merge(nv.ptr(cos), nv.ptr(sin), P, n, D, nv.dtype_code(cos), sec, nsec, nv.ptr(cos_t),
                                       nv.ptr(sin_t), s), "rtk_rope_merge")

    # ---- deferred eviction -----------------------------------------------------------------------
    def _get_batch(self, layer_idx, Hq, Hkv, L, D, keep, P, dtype, device, prompt=0) -> _Batch:
        refround = self.score_rounding == "reference" and dtype in (torch.bfloat16, torch.float16)
        if refround and D != 128:
            raise NotImplementedError("score_rounding='reference' needs head_dim 128")
        # "fast" (opt in): bf16 chunks of head_dim 128 on the fp16 matrix instruction; every other shape scores as usual
        fast = self.score_rounding == "fast" and dtype == torch.bfloat16 and D == 128
        keep_all = keep == L and not self.score_when_keeping_all
        defer = bool(self.defer_rerotation and self.pos_embed_reforge)
        key = (Hq, Hkv, L, D, keep, P, bool(self.pos_embed_reforge), dtype, device, refround, fast, keep_all, defer, prompt)
        b = self._batch
        wrap = self.flush_every_layers > 0
        if b is not None and b.key == key and (layer_idx < b.slots or b.wrap) and b.wrap == wrap:
            return b
        self._flush()
        if wrap:
            slots = min(self.flush_every_layers, max(int(self.num_hidden_layers), 1))
        else:
            slots = max(int(self.num_hidden_layers), layer_idx + 1, b.slots if b is not None and b.key == key else 0)
        self._batch = None  # release the old buffers before allocating the new ones
        self._batch = _Batch(key, slots, Hq, Hkv, L, D, keep, P, bool(self.pos_embed_reforge), dtype, device, refround, fast,
                             keep_all, self.skip_masked_columns, self.in_place_compaction, prompt)
        self._batch.wrap = wrap
        self._batch.defer = defer
        self._batch.c.defer_rot = int(defer)
        return self._batch

    def _claim_slot(self, b: _Batch, layer_idx: int) -> int:
        """The layer's slot in the batch; with flush_every_layers the pending units are flushed first when that slot (or
        a later one: the slots of a flush ascend with its layers) is still taken."""
        sl = b.slot(layer_idx)
        if b.wrap and b.pending and (sl <= b.slot(b.pending[-1]) or layer_idx <= b.pending[-1]):
            self._flush()
        return sl

    # the flush of a chunk's pending units, once per chunk: functions of _flush, bound as methods
    _flush, _flush_c, _flush_general, _wait_workers = _fl._flush, _fl._flush_c, _fl._flush_general, _fl._wait_workers
    _shift_pending_ids, _score_unscored, _score_prompt_run = _fl._shift_pending_ids, _fl._score_unscored, _fl._score_prompt_run
    _select_units, _select_prompt_units, _select_unselected = _fl._select_units, _fl._select_prompt_units, _fl._select_unselected
    _new_id_tables, _scan_unit, _evict_staged = _fl._new_id_tables, _fl._scan_unit, _fl._evict_staged
    _archive, _compact, _advance_layers, _end_flush = _fl._archive, _fl._compact, _fl._advance_layers, _fl._end_flush
    _order_compaction, _reset_compaction = _fl._order_compaction, _fl._reset_compaction

    # ---- the hot path ---------------------------------------------------------------------------
    def _entry_guard(self, who: str):
        """What `update`, `update_pre_rope` and `append_pre_rope` (`who`) check first, in this order."""
        if self.forked_from is not None:
            self._branch_update_check(who)
        if self.focused_from is not None:
            _focus.refuse_compression(self, who)
        self._shift_latch_check()

    def update(
        self,
        key_states: torch.Tensor,
        value_states: torch.Tensor,
        layer_idx: int,
        cache_kwargs: Optional[Dict[str, Any]] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        Input
            query_states: [bsz, num_heads, q_len, d]      (cache_kwargs['query_states'], post-RoPE)
            key_states:   [bsz, num_key_value_heads, q_len, d]
            position_ids: [3, bsz, q_len] / [bsz, q_len]  (cache_kwargs['position_ids'])
        Output
            key_states_output, value_states_output: the layer's UNCOMPRESSED keys/values
            ([prefix | whole current chunk]) for this layer's self attention (reference :217-323).

        A chunk whose geometry matches the current batch goes through ONE library call (rtk_pivotkv_update: argument
        blocks bound once per batch and per layer); everything else - the first update of a geometry, text / decode
        appends, worker streams, small chunks, rotary modules that must be called - through `_update_general`.

        Like the reference, `update` pops position_ids / query_states / rotary_emb / mrope_section from `cache_kwargs` and
        leaves every tensor it is handed untouched - with ONE opt-in exception the reference does not have:
        cache_kwargs["shift_next_position_ids"] = True lets the launch apply the NEXT layer's continuity shift
        (qwen2_vl.py:68-73) to `position_ids` in place, i.e. after update(l) the caller's ids tensor may already carry layer
        l + 1's temporal offset.  Only a caller that shares one ids tensor between its layers and shifts it in place itself
        (the Qwen2-VL attention patch: `shift_temporal_ids_` then finds the shift done) should set it.
        """
        self._entry_guard("PivotKVCache.update")
        b = self._batch
        if b is not None and b.c_capable and cache_kwargs is not None and self.kvcache_compression \
                and self.overlap_streams <= 0 and self.one_call_update and b.prompt == self._prompt_rows(b.L):
            out = self._update_c(b, key_states, value_states, layer_idx, cache_kwargs, None)
            if out is not None:
                return out
        return self._update_general(key_states, value_states, layer_idx, cache_kwargs)

    def _update_c(self, b: _Batch, key_states, value_states, layer_idx, ck, q0, shift_ids_in_place=True, q_out=None):
        """One rtk_pivotkv_update call.  q0 None: `ck["query_states"]` / key_states are rotated (the reference's
        protocol); else q0 / key_states are the pre-RoPE projections and the rotated queries are written over q0.
        Returns None - having changed nothing - when the call does not fit the batch."""
        q = ck.get("query_states") if q0 is None else q0
        pos = ck.get("position_ids")
        if q is None or pos is None or (layer_idx >= b.slots and not b.wrap) or layer_idx >= len(self._layers):
            return None
        if not self._bound_rotary(b, ck.get("rotary_emb")) or ck.get("mrope_section") != b.mrope_section:
            return None
        dt = b.dtype
        if q.shape != b.qshape or key_states.shape != b.kshape or value_states.shape != b.kshape \
                or q.dtype is not dt or key_states.dtype is not dt or value_states.dtype is not dt:
            return None
        idx = b.dev_index
        if not (q.is_cuda and q.get_device() == idx and key_states.get_device() == idx
                and value_states.get_device() == idx and pos.is_cuda and pos.get_device() == idx
                and nv.current_device() == idx):
            return None
        L, P = b.L, b.P
        if pos.dtype is not torch.int64 or pos.shape[-1] != L or pos.shape[0] != P or pos.ndim != b.pos_ndim \
                or pos.stride(-1) != 1 or (pos.ndim == 3 and (pos.shape[1] != 1 or pos.stride(0) < L)):
            return None   # (ids whose rows alias - `.expand(3, ..)` - take the stage-by-stage route)
        mask = self.keypatches_mask_chunk
        if mask is None:
            mptr = None
        elif mask is b.mask_obj:
            mptr = b.mask_ptr
        else:
            if not (mask.is_cuda and mask.dtype is torch.bool and mask.numel() in (L, b.Lv) and mask.is_contiguous()
                    and mask.get_device() == idx):   # (prompt-guided units: the mask may cover the video rows only)
                return None
            b.mask_obj, b.mask_ptr = mask, mask.data_ptr()
            mptr = b.mask_ptr
        st = self._layers[layer_idx]
        c = st.c
        if c.pending:
            self._flush()
        P0 = c.length
        if P0 + L > c.cap:   # (cap is 0 for buffers the library may not use)
            return None
        pre = q0 is not None
        roundtrip = pre and self.prologue_operands == "reference"
        mode = (2 if roundtrip else 1) if pre else 0
        if b.pending and b.c.pre_rope != mode:
            self._flush()
        slot = self._claim_slot(b, layer_idx)
        b.c.pre_rope = mode   # what the units of this batch's next flush were appended from
        qs, ks, vs = q.stride(), key_states.stride(), value_states.stride()
        if qs[3] != 1 or ks[3] != 1 or vs[3] != 1:
            return None
        io = b.io
        stream = nv.raw_stream(idx)
        _fill_io(io, q, qs, key_states, ks, value_states, vs, pos)
        q_in_place = False
        if pre:
            rt = nv.RTK_UPDATE_ROUNDTRIP if roundtrip else 0
            if q_out is None or q_out is q:
                io.q_rot, io.qr_stride_h, io.qr_stride_l, io.flags = io.q, qs[1], qs[2], nv.RTK_UPDATE_PRE_ROPE | rt
            else:
                io.q_rot, io.qr_stride_h, io.qr_stride_l = q_out.data_ptr(), q_out.stride(1), q_out.stride(2)
                # the rotated queries go elsewhere, so q0 survives: the batched passes score it where it lies
                q_in_place = self._scores_q0_in_place(b)
                io.flags = nv.RTK_UPDATE_PRE_ROPE | rt | (nv.RTK_UPDATE_Q_IN_PLACE if q_in_place else 0)
        else:
            io.q_rot, io.flags = None, 0
            # the NEXT layer's continuity shift rides in this launch (its `shift_temporal_ids_` then finds it done) - for a
            # caller that asked for it (it writes the caller's ids: the attention patch's own in-place shift, one layer
            # early), and only where the library cannot decline AFTER the launch (batched passes / keep-all batches)
            nxt = False
            if self.shift_next_in_update and ck.get("shift_next_position_ids") and (b.batched_passes or b.keep_all) \
                    and b.shift_latch is not None:
                nxt = self._next_layer_prev(layer_idx, idx)
            if nxt is not False:
                io.flags, io.next_prev = nv.RTK_UPDATE_SHIFT_NEXT, nxt
                # the arrival counters serve ONE launch at a time: launches that share them are ordered on one stream.  A
                # caller that switched its current stream between two layers first waits for the device (rare)
                if b.shift_stream is not None and b.shift_stream != stream:
                    torch.cuda.synchronize(b.device)
                b.shift_stream = stream
        self._preshifted = None
        c.mask = mptr
        rc = nv.lib.rtk_pivotkv_update(b.cref, st.cref, slot, b.ioref, stream)
        if rc:
            c.mask = None
            if rc == nv.RTK_EUNSUPPORTED:
                # declined BEFORE anything was launched - also with the in-launch shift: the library only accepts that flag
                # where nothing can decline after the prepare launch (include/retake_hip.h, RTK_UPDATE_SHIFT_NEXT)
                return None
            nv.check(rc, "rtk_pivotkv_update")
        if io.flags & nv.RTK_UPDATE_SHIFT_NEXT:
            self._preshifted = (weakref.ref(pos), _version_of(pos), layer_idx + 1, stream)
        if st.pinned < 0:    # the layer's first compressed chunk: what it held before it is pinned (video_window_rows)
            st.pinned = P0
        if self.video_budget_rescore is not None:   # the rotated queries lie in q (in place) or in q_out
            _video_bound.observe(self, st, q if (not pre or q_out is None) else q_out)
        if not self._warned:
            self._warn_compression()
        if not pre:  # the reference's cache_kwargs protocol (:235, :241-243)
            ck.pop("position_ids", None)
            ck.pop("query_states", None)
            ck.pop("rotary_emb", None)
            ck.pop("mrope_section", None)
            ck.pop("shift_next_position_ids", None)   # (the build's own key)
        else:
            if shift_ids_in_place:     # the flush shifts the caller's ids in place (qwen2_vl.py:73)
                b.shift_ids = pos
                b.c.shift_row = io.pos
        nev = self.num_evicted_tokens
        if len(nev) > layer_idx:
            nev[layer_idx] += L - b.keep   # reference :310
        else:
            self.update_num_evicted_tokens(L - b.keep, layer_idx)
        if mask is not None:
            b.masks[layer_idx] = mask
        b.q_keep[slot] = q if q_in_place else None
        if b.keep_all or not b.batched_passes:   # nothing to score, or scored inside the call
            b.scored.add(layer_idx)
        b.pending.append(layer_idx)
        b.c_pending += 1
        self._compressed_in_forward = True
        self._last_slot = (b, slot)
        n = P0 + L
        return st._k.narrow(2, 0, n), st._v.narrow(2, 0, n)

    def _next_layer_prev(self, layer_idx: int, dev_index: int):
        """Address of the last temporal id cached for layer_idx + 1 (None: nothing cached, the rule's prev = -1), or
        False when this launch must not shift for it: there is no such layer, its previous chunk is still pending, or its
        ids live on another device (a model spread over GPUs by device_map: that layer gets its own launch there)."""
        nxt = layer_idx + 1
        if nxt >= int(self.num_hidden_layers):
            return False
        if len(self._layers) > nxt:
            st = self._layers[nxt]
            c = st.c
            if c.pending:
                return False
            if nxt < self._pos_layers and c.pos and c.pos_len:
                if st.pos is None or st.pos.get_device() != dev_index:
                    return False
                return c.pos + 8 * (c.pos_len - 1)
        return None

    def _scores_q0_in_place(self, b: _Batch) -> bool:
        """Can the chunk-batched passes read the pre-RoPE queries where they lie?  Only when q~ IS q0."""
        return bool(b.batched_passes and not b.fast and not b.keep_all and self.score_queries_in_place
                    and self.prologue_operands == "pre_rope")

    def update_pre_rope(self, query_states, key_states, value_states, layer_idx, position_ids, rotary_emb,
                        mrope_section=None, shift_ids_in_place=True, query_out=None):
        """The attention patch's whole prologue as ONE kernel (not in the reference: there it is the continuity shift,
        the rotary module, apply_multimodal_rotary_pos_emb and PivotKVCache.update, qwen2_vl.py:68-86 + :217-259).
        query_states [1, Hq, L, D], key_states / value_states [1, Hkv, L, D] are the PRE-RoPE projections of a video
        chunk.  Returns (rotated queries - written over `query_states` unless `query_out` says otherwise -, keys, values)
        with keys / values as `update` returns them, or None - nothing touched - when this call has to take the eager
        route (text segments, chunks below 512 tokens, rotary modules that must be called, worker streams,
        score_rounding="reference" combined with prologue_operands="pre_rope").
        What the deferred score passes and the re-rotation are handed is `prologue_operands`: "reference" (default) - the
        un-rotation of the rotated rows in the model dtype, the reference's own operands (longvideo_cache.py:76-78,
        :248-259), so scores / kept sets / kept keys follow the reference's bf16 run bit for bit; "pre_rope" - the
        projections themselves.
        shift_ids_in_place: the Qwen2-VL patch shifts the ids tensor it was handed (qwen2_vl.py:73; done here by the
        chunk's flush, with the last layer's rule - what the reference's layer loop leaves behind); the LLaVA patch
        shifts a private clone (llava_onevision.py:76-88), i.e. leaves the caller's tensor alone.
        query_out: where the rotated queries go (same shape and dtype, head_dim contiguous); it is the first element of
        the returned tuple.  None: the library's pick - with prologue_operands="pre_rope" a fresh tensor when the
        chunk-batched score passes can then read `query_states` where it lies (no copy of the queries is made;
        `query_states` must stay unmodified until the chunk's flush, and is kept alive by the cache), else over
        `query_states`; pass `query_states` itself to force the in-place rotation."""
        self._entry_guard("PivotKVCache.update_pre_rope")
        if not (self.kvcache_compression and self.pos_embed_reforge and self.one_call_update) or self.overlap_streams > 0 \
                or position_ids is None or not key_states.is_cuda or key_states.shape[0] != 1 \
                or (torch.is_grad_enabled() and query_states.requires_grad):
            return None
        L = key_states.shape[2]
        b = self._batch
        lp = self._prompt_rows(L)
        if b is None or b.L != L or b.prompt != lp or not b.c_capable or not self._bound_rotary(b, rotary_emb) \
                or (layer_idx >= b.slots and not b.wrap) or layer_idx >= len(self._layers) \
                or self._layers[layer_idx].c.length + L > self._layers[layer_idx].c.cap:
            # not the steady state: find / build the batch of this geometry, bind the rotary, make room
            dev = key_states.device
            rot = self._rotary(rotary_emb, dev)
            keep_len = max(1, int(self.compression_ratio * (L - lp)))
            if rot is None or L < 512 or keep_len > L or (self.score_rounding == "reference"
                                                         and self.prologue_operands != "reference"
                                                         and key_states.dtype in (torch.bfloat16, torch.float16)):
                return None   # (the reference's rounding chain scores the reference's operands)
            Hq, D = query_states.shape[1], query_states.shape[3]
            self._fp8_refuse(key_states.dtype, D, True, rot)
            b = self._get_batch(layer_idx, Hq, key_states.shape[1], L, D, keep_len, 3 if position_ids.ndim == 3 else 1,
                                key_states.dtype, dev, lp)
            if not b.c_capable:
                return None
            self._bind_rotary(b, rotary_emb, mrope_section, rot)
            b.x_like = value_states[:, :, :1]
            self.reserve(layer_idx, L, key_states)
        ck = {"position_ids": position_ids, "rotary_emb": rotary_emb, "mrope_section": mrope_section}
        if query_out is None:
            # the library's pick: a fresh tensor whenever the queries can then be scored where they lie (the chunk-batched
            # passes read q0 itself - no packed copy, a quarter of the kernel's traffic), else over `query_states`
            if self._scores_q0_in_place(b):
                query_out = torch.empty_like(query_states)
        elif query_out is not query_states and (query_out.shape != query_states.shape
                                                or query_out.dtype is not query_states.dtype
                                                or query_out.device != query_states.device or query_out.stride(-1) != 1):
            raise ValueError("query_out must match query_states in shape, dtype and device, with a contiguous head_dim")
        out = self._update_c(b, key_states, value_states, layer_idx, ck, query_states, shift_ids_in_place, query_out)
        if out is None:
            return None
        return (query_states if query_out is None else query_out), out[0], out[1]

    def append_pre_rope(self, query_states, key_states, value_states, layer_idx, position_ids, rotary_emb,
                        mrope_section=None, shift_ids_in_place=True):
        """The attention patch's prologue for a segment that is NOT compressed - text prefill, decode (qwen2_vl.py:68-86
        + the cache's else-branch :319-321) - as one kernel (rtk_pivotkv_append_rope): continuity shift, rotary tables,
        RoPE of q (in place) and k, append of the rotated k and of v, the shifted ids appended to the layer's position
        cache; the caller's ids are shifted in place afterwards when `shift_ids_in_place` (Qwen2-VL; LLaVA shifts a
        clone).  Replaces ~25 eager launches per layer and token.  Returns (rotated q, keys, values) like `update`, or
        None - nothing touched - when the op-by-op route has to run (compression on: `update_pre_rope`; no reforging;
        rotary modules that must be called; CPU tensors)."""
        self._entry_guard("PivotKVCache.append_pre_rope")
        if self.kvcache_compression or not (self.pos_embed_reforge and self.one_call_update) or position_ids is None \
                or not key_states.is_cuda or key_states.shape[0] != 1 \
                or (torch.is_grad_enabled() and query_states.requires_grad):
            return None
        dev = key_states.device
        rot = self._rotary(rotary_emb, dev)
        if rot is None:
            return None
        q, k, v, pos = query_states, key_states, value_states, position_ids
        n, D = k.shape[2], k.shape[3]
        dt = k.dtype
        P = 3 if pos.ndim == 3 else 1
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if q.ndim != 4 or q.shape[0] != 1 or q.shape[2] != n or q.shape[3] != D or v.shape != k.shape \
                or q.dtype is not dt or v.dtype is not dt or dt not in (torch.float32, torch.bfloat16, torch.float16) \
                or pos.dtype is not torch.int64 or not pos.is_cuda or pos.shape[-1] != n or pos.shape[0] != P \
                or pos.stride(-1) != 1 or (pos.ndim == 3 and pos.shape[1] != 1) or pos.ndim not in (2, 3) \
                or q.get_device() != idx or v.get_device() != idx or pos.get_device() != idx or nv.current_device() != idx:
            return None
        qs, ks, vs = q.stride(), k.stride(), v.stride()
        if qs[3] != 1 or ks[3] != 1 or vs[3] != 1:
            return None
        # M-RoPE ids of a decode step are one row seen three times (`.expand(3, -1, -1)`, qwen2_vl.py:589: stride 0); the
        # kernel then moves t, h and w together, like the reference's in-place shift of the shared storage.  Rows that
        # overlap only partly are not served.
        if P == 3 and 0 < pos.stride(0) < n:
            return None
        st = self._store(layer_idx)
        if st.pending:
            self._flush()
        st = self.reserve(layer_idx, n, k)
        self._pos_reserve(st, P, pos.ndim, n, dev)
        if st.c.pos_len != st.base + st.c.length + st.len8:   # a cache whose earlier rows carry no ids (filled without reforging): not ours
            return None
        io = self._aio
        _fill_io(io, q, qs, k, ks, v, vs, pos)
        io.q_rot, io.qr_stride_h, io.qr_stride_l, io.flags = io.q, qs[1], qs[2], 0
        nsec = len(mrope_section) if mrope_section else 0
        sec = (C.c_int * nsec)(*mrope_section) if nsec else None
        rc = nv.lib.rtk_pivotkv_append_rope(st.cref, C.addressof(io), q.shape[1], k.shape[1], n, D, nv.dtype_code(k), P,
                                            rot.inv.data_ptr(), rot.scaling, sec, nsec, nv.round_mode(dt),
                                            int(bool(shift_ids_in_place)), nv.raw_stream(idx))
        if rc == nv.RTK_EUNSUPPORTED:
            return None
        nv.check(rc, "rtk_pivotkv_append_rope")
        self._pos_layers = max(self._pos_layers, layer_idx + 1)
        if self._watch is not None:
            _focus.capture(self, layer_idx, q)
        m = st.c.length
        return q, st._k.narrow(2, 0, m), st._v.narrow(2, 0, m)

    def _warn_compression(self):
        """The reference's logger.warning_once (:232): a log line on stderr, once per process."""
        self._warned = True
        _warn_once("Enable PivotKVCache compression: length after compression %.2f" % (self.compression_ratio))

    def _bound_rotary(self, b: _Batch, rotary_emb_fn) -> bool:
        """Is `rotary_emb_fn` the batch's bound rotary module, natively served and unchanged since its snapshot?"""
        hit = self._rotaries.get(id(rotary_emb_fn))
        return hit is not None and hit[0] is rotary_emb_fn and hit[1] is not None and hit[1] is b.rot \
            and hit[2] == _inv_stamp(rotary_emb_fn)

    def _bind_rotary(self, b: _Batch, rotary_emb_fn, mrope_section, rot: Optional[_Rotary]):
        """The rotary module / M-RoPE sections the batch's pending units were (and its next units will be) rotated
        with; units of different rotaries never share a flush."""
        same_fn = (b.rotary_emb_fn is rotary_emb_fn and b.rot is rot) or (rot is not None and b.rot is rot)
        if b.pending and (not same_fn or b.mrope_section != mrope_section):
            self._flush()
        b.rotary_emb_fn, b.rot = rotary_emb_fn, rot
        if b.mrope_section != mrope_section or b.c.inv_freq != (rot.inv.data_ptr() if rot is not None else None):
            b.mrope_section = list(mrope_section) if mrope_section is not None else None
            c = b.c
            c.nsec = len(mrope_section) if mrope_section else 0
            if c.nsec > 8:
                raise ValueError("mrope_section has more than 8 entries")
            for i in range(c.nsec):
                c.sections[i] = int(mrope_section[i])
            b.sec = (C.c_int * c.nsec)(*b.mrope_section) if c.nsec else None
            c.inv_freq = rot.inv.data_ptr() if rot is not None else None
            c.attention_scaling = rot.scaling if rot is not None else 1.0

    # ---- `update` stage by stage, what the one-call route does not serve: functions of _update_stages, bound as methods
    _update_general, _bind_update, _ids_2d, _run_stages = _us._update_general, _us._bind_update, _us._ids_2d, _us._run_stages
    _run_on_worker, _next_side, _score_ws_pointer = _us._run_on_worker, _us._next_side, _us._score_ws_pointer
    _score_stage, _append_tail, _fused_prepare = _us._score_stage, _us._append_tail, _us._fused_prepare
    _stage_pre, _stage_passes, _stage_post = _us._stage_pre, _us._stage_passes, _us._stage_post


def _option_of(config, key: str, allowed):
    """longvideo_kwargs[key] (a top-level key, default None) if it is one of `allowed`, else ValueError."""
    kind = config.longvideo_kwargs.get(key, None)
    if kind not in allowed:
        raise ValueError(f"{key} must be {' or '.join(map(repr, allowed))}, got {kind!r}")
    return kind


def build_kvcache(config, reserve_tokens: Optional[int] = None, reserve_archive_tokens: Optional[int] = None):
    """DynamicCache unless longvideo_kwargs enables 'pivotkv' compression (reference :326-334).  reserve_tokens /
    reserve_archive_tokens: optional capacity hints for the pre-allocated PivotKV cache (see PivotKVCache.__init__)."""
    if getattr(config, "longvideo_kwargs", None) is None or not config.longvideo_kwargs.get("kvcache_compression", False):
        return DynamicCache()
    compression_method = config.longvideo_kwargs["kvcache_compression_kwargs"]["compression_method"]
    if compression_method.lower() == "pivotkv":
        cache = PivotKVCache(config, reserve_tokens=reserve_tokens, reserve_archive_tokens=reserve_archive_tokens)
        cache.attention_kernel = _option_of(config, "attention_kernel", ATTENTION_KERNELS)
        cache.kv_cache_dtype = _option_of(config, "kv_cache_dtype", KV_CACHE_DTYPES)
        cache.decode_attention = _option_of(config, "decode_attention", (None, "packed"))
        if cache.decode_attention is not None and cache.attention_kernel != "hip":
            raise ValueError("decode_attention='packed' needs attention_kernel='hip': it is a kernel of the native attention")
        cache.multi_token_attention = _option_of(config, "multi_token_attention", (None, "packed"))
        if cache.multi_token_attention is not None and cache.decode_attention != "packed":
            raise ValueError("multi_token_attention='packed' needs decode_attention='packed' (and through it "
                             "attention_kernel='hip'): it widens that kernel's envelope")
        if cache.kv_cache_dtype is not None:
            if cache.attention_kernel != "hip":
                raise ValueError("kv_cache_dtype='fp8_e4m3' needs attention_kernel='hip': the third-party attention routes "
                                 "cannot read the fp8 rows")
            if cache.defer_rerotation:
                raise ValueError("kv_cache_dtype='fp8_e4m3' does not serve defer_rerotation (the sharded prefill)")
        _video_bound.configure_position_limit(cache, config)
        W = _video_bound.configure(cache, config, "window", "a prompt-guided cache belongs to one question, a window to a "
                                   "stream that does not end")
        B = _video_bound.configure(cache, config, "budget", "its scores answer one question and are not comparable between "
                                   "chunks, a budget ranks the rows of a stream that does not end",
                                   clash=None if W is None else "video_window_rows: a layer's video region is bounded by score "
                                   "or by age, not both")
        if B is not None:
            cache.score_when_keeping_all = True   # no region row without a score
        _video_bound.configure_rescore(cache, config)
        if cache.prompt_guided_scoring:   # what the mode does not serve: refused here, never a silent fallback
            for key, value, served in (("score_rounding", cache.score_rounding, "fp32"),
                                       ("kv_cache_dtype", cache.kv_cache_dtype, None),
                                       ("defer_rerotation", cache.defer_rerotation, False),
                                       ("overlap_streams", cache.overlap_streams, 0),
                                       ("flush_every_layers", cache.flush_every_layers, 0),
                                       ("native_rope", cache.native_rope, True)):
                if value != served:
                    raise ValueError(f"prompt_guided_scoring=True does not serve {key}={value!r} (only {key}={served!r}): "
                                     "the prompt-guided scores are defined for the default fp32 score arithmetic, 16-bit cache "
                                     "rows, one flush per chunk on the caller's stream and the native RoPE")
        return cache
    raise NotImplementedError

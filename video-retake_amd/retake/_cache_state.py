"""Host-side state of a PivotKVCache, mirroring the library's argument blocks (include/retake_hip.h): what a layer owns
(`_LayerStore`: the buffers the reference keeps as lists, its longvideo_cache.py:141-143), what a slot of the per-chunk
batch owns (`_Batch`: operands, scores and selection of one deferred eviction, :248-295), one stage-by-stage update, a
rotary module's snapshot, a worker stream, the `key_cache` / `value_cache` list views and the restore points (CacheMark)."""
from __future__ import annotations

import collections
import ctypes as C
import weakref
from typing import Dict, List, Optional

import torch

from . import _native as nv


def _c_field(name: str) -> property:
    """A _LayerStore property that only forwards to field `name` of the layer's rtk_layer_state block `c`."""
    return property(lambda self: getattr(self.c, name), lambda self, n: setattr(self.c, name, n))


class _LayerStore:
    """One layer's pre-allocated K/V buffers [1, Hkv, cap, D] and position ids [P, cap].  The numbers live in a
    rtk_layer_state block (`c`) the library reads and advances itself (rtk_pivotkv_update / rtk_pivotkv_flush)."""

    __slots__ = ("c", "cref", "_k", "_v", "_pos", "pending_event", "pos_ndim", "k8", "v8", "ks8", "vs8", "len8", "archive_at",
                 "sk", "sv", "base", "pinned", "sc", "sc_len", "sc_seen", "oq", "oq_rows", "oq_new")

    def __init__(self):
        self.c = nv.LayerState()
        self.cref = C.addressof(self.c)
        self._k = self._v = self._pos = None
        self.pending_event = None  # worker-stream completion of this layer's scoring (overlap_streams > 0)
        self.pos_ndim = 0          # 3: ids are [3, 1, n] (M-RoPE), 2: [1, n]
        # kv_cache_dtype="fp8_e4m3": the archive of the kept video rows - e4m3 codes uint8 [1, Hkv, cap8, D], one fp32
        # scale per (kv head, row) [1, Hkv, cap8], rows in use, and the 16-bit `length` at the first archive write
        self.k8 = self.v8 = self.ks8 = self.vs8 = None
        self.len8 = 0
        self.archive_at = -1
        # a branch (PivotKVCache.fork): views of the parent's 16-bit rows [0, base), which precede this layer's own rows
        # in the sequence (k / v / length then describe the own rows alone; the ids in `pos` cover the whole sequence)
        self.sk = self.sv = None
        self.base = 0
        # video_window_rows: the 16-bit rows the layer held before its first compressed chunk arrived (the system prompt, the
        # attention sink) - a slide never drops or moves them; -1 until that chunk (with fp8 rows the archive IS the video
        # region and `archive_at` is this number)
        self.pinned = -1
        # video_budget_rows: one fp32 score per row of the video region, in region order (row i of the region is row
        # pinned + i of the 16-bit buffers, or row i of the archive) - the value the selection saw for the row - and how
        # many leading region rows carry one.  None unless a budget is on
        self.sc = None
        self.sc_len = 0
        # video_budget_rescore: how many leading region rows existed at the last re-scoring (the OLD rows of the next one:
        # it becomes the region's rows after a re-scoring and the budget after an eviction; a rewind caps it at the restored
        # sc_len), and the last `oq_rows` rotated query rows of the layer's newest chunk [Hq, W, D] in the model dtype
        # (`oq_new`: captured since the last re-scoring).  No buffer unless the key is on
        self.sc_seen = 0
        self.oq = None
        self.oq_rows = 0
        self.oq_new = False

    def _sync(self):
        k, v, c = self._k, self._v, self.c
        c.k = k.data_ptr() if k is not None else None
        c.v = v.data_ptr() if v is not None else None
        # the library may only use the buffers when both are dense [1, Hkv, cap, D] blocks of one capacity
        ok = (k is not None and v is not None and k.ndim == 4 and k.shape == v.shape and k.is_contiguous()
              and v.is_contiguous())
        c.cap = k.shape[2] if ok else 0

    @property
    def k(self):
        return self._k

    @k.setter
    def k(self, t):
        self._k = t
        self._sync()

    @property
    def v(self):
        return self._v

    @v.setter
    def v(self, t):
        self._v = t
        self._sync()

    @property
    def pos(self):           # int64 [P, cap]: position ids of the cached tokens (pos_embed_reforge)
        return self._pos

    @pos.setter
    def pos(self, t):
        self._pos = t
        self.c.pos = t.data_ptr() if t is not None else None
        self.c.pos_cap = t.shape[1] if t is not None else 0

    length = _c_field("length")              # committed tokens
    pending = _c_field("pending")            # uncompressed chunk tokens sitting at [length, length + pending)
    pending_keep = _c_field("pending_keep")
    pos_len = _c_field("pos_len")


class _Side:
    """A worker stream with its own scratch buffers (overlap_streams > 0)."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.ws: Dict[str, torch.Tensor] = {}


class _Update:
    """One stage-by-stage update (PivotKVCache._update_general), handed from stage to stage: the batch, the layer with
    its slot and store, the operands, the chunk's tail in the layer's buffers, and what the stages make."""

    __slots__ = ("b", "layer", "slot", "st",
                 "q", "k", "v", "ids", "mask", "a_scale", "k_tail", "v_tail",
                 "pos_in", "cos", "sin")   # ids as [P, L]; cos / sin tables of the chunk's ids


class _Rotary:
    """What the kernels need of an inv_freq * position rotary module (native RoPE): its inv_freq on the device and
    attention_scaling.  HF builds one rotary module per attention layer; modules with equal contents share an entry."""

    __slots__ = ("inv", "scaling", "device")

    def __init__(self, inv, scaling, device):
        self.inv, self.scaling, self.device = inv, scaling, device


def _version_of(t: torch.Tensor):
    """The tensor's version counter, None for tensors that do not keep one (created under torch.inference_mode()): for
    those a shift the previous layer's launch has already applied is simply applied again (it is idempotent)."""
    return None if t.is_inference() else t._version


def _on_device(index: int, fn, *args):
    """fn(*args) with device `index` current: entered through torch.cuda.device only when it is not already (the usual
    case on the per-layer paths, where the context manager would cost more than the call)."""
    if nv.current_device() == index:
        return fn(*args)
    with torch.cuda.device(index):
        return fn(*args)


def _inv_stamp(rotary_emb_fn):
    """Identity + write counter of a rotary module's inv_freq: the native-RoPE snapshot of the module (_Rotary) is only
    valid while this is unchanged (a module whose inv_freq is re-assigned or modified in place is snapshotted again)."""
    inv = getattr(rotary_emb_fn, "inv_freq", None)
    return (inv.data_ptr(), _version_of(inv)) if isinstance(inv, torch.Tensor) else None


class _Batch:
    """Per-chunk batch of pending evictions: slot = layer index.  All units share the chunk geometry."""

    def __init__(self, key, slots, Hq, Hkv, L, D, keep, P, reforge, dtype, device, refround=False, fast=False,
                 keep_all=False, skip_masked=True, in_place_compaction=True, prompt=0):
        self.key, self.slots, self.keep, self.P, self.reforge = key, slots, keep, P, reforge
        # prompt-guided scoring: the chunk's last `prompt` rows are the appended prompt; they score the Lv video keys, the
        # selection runs over those Lv columns and no prompt row is cached (0: an ordinary chunk)
        self.prompt, self.Lv = int(prompt), L - int(prompt)
        self.wrap = False          # flush_every_layers: slot = layer % slots (else slot == layer)
        self.keep_all = keep_all   # keep == L and no scoring asked for: the selection is the identity
        # dtype code of the scoring entry points: bf16 payloads with the reference's bf16 rounding chain, or through the
        # fp16 matrix instruction with pre-scaled queries (score_rounding="fast"), on request
        self.score_dt = ((nv.RTK_BF16_REFROUND if refround else (nv.RTK_BF16_FAST if fast else nv.RTK_BF16))
                         if dtype == torch.bfloat16 else
                         ((nv.RTK_F16_REFROUND if refround else nv.RTK_F16) if dtype == torch.float16 else nv.RTK_F32))
        self.fast = self.score_dt == nv.RTK_BF16_FAST
        self.batched_passes = dtype in (torch.bfloat16, torch.float16) and D == 128 and L >= 512
        if self.batched_passes:   # all layers of a chunk per launch: splits chosen for the stream length (same flag everywhere)
            self.score_dt |= nv.RTK_SCORE_MANY_UNITS
        if self.prompt:   # scored at the flush whatever the shape (rtk_pivotkv_score_prompt_batched): q~ waits in the slot's workspace
            self.batched_passes = True
        # what rtk_pivotkv_prepare is told: the payload dtype (the reference-rounding mode prepares like plain bf16)
        self.prep_dt = ((nv.RTK_BF16 if dtype == torch.bfloat16 else nv.RTK_F16) if refround else self.score_dt & 0xFF) \
            | (self.score_dt & ~0xFF)
        self.Hkv, self.L, self.D, self.dtype, self.device = Hkv, L, D, dtype, device
        self.Hq = Hq
        # constants of the geometry every launch of the batch restates: bytes per payload element, the layout of the ids
        # in the position cache ([3, 1, n] M-RoPE ids or [1, n]) and the 16-bit format intermediate results are rounded to
        # (the library's dtype code is c.dtype below)
        self.esize = 4 if dtype == torch.float32 else 2
        self.pos_ndim = 3 if P == 3 else 2
        self.round_mode = nv.round_mode(dtype)
        self.defer_select = L >= 512 or bool(self.prompt)   # the chip-wide selection kernels; smaller chunks select inside update
        self.keep_idx = torch.arange(keep, dtype=torch.int64, device=device).repeat(slots, 1) if keep_all \
            else torch.empty((slots, keep), dtype=torch.int64, device=device)
        self.pos_new = torch.empty((P, slots, keep), dtype=torch.int64, device=device) if P else None
        # deferred selection (flushed for all layers at once): per-slot column partials of the scoring passes, the
        # final score, a private copy of the chunk's position ids (the caller shifts its tensor in place for the next
        # layer), the key-patch mask of the update and the selection scratch
        self.rs_n = C.c_int(0)
        self.part_floats = nv.lib.rtk_pivotkv_score_partials(Hq, Hkv, L, D, self.score_dt, C.byref(self.rs_n))
        self.pos_old = torch.empty((slots, P, L), dtype=torch.int64, device=device) if P else None
        self.sel_bytes = nv.lib.rtk_pivotkv_select_workspace_bytes(L)
        self.masks: Dict[int, Optional[torch.Tensor]] = {}
        self.selected = set()      # layers whose selection already ran inside update (small chunks)
        self.scored = set()        # layers whose matrix passes already ran inside update
        # one score workspace per slot (q~, lse partials): the matrix passes of all layers run in one launch each
        self.ws_bytes = nv.lib.rtk_pivotkv_score_workspace_bytes(Hq, Hkv, L, D, self.score_dt)
        self.ws_stride = (self.ws_bytes + 255) & ~255
        self.partials = self.score = self.sel_ws = self.score_ws = self.key_index = None
        # prompt-guided units: per-slot scratch of the thin score kernels and the video rows' ids as dense [P, Lv] blocks
        self.prompt_bytes = nv.lib.rtk_pivotkv_score_prompt_workspace_bytes(Hq, Hkv, L, self.prompt, D, self.score_dt) \
            if self.prompt else 0
        self.prompt_ws = self.pos_video = None
        self.prompt_ws_base = 0
        self.score_ws_base = 0
        self.v_stage = None
        if reforge:  # kept K is re-rotated from the un-rotated copy straight into the cache: no K staging
            self.k_unrot = torch.empty((slots, Hkv, L, D), dtype=dtype, device=device)
            self.k_stage = None
        else:
            self.k_unrot = None
            self.k_stage = None if (keep_all or in_place_compaction) else torch.empty((slots, Hkv, keep, D), dtype=dtype, device=device)
        self.cos_new = self.sin_new = None   # tables of a third-party rotary module, allocated when one is used
        self.pending: List[int] = []
        self.c_pending = 0         # how many of them were appended by rtk_pivotkv_update (the one-call path)
        self.rotary_emb_fn = None
        self.rot: Optional[_Rotary] = None
        self.mrope_section = None
        self.sec = None            # ... as the ctypes array the launches take (written by PivotKVCache._bind_rotary)
        self.x_like = None
        self.mask_obj = None       # the last key-patch mask tensor that passed validation, and its address
        self.mask_ptr = None
        self.shift_ids = None      # pre-RoPE units: the caller's ids tensor, shifted in place by the flush
        self.defer = False         # deferred re-rotation (PivotKVCache.defer_rerotation)
        self.qshape, self.kshape = torch.Size((1, Hq, L, D)), torch.Size((1, Hkv, L, D))
        self.dev_index = device.index if device.index is not None else torch.cuda.current_device()
        # the one-call path (rtk_pivotkv_update / rtk_pivotkv_flush): argument blocks bound once per batch
        self.c = nv.PivotKVBatch()
        self.cref = C.addressof(self.c)
        self.io = nv.UpdateIO()
        self.ioref = C.addressof(self.io)
        # RTK_UPDATE_SHIFT_NEXT's words (launch count + arrival counters of the prepare launch), zeroed once
        self.shift_ticket = torch.zeros(max(1, nv.lib.rtk_pivotkv_shift_ticket_ints(L, D)), dtype=torch.int32, device=device)
        self.io.ticket, self.io.ticket_ints = self.shift_ticket.data_ptr(), self.shift_ticket.numel()
        # ... and a word of PINNED HOST memory the watching workgroup increments if its bounded wait ever runs out (it then
        # shifts nothing): the host reads it without a device synchronisation (PivotKVCache._shift_latch_check raises)
        self.shift_status = torch.zeros(1, dtype=torch.int32, pin_memory=True) if device.type == "cuda" else None
        self.shift_latch = self.shift_status.numpy() if self.shift_status is not None else None
        self.io.status = self.shift_status.data_ptr() if self.shift_status is not None else None
        self.shift_stream = None   # the stream of the batch's last RTK_UPDATE_SHIFT_NEXT launch (the words serve one stream at a time)
        # prologue route: queries that are scored where they lie (no packed copy) - the pointers the library reads at
        # the flush, and the tensors themselves, kept alive until then
        self.q_units = (C.c_void_p * slots)()
        self.q_keep: List[Optional[torch.Tensor]] = [None] * slots
        c = self.c
        c.Hq, c.Hkv, c.L, c.D, c.keep, c.P, c.slots = Hq, Hkv, L, D, keep, P, slots
        c.dtype = nv.RTK_BF16 if dtype == torch.bfloat16 else (nv.RTK_F16 if dtype == torch.float16 else nv.RTK_F32)
        c.score_dtype, c.prep_dtype = self.score_dt, self.prep_dt
        c.reforge, c.keep_all, c.round_mode = int(reforge), int(keep_all), self.round_mode
        c.rs_n, c.skip_masked, c.batched_passes = self.rs_n.value, int(skip_masked), int(self.batched_passes)
        c.partial_floats = self.part_floats
        c.keep_idx = self.keep_idx.data_ptr()
        c.pos_new = self.pos_new.data_ptr() if P else None
        c.pos_old = self.pos_old.data_ptr() if P else None
        c.k_unrot = self.k_unrot.data_ptr() if reforge else None
        c.k_stage = self.k_stage.data_ptr() if self.k_stage is not None else None
        c.q_units = C.addressof(self.q_units)
        # the one-call path serves the deferred chip-wide selection (L >= 512) of reforging caches with position ids
        self.c_capable = bool(reforge and P and L >= 512)
        # rtk_pivotkv_flush compacts the tails in place in one launch (rtk_pivotkv_compact_batched): tickets and flags
        # of its workgroups live here, zeroed once; the staging rows are then only allocated by the stage-by-stage route
        self.compact_sync = None
        self.sync_stream = None    # the stream the batch's last in-place compaction was launched on
        if in_place_compaction and not keep_all:
            n_ints = nv.lib.rtk_pivotkv_compact_sync_ints(slots, Hkv, keep, D, c.dtype)
            if n_ints:
                self.compact_sync = torch.zeros(n_ints, dtype=torch.int32, device=device)
                c.compact_sync, c.compact_sync_ints = self.compact_sync.data_ptr(), n_ints
        if not keep_all:
            self.ensure_scoring()
            if self.compact_sync is None:
                self.ensure_staging()
        else:  # nothing is scored or staged: the scratch is allocated only if a route that needs it comes along
            self._dummy = torch.empty(512, dtype=torch.uint8, device=device)
            c.score_ws = (self._dummy.data_ptr() + 255) & ~255
            c.score_ws_stride, c.score_ws_bytes = 0, 0

    def slot(self, layer_idx: int) -> int:
        return layer_idx % self.slots if self.wrap else layer_idx

    def ensure_scoring(self):
        """Scoring scratch of every slot (q~ / lse workspace, column partials, scores, selection scratch, live-key
        lists); keep-all batches get it only on the routes that still un-rotate the queries."""
        if self.partials is not None:
            return
        slots, L, device, c = self.slots, self.L, self.device, self.c
        self.partials = torch.empty((slots, self.part_floats), dtype=torch.float32, device=device)
        self.score = torch.empty((slots, L), dtype=torch.float32, device=device)
        self.sel_ws = torch.empty((slots, self.sel_bytes), dtype=torch.uint8, device=device)
        self.score_ws = torch.empty(slots * self.ws_stride + 256, dtype=torch.uint8, device=device)
        self.score_ws_base = (self.score_ws.data_ptr() + 255) & ~255
        # pass 2's live-key lists (the unmasked tokens of every slot + their count): the columns the mask override
        # discards (reference :272-274) are not computed
        self.key_index = torch.empty((slots, L + 1), dtype=torch.int32, device=device)
        c.partials, c.score, c.sel_ws = self.partials.data_ptr(), self.score.data_ptr(), self.sel_ws.data_ptr()
        c.sel_ws_stride = self.sel_bytes
        c.score_ws, c.score_ws_stride, c.score_ws_bytes = self.score_ws_base, self.ws_stride, self.ws_bytes
        c.key_index = self.key_index.data_ptr()
        if self.prompt:
            self.prompt_ws = torch.empty(slots * self.prompt_bytes + 256, dtype=torch.uint8, device=device)
            self.prompt_ws_base = (self.prompt_ws.data_ptr() + 255) & ~255
            self.pos_video = torch.empty((slots, self.P, self.Lv), dtype=torch.int64, device=device) if self.P else None

    def ensure_staging(self):
        if self.v_stage is None:
            self.v_stage = torch.empty((self.slots, self.Hkv, self.keep, self.D), dtype=self.dtype, device=self.device)
            self.c.v_stage = self.v_stage.data_ptr()
            if not self.reforge and self.k_stage is None:
                self.k_stage = torch.empty_like(self.v_stage)
                self.c.k_stage = self.k_stage.data_ptr()

    def ensure_tables(self):
        if self.cos_new is None:
            self.cos_new = torch.empty((self.slots * self.keep, self.D), dtype=torch.float32, device=self.device)
            self.sin_new = torch.empty((self.slots * self.keep, self.D), dtype=torch.float32, device=self.device)


class _CacheView:
    """List-like view handed out as `key_cache` / `value_cache`: indexing flushes pending compaction
    first, so readers always see the compacted cache exactly like the reference's lists."""

    def __init__(self, owner: "PivotKVCache", which: str):
        # a weak reference: the cache owns its views, not the other way round - with a strong one the pair is a reference
        # cycle and a dropped cache (gigabytes of device memory) lives on until the garbage collector happens to run
        self._ref, self._w = weakref.ref(owner), which

    @property
    def _o(self) -> "PivotKVCache":
        o = self._ref()
        if o is None:
            raise ReferenceError("the PivotKVCache this view belongs to has been released")
        return o

    def __len__(self):
        return len(self._o._layers)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        st = self._o._layers[i]
        if st.k is None:
            return []
        if st.pending:
            self._o._flush()
        if st.len8 or st.base:
            return self._o._dense(st, self._w)
        buf = st.k if self._w == "k" else st.v
        return buf[:, :, :st.length]

    def __setitem__(self, i, value):
        # external writers (e.g. HF crop / reorder utilities) replace a layer wholesale
        self._o._adopt(i, self._w, value)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def append(self, value):
        self._o._layers.append(_LayerStore())
        if not (isinstance(value, list) and len(value) == 0):
            self._o._adopt(len(self._o._layers) - 1, self._w, value)


# one layer's numbers at a mark.  has_kv / has_pos: did the layer own K / V and id buffers (a skipped layer owns none)
# sc_len: the scored rows of the video region (video_budget_rows; 0 without a budget); sc_seen: how many of them the last
# re-scoring had seen (video_budget_rescore) - recorded, but a rewind caps the LIVE count at sc_len instead of restoring this
# one: a re-scoring above the mark has happened, the blended scores stay, and so does the fact that those rows were observed
_LayerMark = collections.namedtuple("_LayerMark",
                                    "length pos_len pos_ndim len8 archive_at num_evicted has_kv has_pos sc_len sc_seen",
                                    defaults=(0, 0))


class CacheMark:
    """A restore point of one PivotKVCache (`PivotKVCache.mark`): the host-side numbers that say which rows of the layers'
    buffers are in use - no tensor of the cache, no copy of a row.  `PivotKVCache.rewind` puts them back; the rows below a
    mark are never rewritten by later work (a compressed chunk compacts inside its own tail, text and decode rows append
    at `length`, the fp8 archive appends at `len8`), so that restores the cache.  Immutable.

      serial, epoch   the cache's mark counter / buffer epoch when the mark was taken (rewind checks both)
      layers          per layer, skipped ones included: (length, pos_len, pos_ndim, len8, archive_at, num_evicted, ..)
      n_layers, pos_layers, n_evicted   len(cache._layers), len(position_cache), len(num_evicted_tokens)
      seen_tokens     the base class's `_seen_tokens`, None when the installed base class keeps none
      resume_position_ids   CPU int64 [P], None unless the prefill glue set it: the ids a fresh prefill gave the first text
                      row after the video (`_prefill.followup_position_ids` continues from them)"""

    __slots__ = ("_ref", "serial", "epoch", "layers", "n_layers", "pos_layers", "n_evicted", "seen_tokens", "flushes",
                 "compressed", "video_end", "resume_position_ids", "__weakref__")

    def __init__(self, ref, serial, epoch, layers, n_layers, pos_layers, n_evicted, seen_tokens, flushes, compressed,
                 video_end, resume_position_ids=None):
        for name, value in (("_ref", ref), ("serial", serial), ("epoch", epoch), ("layers", layers),
                            ("n_layers", n_layers), ("pos_layers", pos_layers), ("n_evicted", n_evicted),
                            ("seen_tokens", seen_tokens), ("flushes", flushes), ("compressed", compressed),
                            ("video_end", video_end), ("resume_position_ids", resume_position_ids)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError(f"CacheMark is immutable (cannot set {name!r})")

    def __delattr__(self, name):
        raise AttributeError(f"CacheMark is immutable (cannot delete {name!r})")

    @property
    def cache(self):
        """The cache the mark belongs to, None once it has been released."""
        return self._ref()

    def _with_resume(self, ids):
        """The same restore point (same serial) carrying `ids` as resume_position_ids."""
        return CacheMark(self._ref, self.serial, self.epoch, self.layers, self.n_layers, self.pos_layers, self.n_evicted,
                         self.seen_tokens, self.flushes, self.compressed, self.video_end, ids)

    def __repr__(self):
        return (f"CacheMark(serial={self.serial}, epoch={self.epoch}, layers={self.n_layers}, "
                f"rows={[m.length + m.len8 for m in self.layers]})")

"""The deferred eviction of a chunk, once per chunk for all pending layers (reference longvideo_cache.py:260-318):
rtk_pivotkv_flush in one call for the units of the one-call update, else the same chain stage by stage - score passes,
selection, the scan into the cache or the fp8 archive.  The functions take the cache (longvideo_cache binds them as methods)."""
import ctypes as C

import torch

from . import _native as nv
from ._cache_state import _Batch, _on_device


def _flush(cache):
    """Evict every pending (layer, chunk) unit (reference :260-318 for all layers of the chunk): the score passes,
    the selection, one batched gather / re-rotate launch and one batched placement launch."""
    cache._shift_latch_check()
    b = cache._batch
    if b is None or not b.pending:
        return
    if cache.kv_cache_dtype is None and b.c_pending == len(b.pending) and not b.prompt and cache._flush_c(b):
        return
    cache._flush_general(b)

def _flush_c(cache, b: _Batch) -> bool:
    """rtk_pivotkv_flush: the whole chain in one call (units appended by rtk_pivotkv_update only)."""
    layers = b.pending
    if any(layers[i] >= layers[i + 1] for i in range(len(layers) - 1)):
        layers = sorted(set(layers))
    L_ = cache._layers
    n = len(layers)
    if b.reforge and b.P:
        for l in layers:
            st = L_[l]
            if st.c.pos_len + b.keep > st.c.pos_cap:
                cache._pos_reserve(st, b.P, b.pos_ndim, b.keep, b.device)
            elif st.pos_ndim == 0:
                st.pos_ndim = b.pos_ndim
    states = (C.c_void_p * n)(*[L_[l].cref for l in layers])
    slots = (C.c_int32 * n)(*[b.slot(l) for l in layers])
    idx = b.dev_index
    cache._order_compaction(b)
    rc = _on_device(idx, nv.lib.rtk_pivotkv_flush, b.cref, states, slots, n, nv.raw_stream(idx))
    if rc == nv.RTK_EUNSUPPORTED:
        return False
    if rc:
        cache._reset_compaction(b)
    nv.check(rc, "rtk_pivotkv_flush")
    cache._keep_scores(b, layers)
    cache._end_flush(b, layers)
    return True

def _flush_general(cache, b: _Batch):
    """The same chain launched stage by stage (reference :260-318, top to bottom): worker streams, small chunks
    (selection inside update), rotary modules that have to be called for the new ids' tables, the fp8 archive."""
    # taken off the batch first: the id shift below finds the last layer's chunk pending and re-enters _flush
    layers, b.pending = b.pending, []
    # slot of a layer: the layer itself, or (flush_every_layers) layer mod slots - within one flush slots ascend with the
    # layers, so the offset is one number (the score runs and the range of the new-id tables rely on it)
    assert all(b.slot(l) - l == b.slot(layers[0]) - layers[0] for l in layers)
    fp8 = cache.kv_cache_dtype is not None
    with torch.cuda.device(b.device):
        cache._wait_workers(layers)
        cache._shift_pending_ids(b, layers[-1])
        cache._score_unscored(b, layers)
        cache._select_unselected(b, layers)
        # reforge: K is re-rotated at the NEW ids (reference :297-306).  With the native RoPE the scan's kernel
        # computes their cos/sin itself; a third-party rotary module is called once for every pending slot and its
        # section-merged fp32 tables are handed over.
        rot = cache._rotary(b.rotary_emb_fn, b.device) if (b.reforge and b.P and not b.defer) else None
        if b.reforge and rot is None and not b.defer and not fp8:
            cache._new_id_tables(b, layers)
        if fp8:   # the kept rows go to the archive (keep-all chunks included), the 16-bit tail is left to the next chunk
            cache._archive(b, layers, rot)
        elif b.compact_sync is not None and not b.keep_all and (rot is not None or b.defer or not b.reforge):
            cache._compact(b, layers, rot)
        else:
            cache._evict_staged(b, layers, rot)
    # rtk_pivotkv_flush does exactly this itself for its units (finish_layers in pivotkv_update.hip)
    cache._advance_layers(b, layers, fp8)
    cache._keep_scores(b, layers)
    cache._end_flush(b, layers)

def _wait_workers(cache, layers):
    """The current stream waits for the layers whose chunk was scored on a worker stream (overlap_streams > 0)."""
    main = torch.cuda.current_stream()
    for l in layers:
        st = cache._layers[l]
        if st.pending_event is not None:
            main.wait_event(st.pending_event)
            st.pending_event = None

def _shift_pending_ids(cache, b: _Batch, last_layer: int):
    """Pre-RoPE units: the caller's ids tensor takes the last layer's continuity shift now (qwen2_vl.py:73; what the
    reference's layer loop leaves behind) - before the flush appends that layer's new ids."""
    if b.shift_ids is not None:
        ids, b.shift_ids = b.shift_ids, None
        b.c.shift_row = None
        cache._shift_row(ids, last_layer)

def _score_unscored(cache, b: _Batch, layers):
    """The two matrix passes (reference :260-268) of the units `update` left unscored: every run of consecutive
    slots whose queries live alike in one launch per kernel.  (Keep-all units are never scored: `update` marks them.)"""
    unscored = sorted(l for l in layers if l not in b.scored)
    if not unscored:
        return
    off = b.slot(layers[0]) - layers[0]   # (one number: see _flush_general)

    def qkey(l):   # queries scored where they lie (prologue route) carry their strides; packed ones None
        t = b.q_keep[l + off]
        return None if t is None else t.stride()

    D, Hkv = b.D, b.Hkv
    i = 0
    while i < len(unscored):
        j = i
        while j + 1 < len(unscored) and unscored[j + 1] == unscored[j] + 1 and qkey(unscored[j + 1]) == qkey(unscored[i]):
            j += 1
        l0, n = unscored[i], j - i + 1
        mptr = [b.masks.get(l) for l in range(l0, l0 + n)]
        l0 += off     # from here on: the run's first SLOT
        km = (C.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in mptr]) \
            if cache.skip_masked_columns and any(m is not None for m in mptr) else None
        qk = [b.q_keep[l] for l in range(l0, l0 + n)]
        qu, qsh, qsl = None, 0, 0
        if qk[0] is not None:   # units of the prologue route whose queries are scored in place
            qu = (C.c_void_p * n)(*[t.data_ptr() for t in qk])
            qsh, qsl = qk[0].stride(1), qk[0].stride(2)
        if b.prompt:   # prompt-guided units: the prompt's rows score the video keys, final scores, no partials
            cache._score_prompt_run(b, l0, n, qk, qsh, qsl)
            i = j + 1
            continue
        nv.check(nv.lib.rtk_pivotkv_score_passes_batched_q(
            C.c_void_p(b.score_ws_base + l0 * b.ws_stride), b.ws_stride,
            nv.ptr(b.k_unrot[l0]) if b.reforge else None, b.L * D * Hkv * b.esize,
            nv.ptr(b.partials[l0]), b.part_floats, n, b.Hq, Hkv, b.L, D, b.score_dt,
            km, nv.ptr(b.key_index[l0]) if km is not None else None, qu, qsh, qsl, nv.stream()),
            "rtk_pivotkv_score_passes_batched")
        i = j + 1

def _score_prompt_run(cache, b: _Batch, l0: int, n: int, qk, qsh: int, qsl: int):
    """rtk_pivotkv_score_prompt_batched for the n consecutive slots from l0 (up to 28 units per call): rows [Lv, L) of
    the slots' q~ (packed, or qk's tensors where they lie) against rows [0, Lv) of their k~ -> b.score[slot, :Lv]."""
    D, Hkv = b.D, b.Hkv
    for u0 in range(0, n, nv.PROMPT_SCORE_MAX_UNITS):
        m, s0 = min(nv.PROMPT_SCORE_MAX_UNITS, n - u0), l0 + u0
        qu = (C.c_void_p * m)(*[t.data_ptr() for t in qk[u0:u0 + m]]) if qk[0] is not None else None
        nv.check(nv.lib.rtk_pivotkv_score_prompt_batched(
            C.c_void_p(b.score_ws_base + s0 * b.ws_stride), b.ws_stride,
            nv.ptr(b.k_unrot[s0]) if b.reforge else None, b.L * D * Hkv * b.esize,
            nv.ptr(b.score[s0]), b.L, C.c_void_p(b.prompt_ws_base + s0 * b.prompt_bytes), b.prompt_bytes, m,
            b.Hq, Hkv, b.L, b.prompt, D, b.score_dt, qu, qsh, qsl, nv.stream()), "rtk_pivotkv_score_prompt_batched")

def _select_units(cache, b: _Batch, todo, partials, ids):
    """rtk_select_unit blocks of the layers `todo`; `partials` (None: the scores are final) and `ids` are indexed by slot."""
    su = (nv.SelectUnit * len(todo))()
    for u, l in zip(su, todo):
        sl = b.slot(l)
        u.partial = partials[sl].data_ptr() if partials is not None else None
        u.score = b.score[sl].data_ptr()
        m = b.masks.get(l)
        u.mask = m.data_ptr() if m is not None else None
        u.pos = ids[sl].data_ptr() if b.P else None
        u.keep_idx = b.keep_idx[sl].data_ptr()
        u.rank = None
        u.pos_out = (b.pos_new.data_ptr() + sl * b.keep * 8) if b.P else None
        u.workspace = b.sel_ws[sl].data_ptr()
    return su

def _select_prompt_units(cache, b: _Batch, todo):
    """The selection of prompt-guided units: mask override + top-k + id gather / rescale over the Lv VIDEO columns
    (the existing kernels called with L = Lv: keep of Lv, temporal ids rescaled by keep / Lv).  Their ids are handed
    over as dense [P, Lv] blocks; a key-patch mask is read up to Lv."""
    P, keep, Lv = b.P, b.keep, b.Lv
    slots = [b.slot(l) for l in todo]
    if P:
        lo, hi = min(slots), max(slots) + 1
        b.pos_video[lo:hi].copy_(b.pos_old[lo:hi, :, :Lv])
    su = cache._select_units(b, todo, None, b.pos_video)   # (no partials: the scores are final)
    rc = nv.lib.rtk_pivotkv_select_batched(su, len(todo), 0, 0, 0, Lv, keep, P, int(b.reforge), b.slots * keep, b.score_dt,
                                           nv.stream())
    if rc != nv.RTK_EUNSUPPORTED:
        nv.check(rc, "rtk_pivotkv_select_batched")
        return
    # few video rows (a video's tail chunk): outside the chip-wide kernels, one workgroup per unit
    rank = cache._buf("rank", (Lv,), torch.int32, b.device)
    for u in su:
        nv.check(nv.lib.rtk_pivotkv_select(u.score, u.mask, Lv, keep, u.pos, P, int(b.reforge), u.keep_idx, nv.ptr(rank),
                                           u.pos_out, b.slots * keep, u.workspace, b.sel_bytes, nv.stream()),
                 "rtk_pivotkv_select")

def _select_unselected(cache, b: _Batch, layers):
    """Mask override + top-k + id gather / rescale (reference :269-295) of the units not selected inside `update`,
    in one launch.  Keep-all batches: the selection is the identity (keep_idx is set once per batch) and the units
    of the one-call path carry their ids in pos_old only: ids x 1.0 = the ids (:288-292)."""
    todo = [l for l in layers if l not in b.selected]
    if not todo:
        return
    P, keep = b.P, b.keep
    if b.keep_all:
        if P:
            for l in todo:
                b.pos_new[:, b.slot(l)].copy_(b.pos_old[b.slot(l)])
        return
    if b.prompt:
        return cache._select_prompt_units(b, todo)
    su = cache._select_units(b, todo, b.partials, b.pos_old)
    nv.check(nv.lib.rtk_pivotkv_select_batched(su, len(todo), b.Hkv, b.rs_n.value, b.Hq // b.Hkv, b.L, keep, P,
                                               int(b.reforge), b.slots * keep, b.score_dt, nv.stream()),
             "rtk_pivotkv_select_batched")

def _new_id_tables(cache, b: _Batch, layers):
    """Section-merged fp32 cos / sin tables of the NEW ids of every pending slot, from a rotary module that has
    to be called (reference :298), for the staged scan."""
    b.ensure_tables()
    keep, P = b.keep, b.P
    lo, hi = b.slot(min(layers)), b.slot(max(layers))
    n = (hi - lo + 1) * keep
    pos2d = b.pos_new[:, lo:hi + 1].reshape(P, n)   # a copy when the slot range is partial
    cache._rope_tables(b.cos_new[lo * keep:], b.sin_new[lo * keep:], b.rotary_emb_fn, b.x_like, pos2d, n, b.pos_ndim,
                      b.sec, n, b.D)

def _scan_unit(cache, b: _Batch, l: int, u):
    """What the three scans share of layer l's unit.  Fills the fields every unit type names alike - the K source
    (the slot's un-rotated rows with reforge, else the tail), keep_idx, and the position-id bookkeeping (reference
    :308-309; the layer's id buffer is grown first) - and returns (layer store, slot, K tail, V tail, their head
    stride in elements); the tail is where the append put the chunk: rows [length, length + L) of the buffers."""
    st, sl = cache._layers[l], b.slot(l)
    keep, D = b.keep, b.D
    tail, stride_h = st.length * D * b.esize, st.k.shape[2] * D
    k_tail, v_tail = st.k.data_ptr() + tail, st.v.data_ptr() + tail
    if b.reforge:
        u.k_src, u.k_src_stride_h = b.k_unrot[sl].data_ptr(), b.L * D
    else:
        u.k_src, u.k_src_stride_h = k_tail, stride_h
    u.keep_idx = b.keep_idx[sl].data_ptr()
    if b.reforge and b.P:
        cache._pos_reserve(st, b.P, b.pos_ndim, keep, b.device)
        u.pos_src, u.pos_src_stride = b.pos_new.data_ptr() + sl * keep * 8, b.slots * keep
        u.pos_dst, u.pos_dst_stride = st.pos.data_ptr() + st.pos_len * 8, st.pos.shape[1]
    else:
        u.pos_src = u.pos_dst = None
    return st, sl, k_tail, v_tail, stride_h

def _evict_staged(cache, b: _Batch, layers, rot):
    """The eviction scan of the pending layers as two launches (reference :278-318): the evict launch
    (rtk_pivotkv_evict_batched[_rope]) gathers the kept rows - K re-rotated at the new ids straight into the cache with reforge, else K and V into
    the staging rows - and rtk_pivotkv_place_batched puts the staged rows at the head of the tail."""
    keep, D, Hkv, es, dt = b.keep, b.D, b.Hkv, b.esize, b.c.dtype
    tables = b.reforge and rot is None and not b.defer   # of a called rotary module (_new_id_tables)
    if not b.keep_all:
        b.ensure_staging()
    units = (nv.EvictUnit * len(layers))()
    places = (nv.PlaceUnit * (0 if b.keep_all else len(layers) * (1 if b.reforge else 2)))()
    nc = 0
    for u, l in zip(units, layers):
        st, sl, k_tail, v_tail, stride_h = cache._scan_unit(b, l, u)
        staged = []   # (staging rows, tail) of this unit: K unless it goes straight into the cache, V
        if b.reforge:
            if tables:
                u.cos_new = b.cos_new.data_ptr() + sl * keep * D * 4
                u.sin_new = b.sin_new.data_ptr() + sl * keep * D * 4
            u.k_dst, u.k_dst_stride_h = k_tail, stride_h  # straight into the cache
        elif not b.keep_all:
            u.k_dst, u.k_dst_stride_h = b.k_stage[sl].data_ptr(), keep * D
            staged.append((u.k_dst, k_tail))
        u.v_src, u.v_src_stride_h = v_tail, stride_h
        if not b.keep_all:   # (keep-all: every row already sits where the append put it)
            u.v_dst, u.v_dst_stride_h = b.v_stage[sl].data_ptr(), keep * D
            staged.append((u.v_dst, v_tail))
        for stage, tail in staged:
            p = places[nc]
            p.stage, p.stage_stride_h_bytes = stage, keep * D * es
            p.tail, p.tail_stride_h_bytes = tail, stride_h * es
            p.keep_idx = u.keep_idx
            nc += 1
    s = nv.stream()
    if rot is not None:
        nv.check(nv.lib.rtk_pivotkv_evict_batched_rope(units, len(layers), Hkv, D, keep, b.P, dt, nv.ptr(rot.inv),
                                                       rot.scaling, b.sec, b.c.nsec, b.round_mode, 1, s),
                 "rtk_pivotkv_evict_batched_rope")
    elif b.reforge or not b.keep_all:   # (deferred re-rotation: every kept un-rotated K row is copied, bit 1)
        nv.check(nv.lib.rtk_pivotkv_evict_batched(units, len(layers), Hkv, D, keep, b.P if b.reforge else 0, dt,
                                                  3 if b.defer else 1, s), "rtk_pivotkv_evict_batched")
    # kept rows -> head of the tail: in place, except the ~ratio of them whose source lies inside the destination
    # range (parked in the staging rows by the launch above) - reference :313-318 without a full second copy
    if nc:
        nv.check(nv.lib.rtk_pivotkv_place_batched(places, nc, Hkv, keep, D, dt, s), "rtk_pivotkv_place_batched")

def _advance_layers(cache, b: _Batch, layers, fp8: bool):
    """The layers' numbers after a stage-by-stage flush: the kept rows are committed (to the archive with fp8 rows),
    nothing is pending."""
    keep, ids = b.keep, b.reforge and b.P
    for l in layers:
        st = cache._layers[l]
        b.q_units[b.slot(l)] = None
        if fp8:
            st.len8 += keep
        else:
            st.length += keep
        st.pending = 0
        st.pending_keep = 0
        st.c.mask = None
        if ids:
            st.pos_len += keep

def _end_flush(cache, b: _Batch, layers):
    """The batch's own bookkeeping of a completed flush, whichever route ran it: nothing is pending, what `update`
    noted per unit (masks, scored / selected marks, the ids tensor to shift, queries kept alive) is dropped, and
    the position cache covers the flushed layers (reference :308-309)."""
    b.pending = []
    b.c_pending = 0
    cache._flushes += 1
    b.masks.clear()
    b.scored.clear()
    b.selected.clear()
    b.shift_ids = None
    for l in layers:
        b.q_keep[b.slot(l)] = None
    if b.reforge and b.P:
        cache._pos_layers = max(cache._pos_layers, max(layers) + 1)

def _order_compaction(cache, b: _Batch):
    """The in-place compaction's tickets and flags (batch.compact_sync) serve ONE launch at a time: flushes of a batch
    are ordered on one stream.  A flush that arrives on another stream than the batch's previous one first waits for
    the device (rare: the caller changed its current stream between two chunks)."""
    if b.compact_sync is None:
        return
    cur = nv.raw_stream(b.dev_index)
    if b.sync_stream is not None and b.sync_stream != cur:
        torch.cuda.synchronize(b.device)
    b.sync_stream = cur

def _reset_compaction(cache, b: _Batch):
    """After a failed flush: tickets / flags back to zero (a launch that completes leaves them zeroed itself)."""
    if b.compact_sync is not None:
        try:
            b.compact_sync.zero_()
        except Exception:  # noqa: BLE001  (a device-side abort leaves the context unusable; the first error is what is raised)
            pass

def _archive(cache, b: _Batch, layers, rot):
    """The eviction scan of the pending layers into their fp8 archives, one launch (rtk_pivotkv_archive_batched;
    reference :278-310): kept K re-rotated at the new ids and rounded to the model dtype as the compaction does (taken
    from the tail as it is without reforge), kept V from the tail, both quantised per (kv head, row) into rows
    [len8, len8 + keep) of the archive; ids to the position cache.  The 16-bit length does not advance."""
    keep, D, Hkv = b.keep, b.D, b.Hkv
    if b.reforge and (rot is None or not b.P or b.defer):
        raise NotImplementedError("kv_cache_dtype='fp8_e4m3' with pos_embed_reforge needs position ids and the native RoPE, "
                                  "and no deferred re-rotation")
    units = (nv.ArchiveUnit * len(layers))()
    for u, l in zip(units, layers):
        st = cache._layers[l]
        cache._archive_reserve(st, keep, Hkv, D, b.device)
        if st.archive_at < 0:
            st.archive_at = st.length
        _, _, _, v_tail, stride_h = cache._scan_unit(b, l, u)
        u.v_src, u.v_src_stride_h = v_tail, stride_h
        if b.keep_all:
            u.keep_idx = None
        cap8 = st.k8.shape[2]
        u.k8, u.v8, u.dst_stride_h = st.k8.data_ptr() + st.len8 * D, st.v8.data_ptr() + st.len8 * D, cap8 * D
        u.k_scale, u.v_scale, u.scale_stride_h = st.ks8.data_ptr() + st.len8 * 4, st.vs8.data_ptr() + st.len8 * 4, cap8
    mode = nv.COMPACT_K_ROTATE if b.reforge else nv.COMPACT_K_COPY
    sec = b.sec if b.reforge else None
    nv.check(nv.lib.rtk_pivotkv_archive_batched(
        units, len(layers), Hkv, D, keep, b.P if b.reforge else 0, b.c.dtype, mode,
        nv.ptr(rot.inv) if b.reforge else None, rot.scaling if b.reforge else 1.0,
        sec, len(sec) if sec is not None else 0, b.round_mode, nv.stream()),
        "rtk_pivotkv_archive_batched")

def _compact(cache, b: _Batch, layers, rot):
    """The eviction scan of the pending layers as one in-place launch (rtk_pivotkv_compact_batched; reference
    :278-318): kept K re-rotated at the new ids (or copied un-rotated when the rotation is deferred; compacted in
    place without reforge), V compacted inside the tail, ids to the position cache."""
    units = (nv.CompactUnit * len(layers))()
    for u, l in zip(units, layers):
        _, _, k_tail, v_tail, stride_h = cache._scan_unit(b, l, u)
        u.k_tail, u.k_tail_stride_h = k_tail, stride_h
        u.v_tail, u.v_tail_stride_h = v_tail, stride_h
        if not b.reforge:   # K is compacted inside its tail like V: no separate source
            u.k_src, u.k_src_stride_h = None, 0
    mode = nv.COMPACT_K_INPLACE if not b.reforge else (nv.COMPACT_K_COPY if b.defer else nv.COMPACT_K_ROTATE)
    rotate = mode == nv.COMPACT_K_ROTATE
    sec = b.sec if rotate else None
    cache._order_compaction(b)
    nv.check(nv.lib.rtk_pivotkv_compact_batched(
        units, len(layers), b.Hkv, b.D, b.keep, b.P if b.reforge else 0, b.c.dtype, mode,
        nv.ptr(rot.inv) if rotate else None, rot.scaling if rotate else 1.0,
        sec, len(sec) if sec is not None else 0, b.round_mode, b.c.compact_sync, b.c.compact_sync_ints,
        nv.stream()),
        "rtk_pivotkv_compact_batched")

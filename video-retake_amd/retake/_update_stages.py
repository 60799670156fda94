"""`PivotKVCache.update` stage by stage (rtk_pivotkv_prepare / _append / _score_stages_masked / _select): what the one-call
route does not serve - the first update of a geometry, text / decode appends, small chunks, fp32 passes, rotary modules that
must be called, worker streams.  The functions take the cache (longvideo_cache binds them as methods)."""
import ctypes as C
from typing import Optional

import torch

from . import _focus, _native as nv, _video_bound
from ._cache_state import _Side, _Update


def _update_general(cache, key_states, value_states, layer_idx, cache_kwargs=None):
    """`update` stage by stage (inputs and outputs: see its docstring)."""
    if not cache._warned:
        cache._warn_compression()
    cache_kwargs = cache_kwargs if cache_kwargs is not None else {}
    position_ids = cache_kwargs.pop("position_ids", None)
    cache_kwargs.pop("shift_next_position_ids", None)   # (the build's own key: only the one-call route acts on it)
    nv.require_device(key_states, value_states)
    assert key_states.shape[0] == 1, "PivotKVCache supports bsz == 1 only"

    # 1) append: the next layer's hidden states see the uncompressed chunk (reference :238)
    n_new = key_states.shape[2]
    if len(cache._layers) > layer_idx and cache._layers[layer_idx].pending:
        cache._flush()

    if not cache.kvcache_compression:  # text prefill / decode (reference :319-321)
        st = cache.reserve(layer_idx, n_new, key_states)
        P0 = st.length
        st.k[:, :, P0:P0 + n_new].copy_(key_states)
        st.v[:, :, P0:P0 + n_new].copy_(value_states)
        st.length += n_new
        if cache.pos_embed_reforge:
            cache.update_position_ids(position_ids, layer_idx)
        if cache._watch is not None and cache_kwargs.get("query_states") is not None:
            _focus.capture(cache, layer_idx, cache_kwargs["query_states"])
        return st.k[:, :, :st.length], st.v[:, :, :st.length]

    u = cache._bind_update(key_states, value_states, layer_idx, cache_kwargs, position_ids)
    b, st, dev = u.b, u.st, key_states.device
    with torch.cuda.device(dev):
        side = cache._next_side(dev)
        if side is None:
            u.pos_in = cache._ids_2d(u, False)
            prepared = cache._fused_prepare(u, cache._ws)
            if not prepared:
                cache._append_tail(u)
            cache._run_stages(u, cache._ws, prepared)
        else:
            cache._append_tail(u)   # on the caller's stream: all this layer's attention needs
            u.pos_in = cache._ids_2d(u, True)
            cache._run_on_worker(u, side)
    if cache.video_budget_rescore is not None:
        _video_bound.observe(cache, st, u.q)
    cache.update_num_evicted_tokens(n_new - b.keep, layer_idx)  # reference :310
    st.pending = n_new
    st.pending_keep = b.keep
    b.pending.append(layer_idx)
    cache._compressed_in_forward = True
    cache._last_slot = (b, u.slot)
    return st.k[:, :, :st.length + n_new], st.v[:, :, :st.length + n_new]

def _bind_update(cache, key_states, value_states, layer_idx, cache_kwargs, position_ids) -> _Update:
    """The argument handling of a compressed `_update_general` call: pops the rest of the cache_kwargs protocol
    (reference :235, :241-243), checks the operands, finds / builds the batch of the chunk's geometry, binds the
    rotary, claims the layer's slot and makes room for the chunk."""
    query_states = cache_kwargs.pop("query_states")
    rotary_emb_fn = cache_kwargs.pop("rotary_emb")
    mrope_section = cache_kwargs.pop("mrope_section", None)  # M-RoPE only
    bsz, Hq, L, D = query_states.shape
    Hkv = key_states.shape[1]
    assert bsz == 1
    nv.require_device(query_states)
    dev = key_states.device
    nv.dtype_code(key_states)   # (raises for a dtype the kernels do not serve)
    for t in (query_states, key_states, value_states):
        if t.stride(-1) != 1:
            raise ValueError("q/k/v must be contiguous along head_dim")
    lp = cache._prompt_rows(L)   # prompt-guided unit: the last lp rows are the appended prompt, keep counts video rows
    keep_len = max(1, int(cache.compression_ratio * (L - lp)))  # evict new tokens only (reference :263)
    if keep_len > L - lp:   # compression_ratio > 1: the reference's topk refuses it (:276)
        raise RuntimeError(f"PivotKVCache.update: selected index k out of range (keep {keep_len} of {L} tokens)")
    reforge = bool(cache.pos_embed_reforge)
    rot = cache._rotary(rotary_emb_fn, dev) if reforge else None
    if lp and reforge and rot is None:
        raise ValueError("prompt_guided_scoring with pos_embed_reforge needs a rotary module of the static inv_freq * "
                         "position kind and native_rope=True: a rotary module that has to be called is not served")
    cache._fp8_refuse(key_states.dtype, D, reforge, rot, position_ids is not None)

    mask = cache.keypatches_mask_chunk
    if mask is not None:
        nv.require_device(mask)
        if mask.dtype != torch.bool or not mask.is_contiguous():
            mask = mask.to(torch.bool).contiguous()
        assert mask.numel() in (L, L - lp), "keypatches_mask_chunk must have one entry per chunk token"
    Pn = 0
    if position_ids is not None:
        nv.require_device(position_ids)
        Pn = 3 if position_ids.ndim == 3 else 1
    b = cache._get_batch(layer_idx, Hq, Hkv, L, D, keep_len, Pn, key_states.dtype, dev, lp)
    cache._bind_rotary(b, rotary_emb_fn, mrope_section, rot)
    if b.pending and b.c.pre_rope:   # units of the prologue route are flushed among themselves
        cache._flush()
    b.c.pre_rope = 0
    u = _Update()
    u.b, u.layer, u.slot = b, layer_idx, cache._claim_slot(b, layer_idx)
    u.q, u.k, u.v, u.ids, u.mask = query_states, key_states, value_states, position_ids, mask
    b.x_like = value_states[:, :, :1]
    u.st = st = cache.reserve(layer_idx, key_states.shape[2], key_states)
    if st.pinned < 0:    # the layer's first compressed chunk: what it holds now is pinned (video_window_rows)
        st.pinned = st.length
    tail = st.length * D * st.k.element_size()
    u.k_tail, u.v_tail = C.c_void_p(st.k.data_ptr() + tail), C.c_void_p(st.v.data_ptr() + tail)
    u.a_scale = float(getattr(rotary_emb_fn, "attention_scaling", 1.0)) if reforge else 1.0
    u.pos_in = u.cos = u.sin = None
    return u

def _ids_2d(cache, u: _Update, snapshot: bool):
    if u.ids is None:
        return None
    p2 = u.ids.reshape(u.b.P, u.b.L)
    # worker streams read the ids later than the caller's stream runs on: the attention patch shifts the
    # SAME ids tensor in place for the next layer (qwen2_vl.py:73), so they get a private copy
    return p2.clone() if snapshot else (p2 if p2.is_contiguous() else p2.contiguous())

def _run_stages(cache, u: _Update, ws, prepared: bool):
    """The launch stages of one update on the CURRENT stream: un-rotate / pack (unless the fused prepare launch has
    done it), the chunk's ids into the slot, the matrix passes, the selection."""
    if not prepared:
        cache._stage_pre(u, ws)
        if u.b.defer_select and u.pos_in is not None:
            u.b.pos_old[u.slot].copy_(u.pos_in)
    cache._stage_passes(u, ws)
    cache._stage_post(u, ws)

def _run_on_worker(cache, u: _Update, side: _Side):
    """`_run_stages` on a worker stream (overlap_streams > 0): it starts after what the caller's stream has queued
    so far, and the layer's flush waits for its completion event."""
    main = torch.cuda.current_stream()
    ready = torch.cuda.Event()
    ready.record(main)
    for t in (u.q, u.k, u.v, u.pos_in, u.mask):
        if t is not None:
            t.record_stream(side.stream)
    with torch.cuda.stream(side.stream):
        side.stream.wait_event(ready)
        cache._run_stages(u, side.ws, False)
        done = torch.cuda.Event()
        done.record(side.stream)
    u.st.pending_event = done

def _score_ws_pointer(cache, u: _Update, ws):
    b = u.b
    if b.batched_passes:   # the slot's own workspace: q~ must survive until the batched passes of the flush
        return b.score_ws_base + u.slot * b.ws_stride
    wsb = cache._buf("score_ws", (b.ws_bytes + 256,), torch.uint8, b.device, ws)
    return (wsb.data_ptr() + 255) & ~255

def _score_stage(cache, u: _Update, ws, stages):
    b, q, k = u.b, u.q, u.k
    score = b.score[u.slot]
    k_unrot = b.k_unrot[u.slot] if b.reforge else None
    # the matrix passes of a per-update launch know the chunk's key-patch mask: pass 2 skips the columns the
    # selection overwrites with 1.0 anyway (reference :272-274)
    live = u.mask if (stages & nv.SCORE_PASSES) and cache.skip_masked_columns else None
    kidx = cache._buf("key_index", (b.L + 1,), torch.int32, b.device, ws) if live is not None else None
    nv.check(nv.lib.rtk_pivotkv_score_stages_masked(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), k.stride(1), k.stride(2),
        b.Hq, b.Hkv, b.L, b.D, b.score_dt, nv.ptr(u.cos), nv.ptr(u.sin), u.a_scale,
        nv.ptr(score), nv.ptr(k_unrot), C.c_void_p(cache._score_ws_pointer(u, ws)), b.ws_bytes, stages,
        nv.ptr(b.partials[u.slot]), nv.ptr(live), nv.ptr(kidx), nv.stream()), "rtk_pivotkv_score")
    return score

def _stage_pre(cache, u: _Update, ws):
    """RoPE tables of the chunk's ids + un-rotate / pack (reference :248-259), on the CURRENT stream."""
    b = u.b
    b.ensure_scoring()
    if b.reforge:
        L, D = b.L, b.D
        u.cos = cache._buf("old_cos", (L, D), torch.float32, b.device, ws)
        u.sin = cache._buf("old_sin", (L, D), torch.float32, b.device, ws)
        cache._rope_tables(u.cos, u.sin, b.rotary_emb_fn, u.v, u.pos_in, L, u.ids.ndim, b.sec, L, D)
    cache._score_stage(u, ws, nv.SCORE_PREPARE)

def _stage_passes(cache, u: _Update, ws):
    """the two matrix passes (reference :260-268): deferred to the flush (all layers of the chunk in one
    launch per kernel) whenever the batched form supports the shape"""
    b = u.b
    if b.keep_all:         # nothing to choose: no scores
        b.scored.add(u.layer)
        return
    if b.batched_passes:
        return
    cache._score_stage(u, ws, nv.SCORE_PASSES)
    b.scored.add(u.layer)

def _stage_post(cache, u: _Update, ws):
    """small chunks only: column-mass reduction, mask override + top-k + position ids (reference :269-295)
    right away; larger chunks leave this to the batched selection of the flush"""
    b, slot, pos_in = u.b, u.slot, u.pos_in
    if b.keep_all:         # keep_idx is the identity (set once per batch); ids x 1.0 = the ids (:288-292)
        if pos_in is not None:
            b.pos_new[:, slot].copy_(pos_in)
        b.selected.add(u.layer)
        return
    if b.defer_select:
        b.masks[u.layer] = u.mask
        return
    score = cache._score_stage(u, ws, nv.SCORE_FINALIZE)
    L, dev = b.L, b.device
    rank = cache._buf("rank", (L,), torch.int32, dev, ws)
    pos_out = b.pos_new[:, slot] if pos_in is not None else None
    sel_ws = cache._buf("select_ws", (b.sel_bytes,), torch.uint8, dev, ws)
    nv.check(nv.lib.rtk_pivotkv_select(nv.ptr(score), nv.ptr(u.mask), L, b.keep, nv.ptr(pos_in), b.P,
                                       int(b.reforge), nv.ptr(b.keep_idx[slot]), nv.ptr(rank), nv.ptr(pos_out),
                                       b.slots * b.keep, nv.ptr(sel_ws), b.sel_bytes, nv.stream()),
             "rtk_pivotkv_select")
    b.selected.add(u.layer)

def _append_tail(cache, u: _Update):
    """reference :238 - the uncompressed view this layer's attention reads"""
    b, k, v = u.b, u.k, u.v
    nv.check(nv.lib.rtk_pivotkv_append(
        nv.ptr(k), k.stride(1), k.stride(2), nv.ptr(v), v.stride(1), v.stride(2), b.Hkv, b.L, b.D, b.c.dtype,
        u.k_tail, u.v_tail, u.st.k.shape[2] * b.D, nv.stream()), "rtk_pivotkv_append")

def _fused_prepare(cache, u: _Update, ws) -> bool:
    """append + native RoPE tables + un-rotate in ONE launch (k read once); False if the shape needs the
    separate kernels."""
    b, q, k, v, pos_in = u.b, u.q, u.k, u.v, u.pos_in
    if not (b.reforge and b.rot is not None and pos_in is not None):
        return False
    # keep-all chunks are not scored: no q~, no score workspace (any aligned address will do)
    k_only = b.keep_all and b.partials is None
    ws_ptr = b.c.score_ws if k_only else cache._score_ws_pointer(u, ws)
    rc = nv.lib.rtk_pivotkv_prepare(
        nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), k.stride(1), k.stride(2),
        nv.ptr(v), v.stride(1), v.stride(2),
        b.Hq, b.Hkv, b.L, b.D, b.prep_dt | (nv.RTK_PREPARE_K_ONLY if k_only else 0), nv.ptr(pos_in), b.L, b.P,
        nv.ptr(b.rot.inv), u.a_scale, b.sec, b.c.nsec, b.round_mode,
        nv.ptr(b.k_unrot[u.slot]), C.c_void_p(ws_ptr), b.ws_bytes, u.k_tail, u.v_tail, u.st.k.shape[2] * b.D,
        nv.ptr(b.pos_old[u.slot]) if b.defer_select else None, nv.stream())
    if rc == nv.RTK_EUNSUPPORTED:
        return False
    nv.check(rc, "rtk_pivotkv_prepare")
    return True

def _next_side(cache, device) -> Optional[_Side]:
    if cache.overlap_streams <= 0:
        return None
    while len(cache._sides) < cache.overlap_streams:
        cache._sides.append(_Side(device))
    side = cache._sides[cache._side_rr % len(cache._sides)]
    cache._side_rr += 1
    return side

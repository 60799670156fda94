"""Restore points of PivotKVCache and the branches forked at them (not in the reference): mark / rewind / crop move numbers
only, fork shares the parent's rows below a mark.  None of it runs during a prefill.  The functions take the cache
(longvideo_cache binds them as methods)."""
import weakref
from typing import Optional

import torch

from . import _focus
from ._cache_state import CacheMark, _LayerMark


def _take_mark(cache, compressed: bool) -> CacheMark:
    nev = cache.num_evicted_tokens
    layers = tuple(_LayerMark(st.c.length, st.c.pos_len, st.pos_ndim, st.len8, st.archive_at,
                              nev[l] if l < len(nev) else 0, st._k is not None, st._pos is not None, st.sc_len,
                              st.sc_seen)
                   for l, st in enumerate(cache._layers))
    cache._mark_serial += 1
    return CacheMark(weakref.ref(cache), cache._mark_serial, cache._epoch, layers, len(cache._layers), cache._pos_layers, len(nev),
                     getattr(cache, "_seen_tokens", None), cache._flushes, compressed,
                     None if compressed else cache.last_compressed_mark)

def mark(cache) -> CacheMark:
    """A restore point of the cache as it stands (see CacheMark).  Like reading `position_cache` it first flushes
    deferred work (the flush waits for the worker streams), so a mark taken between an `update` and `after_forward`
    equals the one taken after it.  O(layers) on the host; launches nothing besides that flush.  (A branch's marks
    count its own rows.)"""
    cache._branch_check("PivotKVCache.mark")
    if cache.defer_rerotation:
        raise NotImplementedError("PivotKVCache.mark: a cache with defer_rerotation (the sharded prefill's block caches) "
                                  "holds un-rotated keys and provisional ids until `finalize`; it has no restore points")
    cache._flush()
    return cache._take_mark(False)

def video_end(cache) -> Optional[CacheMark]:
    """`last_compressed_mark`: the restore point after the most recent forward that compressed a chunk - after a chunked
    prefill, the end of the video (None: nothing has been compressed).  The prefill glue attaches the ids of the first
    text row that followed (CacheMark.resume_position_ids)."""
    return cache.last_compressed_mark

def set_resume_position_ids(cache, position_ids: torch.Tensor):
    """The prefill glue's note on `video_end`: the ids ([3, 1] / [1], any device) the forward computed for the first text
    row after the video, before the attention patch shifted them."""
    m = cache.last_compressed_mark
    if m is not None:
        cache.last_compressed_mark = m._with_resume(position_ids.detach().reshape(-1).to("cpu", torch.int64).clone())

def _mark_is_dead(cache, serial: int) -> bool:
    return any(lo < serial <= hi for lo, hi in cache._dead_marks)

def _kill_marks_after(cache, serial: int):
    """Every mark taken after `serial` so far is invalid from now on (its rows are about to be overwritten)."""
    if serial < cache._mark_serial:   # (ranges that start at or above `serial` lie inside the new one)
        cache._dead_marks = tuple(r for r in cache._dead_marks if r[0] < serial) + ((serial, cache._mark_serial),)
    for br in cache._branches or ():   # (noted on the branches: this cache may be released before they look)
        if br.forked_from.serial > serial:
            br._fork_dead = "rows"

def _check_mark(cache, mark: CacheMark):
    if not isinstance(mark, CacheMark):
        raise ValueError(f"PivotKVCache.rewind takes a CacheMark (PivotKVCache.mark), got {type(mark).__name__}")
    if mark.cache is not cache:
        raise ValueError("PivotKVCache.rewind: the mark belongs to another cache")
    if cache._mark_is_dead(mark.serial):
        raise ValueError("PivotKVCache.rewind: the mark has been invalidated - the cache was rewound or cropped to an "
                         "earlier point since, and the rows the mark names have been given up")
    if mark.epoch != cache._epoch:
        raise ValueError("PivotKVCache.rewind: buffers of the cache were replaced or rewritten wholesale after the mark was "
                         "taken (key_cache / value_cache / position_cache assigned, or stored rows rotated in place)")
    nev = cache.num_evicted_tokens
    if len(cache._layers) < mark.n_layers or cache._pos_layers < mark.pos_layers or len(nev) < mark.n_evicted:
        raise ValueError("PivotKVCache.rewind: the cache holds fewer layers than the mark records")
    for l, m in enumerate(mark.layers):
        st = cache._layers[l]
        if st.c.length < m.length or st.c.pos_len < m.pos_len or st.len8 < m.len8 or (m.has_kv and st._k is None) \
                or (m.has_pos and st._pos is None) or (m.archive_at >= 0 and st.archive_at != m.archive_at):
            raise ValueError(f"PivotKVCache.rewind: layer {l} is shorter than the mark says")

def rewind(cache, mark: CacheMark) -> None:
    """Back to the state `mark` recorded: the follow-up question's way of not prefilling the video again (rewind to
    `video_end`, append the next question).  O(layers) on the host: the numbers are restored, layers / id lists /
    eviction counts that did not exist at the mark are dropped, `_prompt_len` / the pre-shift memo are cleared.  Nothing
    is launched, copied, freed or reallocated - every buffer that existed at the mark keeps its address -, and
    `kvcache_compression`, `keypatches_mask_chunk`, the batch and the scratch are left alone.  Every mark taken after
    `mark` is invalid afterwards.  ValueError, before anything changes: a mark of another cache, an invalidated one,
    one from before the buffers were replaced (the epoch), or a cache that is shorter than the mark says."""
    cache._branch_check("PivotKVCache.rewind")
    cache._flush()
    cache._shift_latch_check()
    cache._check_mark(mark)
    for st, m in zip(cache._layers, mark.layers):
        st.c.length, st.c.pos_len, st.pos_ndim, st.len8, st.archive_at = m.length, m.pos_len, m.pos_ndim, m.len8, m.archive_at
        st.sc_len = m.sc_len
        st.sc_seen = min(st.sc_seen, m.sc_len)   # (video_budget_rescore: blended scores stay - the observation happened)
        # `pinned` is not in the mark and need not be: it is set once, to the layer's length at its first compressed
        # chunk, and a slide - the only thing that moves rows - voids every earlier mark.  So a valid mark either lies at
        # or below that length (taken before any video row existed: the next compressed chunk pins afresh) or above it
        # (the pinned rows and the number are still what they were)
        if st.pinned >= m.length:
            st.pinned = -1
        if not m.has_kv and st._k is not None:    # a layer that was skipped at the mark owns nothing again
            st.k = st.v = None
        if not m.has_pos and st._pos is not None:
            st.pos = None
    del cache._layers[mark.n_layers:]
    cache._pos_layers = mark.pos_layers
    nev = cache.num_evicted_tokens
    del nev[mark.n_evicted:]
    for l in range(mark.n_evicted):
        nev[l] = mark.layers[l].num_evicted
    if mark.seen_tokens is not None:
        cache._seen_tokens = mark.seen_tokens
    cache._after_rewind(mark.serial)
    cache._flushes = mark.flushes
    cache._compressed_in_forward = False
    lcm = cache.last_compressed_mark
    if lcm is not None and lcm.serial > mark.serial:   # video_end as it was at the mark
        cache.last_compressed_mark = mark if mark.compressed else mark.video_end

def _after_rewind(cache, serial: int):
    cache._prompt_len = 0
    cache._preshifted = None
    cache._kill_marks_after(serial)

def _crop_floor(cache):
    """Rows per layer a crop may not go below: the boundary after the most recent compressed flush, as
    `last_compressed_mark` recorded it - or None when the cache holds compressed rows and no such record of them."""
    m = cache.last_compressed_mark
    if m is not None and m.epoch == cache._epoch and m.flushes == cache._flushes:
        return [m.layers[l].length + m.layers[l].len8 + cache._layers[l].base if l < m.n_layers else 0
                for l in range(len(cache._layers))]
    if cache._flushes == 0 and not any(cache.num_evicted_tokens):
        return [0] * len(cache._layers)
    return None

def crop(cache, max_length: int):
    """transformers' DynamicCache.crop on this cache: keep the first `max_length` rows of every layer (negative: drop
    that many trailing rows; at or above the current length: nothing happens).  Assisted and prompt-lookup generation
    call it to give up rejected candidate tokens.  Served down to the boundary after the most recent compressed flush
    only: below it a length alone cannot say what `num_evicted_tokens` or the archive split were - ValueError, and
    the cache stays as it was.  Like `rewind` it moves numbers only.  Every mark taken after `video_end` is invalid
    afterwards (which of them name dropped rows is not tracked)."""
    cache._branch_check("PivotKVCache.crop")
    cache._flush()
    cache._shift_latch_check()
    cur = cache.get_seq_length()
    if max_length < 0:
        max_length = cur - abs(max_length)
    if cur <= max_length:
        return
    if max_length < 0:
        raise ValueError(f"PivotKVCache.crop: cannot drop more rows than the cache holds ({cur})")
    if cache.defer_rerotation:
        raise NotImplementedError("PivotKVCache.crop: not served with defer_rerotation (see PivotKVCache.mark)")
    floor = cache._crop_floor()
    drops = []
    for l, st in enumerate(cache._layers):
        total = st.c.length + st.len8 + st.base if st._k is not None else 0
        drop = max(0, total - max_length)
        if drop and (floor is None or total - drop < floor[l]):
            raise ValueError(
                f"PivotKVCache.crop({max_length}): layer {l} would be cut inside its compressed video rows "
                f"({'no boundary is recorded' if floor is None else f'they end at row {floor[l]}'}): a length alone cannot "
                "restore num_evicted_tokens or the archive split there - rewind to a mark instead")
        if drop and st.c.pos_len not in (0, total):
            raise ValueError(f"PivotKVCache.crop: layer {l} keeps ids for {st.c.pos_len} of its {total} rows")
        drops.append(drop)
    for st, drop in zip(cache._layers, drops):
        st.c.length -= drop
        if st.c.pos_len:
            st.c.pos_len -= drop
        if cache.kv_cache_dtype is None and st.pinned >= 0:   # (video_budget_rows: scores of rows that are gone)
            st.sc_len = min(st.sc_len, max(st.c.length - st.pinned, 0))
            st.sc_seen = min(st.sc_seen, st.sc_len)
    if hasattr(cache, "_seen_tokens"):
        cache._seen_tokens = max_length
    m = cache.last_compressed_mark
    cache._after_rewind(m.serial if m is not None else 0)

def shared_len(cache, layer_idx) -> int:
    """Rows of the parent's 16-bit buffers that precede the layer's own rows: 0 unless this cache is a branch."""
    if layer_idx is None or layer_idx >= len(cache._layers):
        return 0
    return cache._layers[layer_idx].base

def shared(cache, layer_idx):
    """(ks, vs) views [1, Hkv, base, D] of the parent's rows the branch shares in this layer, or None."""
    if not cache.shared_len(layer_idx):
        return None
    st = cache._layers[layer_idx]
    return st.sk, st.sv

def _branch_check(cache, who="PivotKVCache"):
    """A branch is valid while its parent has not given up the rows they share: ValueError - what `rewind` raises for
    such a mark - once the parent was rewound or cropped below the fork point, or had its buffers rewritten wholesale.
    (A parent that was merely released is fine: the views own the storage.)"""
    m = cache.forked_from
    if m is None:
        return
    parent = m.cache
    if cache._fork_dead is None and parent is not None:
        if parent._mark_is_dead(m.serial):
            cache._fork_dead = "rows"
        elif m.epoch != parent._epoch:
            cache._fork_dead = "epoch"
    if cache._fork_dead == "rows":
        raise ValueError(f"{who}: the mark this branch was forked at has been invalidated - the parent cache was rewound "
                         "or cropped to an earlier point since, and the rows the branch shares have been given up")
    if cache._fork_dead == "epoch":
        raise ValueError(f"{who}: buffers of the parent cache were replaced or rewritten wholesale after the branch was "
                         "forked (key_cache / value_cache / position_cache assigned, or stored rows rotated in place)")

def _branch_refuse_write(cache):
    if cache.forked_from is not None:
        raise NotImplementedError("a branch (PivotKVCache.fork): key_cache / value_cache / position_cache are dense copies "
                                  "of [the parent's rows | the branch's own]; assigning through them is not supported")

def _branch_update_check(cache, who: str):
    """What every row-writing entry point of a branch checks first: the branch is still valid, and the call does not
    compress (branches carry questions, not video)."""
    cache._branch_check(who)
    if cache.kvcache_compression:
        raise NotImplementedError(f"{who}: a branch (PivotKVCache.fork) does not compress video chunks - branches carry "
                                  "questions, not video (set kvcache_compression = False, or feed the video to the parent)")

def fork(cache, mark: Optional[CacheMark] = None, reserve_tokens: Optional[int] = None) -> "PivotKVCache":
    """A BRANCH of this cache at `mark` (default: `self.mark()`, which flushes first; a given mark is checked as `rewind`
    checks it): a second live conversation about the same video for the memory of its own rows.  Per layer the branch
    holds VIEWS of this cache's 16-bit rows [0, mark.length) and archive rows [0, mark.len8) - rows below a restore
    point are never rewritten - a copy of the position ids [0, mark.pos_len) (P x 8 bytes a row: every id-reading
    kernel stays as it is) and empty K / V buffers of its own, `reserve_tokens` rows (default 1024) to begin with.
    `branch.forked_from` is the mark; get_seq_length / get_prev_temporal_idx / num_evicted_tokens / archive_len answer
    for the whole sequence, as this cache's did at the mark.

    A branch serves text and decode rows (`update` with compression off, `append_pre_rope`) into its own buffers,
    `attention` over [archive | shared | own] (rtk_attention_forward_shared / rtk_attention_decode_shared - no other
    route sees the shared rows: a call the native attention declines raises NotImplementedError), `mark` / `rewind` /
    `crop` within its own rows (the crop floor is the fork point) and `_prefill.followup_position_ids(
    branch.forked_from, n, device)` when forked at `video_end`.  It refuses, before any launch: a compressing update
    (NotImplementedError: branches carry questions, not video), assignment through key_cache / value_cache (reading
    them gives a dense copy in sequence order, a diagnostic), a fork of its own.

    The branch stays valid while this cache keeps the shared rows: rewinding it to `mark` itself, answering its own
    questions above `mark`, or releasing it altogether are all fine; rewinding or cropping it BELOW `mark` makes every
    later call on the branch raise the ValueError `rewind` raises for such a mark.  A parent that outgrows a buffer
    allocates a new one and the old one stays alive until the branches are dropped (`reserve_tokens` avoids that).

    ValueError without attention_kernel="hip"; NotImplementedError with defer_rerotation, on a float32 model, with
    head_dim != 128, or on a branch (no nested forks)."""
    _focus._refuse_focused(cache, "fork")
    if cache.attention_kernel != "hip":
        raise ValueError("PivotKVCache.fork needs attention_kernel='hip': only the native attention reads the rows a "
                         "branch shares with its parent")
    if cache.defer_rerotation:
        raise NotImplementedError("PivotKVCache.fork: not served with defer_rerotation (see PivotKVCache.mark)")
    if cache.forked_from is not None:
        raise NotImplementedError("PivotKVCache.fork: this cache is itself a branch; nested forks are not served "
                                  "(fork the parent again)")
    if cache.head_dim != 128:
        raise NotImplementedError(f"PivotKVCache.fork needs head_dim 128, got {cache.head_dim}")
    for st in cache._layers:
        if st._k is not None and st._k.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"PivotKVCache.fork needs a bfloat16 or float16 model, got {st._k.dtype}")
    if mark is None:
        mark = cache.mark()
    else:
        cache._flush()
        cache._shift_latch_check()
        cache._check_mark(mark)
    br = type(cache)(cache.config, reserve_tokens=reserve_tokens)
    br.attention_kernel, br.kv_cache_dtype, br.decode_attention = cache.attention_kernel, cache.kv_cache_dtype, cache.decode_attention
    br.multi_token_attention = cache.multi_token_attention
    br.kvcache_compression = False
    cap = br.reserve_tokens or 1024
    for l, m in enumerate(mark.layers):
        pst, st = cache._layers[l], br._store(l)
        if m.has_kv:
            k, v = pst._k, pst._v
            st.sk, st.sv, st.base = k[:, :, :m.length], v[:, :, :m.length], m.length
            shape = (1, k.shape[1], cap, k.shape[3])
            st.k = torch.empty(shape, dtype=k.dtype, device=k.device)
            st.v = torch.empty(shape, dtype=k.dtype, device=k.device)
            if m.len8:
                st.k8, st.v8, st.ks8, st.vs8 = (t[:, :, :m.len8] for t in (pst.k8, pst.v8, pst.ks8, pst.vs8))
                st.len8, st.archive_at = m.len8, m.archive_at
        if m.has_pos:
            ids = torch.empty((pst._pos.shape[0], m.pos_len + cap), dtype=torch.int64, device=pst._pos.device)
            ids[:, :m.pos_len].copy_(pst._pos[:, :m.pos_len])
            st.pos, st.pos_len, st.pos_ndim = ids, m.pos_len, m.pos_ndim
    br._pos_layers = mark.pos_layers
    br.num_evicted_tokens = [mark.layers[l].num_evicted for l in range(mark.n_evicted)]
    if mark.seen_tokens is not None:
        br._seen_tokens = mark.seen_tokens
    br._flushes = mark.flushes
    br._warned = True
    br.forked_from = mark
    # the branch's own restore point at the fork: its `video_end` and crop floor
    br.last_compressed_mark = br._take_mark(True)._with_resume(mark.resume_position_ids)
    if cache._branches is None:
        cache._branches = weakref.WeakSet()
    cache._branches.add(br)
    return br

"""The bounded video region of PivotKVCache (not in the reference): ONE mechanism, two policies.  A layer's region is
everything behind its pinned rows - the rows it held before its first compressed chunk arrived (the system prompt: the
attention sink); with fp8 rows it is the archive, whose ids begin at `archive_at`.  `video_window_rows` bounds it by age (`slide_window`: the oldest rows go), `video_budget_rows` by score (`evict_budget`: the newest row
and the best-scored others stay); build_kvcache refuses the two together.  The functions take the cache.

`after_forward` calls the policy that is on.  `_plan` walks the layers, picks those whose region holds more than rows + slack, refuses
what cannot be moved - before anything is launched or changed - and describes what moves as byte streams `(data_ptr,
stream_stride, streams, row_bytes, first)`.  The policy appends its own tail to each and launches per device on the current
stream; `_commit` keeps the books: length / len8 and pos_len shrink, num_evicted_tokens and the policy's `*_dropped` list
grow, `_seen_tokens` is left alone.  Rows below every earlier mark are rewritten, so the epoch moves: earlier marks raise
in `rewind`, live branches are dead; the `video_end` that `after_forward` takes next is valid.  No buffer is allocated or
replaced.

`video_position_limit` (this project's own rule, no reference counterpart) rides on a move: `rebase_positions` shifts the
ids of the layers just moved down to follow their pinned rows and re-rotates their keys by the same delta, decided on the
device per layer; `position_offset` is the cumulative delta.  With `video_position_gap` = G on top (again this project's
own rule, no reference counterpart, answer quality not evaluated) the delta is per ROW: inner id gaps above G close to G as
well, each key is re-rotated by its own row's delta, and `position_offset` grows by the last row's.

`video_budget_rescore` (again this project's own rule, no reference counterpart, answer quality not evaluated) acts in
front of the budget's eviction: `observe` keeps the last rotated query rows of a layer's newest chunk, `rescore_budget`
blends the stored scores of the region's old rows with what those queries see of them.
"""
import torch

from . import _native as nv
from ._cache_state import _Batch, _LayerStore, _on_device


def bound(cache):
    """(rows, slack) of the window or the budget, whichever is on; None with both off."""
    if cache.video_window_rows is not None:
        return cache.video_window_rows, cache.video_window_slack
    return None if cache.video_budget_rows is None else (cache.video_budget_rows, cache.video_budget_slack)


def configure(cache, config, word: str, prompt_guided: str, clash=None):
    """build_kvcache: longvideo_kwargs' video_<word>_rows / video_<word>_slack, validated and set on the cache -> the rows
    (None: off).  `prompt_guided`: the policy's own sentence on why it does not serve prompt_guided_scoring; `clash`: the
    option the policy does not go together with and why, if that option is on."""
    rows_key, slack_key = f"video_{word}_rows", f"video_{word}_slack"
    rows, slack = config.longvideo_kwargs.get(rows_key, None), config.longvideo_kwargs.get(slack_key, 0)
    keys = f"{rows_key} / {slack_key}"

    def is_int(x, least):
        return isinstance(x, int) and not isinstance(x, bool) and x >= least
    if not (rows is None or is_int(rows, 1)) or not is_int(slack, 0):
        raise ValueError(f"{keys}: {rows_key} must be an int > 0 (or None: no {word}) and {slack_key} "
                         f"an int >= 0, got {rows!r} and {slack!r}")
    if rows is not None:
        if clash is not None:
            raise ValueError(f"{keys} do not go together with {clash}")
        if cache.defer_rerotation:
            raise ValueError(f"{keys} do not serve defer_rerotation (the sharded prefill): its block caches hold "
                             "un-rotated keys and provisional ids until `finalize`")
        if cache.prompt_guided_scoring:
            raise ValueError(f"{keys} do not serve prompt_guided_scoring: {prompt_guided}")
        setattr(cache, rows_key, rows)
        setattr(cache, slack_key, slack)
    return rows


def configure_position_limit(cache, config):
    """build_kvcache: longvideo_kwargs' video_position_limit and video_position_gap, validated and set on the cache (None:
    off).  Every refusal names the key it clashes with; nothing else has happened yet.  The gap needs the limit, and every
    refusal of the limit holds with the gap set."""
    kw, key, gap_key = config.longvideo_kwargs, "video_position_limit", "video_position_gap"
    P, G = kw.get(key, None), kw.get(gap_key, None)
    if P is None:
        if G is not None:
            raise ValueError(f"{gap_key} needs {key}: ids are renumbered only where that limit has been reached")
        return None
    if not isinstance(P, int) or isinstance(P, bool) or P < 0:
        raise ValueError(f"{key} must be an int >= 0 (or None: the ids are never re-based), got {P!r}")
    if kw.get("video_window_rows", None) is None and kw.get("video_budget_rows", None) is None:
        raise ValueError(f"{key} needs video_window_rows or video_budget_rows: the ids are re-based only where a bounded "
                         "video region has just moved its rows")
    if not cache.pos_embed_reforge:
        raise ValueError(f"{key} needs pos_embed_reforge=True: without it the cache keeps no ids to re-base")
    if cache.kv_cache_dtype is not None:
        raise ValueError(f"{key} does not serve kv_cache_dtype={cache.kv_cache_dtype!r}: re-quantising e4m3 codes at every "
                         "re-base compounds a 2^-4 relative error per row, so it is not built")
    if not cache.native_rope:
        raise ValueError(f"{key} needs native_rope=True: the rotation by the id delta is computed on the device from the "
                         "rotary module's inv_freq, a module that has to be called cannot serve it")
    if G is not None and (not isinstance(G, int) or isinstance(G, bool) or G < 1):
        raise ValueError(f"{gap_key} must be an int >= 1 (or None: {key} re-bases a region by one delta), got {G!r}")
    cache.video_position_limit, cache.video_position_gap = P, G
    return P


def configure_rescore(cache, config):
    """build_kvcache: longvideo_kwargs' video_budget_rescore (alpha) and video_budget_observe_rows (W, read only with alpha
    set), validated and set on the cache (None: off).  Every refusal names its keys; nothing else has happened yet."""
    kw, key, rows_key = config.longvideo_kwargs, "video_budget_rescore", "video_budget_observe_rows"
    configure_archive_rescore(cache, config)
    alpha = kw.get(key, None)
    if alpha is None:
        return None
    W = kw.get(rows_key, 64)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0 < alpha <= 1:
        raise ValueError(f"{key} must be a float in (0, 1] (or None: scores stay as they arrived), got {alpha!r}")
    if not isinstance(W, int) or isinstance(W, bool) or W < 1:
        raise ValueError(f"{rows_key} must be an int >= 1 (the newest chunk's last query rows that {key} observes with), "
                         f"got {W!r}")
    if cache.video_budget_rows is None:
        raise ValueError(f"{key} needs video_budget_rows: it blends the scores the budget evicts by (video_window_rows bounds "
                         "a region by age and keeps no scores)")
    if cache.kv_cache_dtype is not None and not cache.archive_rescore:
        raise ValueError(f"{key} does not serve kv_cache_dtype={cache.kv_cache_dtype!r}: the archive's e4m3 key rows are not "
                         "scored again, it is not built - unless asked for: set archive_rescore=True")
    cache.video_budget_rescore, cache.video_budget_observe_rows = float(alpha), W
    return cache.video_budget_rescore


def configure_archive_rescore(cache, config):
    """build_kvcache: longvideo_kwargs' archive_rescore, validated and set on the cache (False: off).  True lets
    video_budget_rescore and PivotKVCache.focus score the e4m3 key rows of an fp8 archive as they lie
    (rtk_pivotkv_rescore_fp8k_batched) - scores taken on lossy keys are another rule than scores taken on 16-bit keys, hence
    a key of its own.  What kv_cache_dtype refuses (video_position_limit, prompt_guided_scoring, defer_rerotation) stays
    refused by those keys' own checks."""
    key = "archive_rescore"
    on = config.longvideo_kwargs.get(key, None)
    if on is not None and not isinstance(on, bool):
        raise ValueError(f"{key} must be True or False (or None: off), got {on!r}")
    if on and cache.kv_cache_dtype is None:
        raise ValueError(f"{key}=True needs kv_cache_dtype: it scores the e4m3 key rows of the fp8 archive, a 16-bit cache "
                         "has none (video_budget_rescore and focus serve it as it is)")
    cache.archive_rescore = bool(on)


def _rebase_rotary(cache):
    """The native-RoPE snapshot the last chunk was rotated with; ValueError - before anything is launched - for a rotary
    module that has to be called (no inv_freq, the dynamic / longrope kinds)."""
    b = cache._batch
    if b is None or b.rot is None:
        raise ValueError("video_position_limit: the rotary module of this model has to be called (it has no inv_freq, or is "
                         "of a dynamic / longrope kind), so the keys cannot be re-rotated by an id delta on the device - "
                         "build the cache without video_position_limit")
    return b


def _offsets(cache, device):
    """The device's int64 array of cumulative deltas, one slot per layer (zeros at first; it grows with the layers)."""
    n = max(int(cache.num_hidden_layers), len(cache._layers))
    t = cache._position_offsets.get(device)
    if t is None or t.numel() < n:
        new = torch.zeros(n, dtype=torch.int64, device=device)
        if t is not None:
            new[:t.numel()].copy_(t)
        cache._position_offsets[device] = t = new
    return t


def rebase_positions(cache, by_device):
    """video_position_limit (not in the reference; a rule of this project's own): for every layer the policy has just moved,
    ONE rtk_pivotkv_rebase_batched call per device - decided on the device, nothing is read back.  With t the layer's
    temporal ids, `first` its first region row and `end` its pos_len:

        base = t[first - 1] + 1 if first > 0 else 0;  delta = t[first] - base
        if delta > 0 and t[end - 1] >= video_position_limit:
            t[first:end] -= delta;  K[:, first:length, temporal channels] <- R(-delta) K;  position_offset(layer) += delta

    Called after `_commit`: the lengths are the moved region's.  Rows 1 / 2 of M-RoPE ids, the other channels, V and the
    pinned rows are not touched; 16-bit rows behind the region move with it, ids and keys alike.

    With video_position_gap = G (also this project's own rule; the reference has no counterpart and answer quality is not
    evaluated) the call is rtk_pivotkv_renumber_batched and the delta is per row - under the budget an old survivor keeps
    t[first] low, the delta above stays 0 and the holes evictions open elsewhere are never closed without it:

        e[first] = max(0, t[first] - prev - 1), prev = t[first - 1] if first > 0 else -1;  e[i] = max(0, t[i] - t[i - 1] - G)
        d[i] = e[first] + ... + e[i];  total = d[end - 1]
        if total > 0 and t[end - 1] >= video_position_limit:
            t[i] -= d[i];  K[:, i, temporal channels] <- R(-d[i]) K;  position_offset(layer) += total

    Gaps <= G stay (0 and negative ones too); a row with d = 0 keeps its bits.  The per-row deltas live in one scratch
    buffer per device, sized once for a full region, its slack and a chunk: no buffer is replaced after warm-up."""
    if cache.video_position_limit is None or not by_device:
        return
    b = _rebase_rotary(cache)
    gap = cache.video_position_gap
    for dev, layers in by_device.items():
        groups = {}
        device = layers[0][1]._k.device
        if gap is not None:
            # the per-row deltas: one row of scratch per layer, sized once - a full region with its slack and a chunk in
            # flight, or whatever lies behind the pinned rows now (16-bit rows behind a window's region) if that is more
            room = max(max(st.c.pos_len - st.pinned for _, st, *_ in layers), sum(bound(cache)) + b.L)
            row_delta = cache._buf(f"renumber_rows{dev}", (len(cache._layers), room), torch.int64, device)
        for l, st, *_ in layers:
            first = st.pinned
            if st._pos is None or st.c.pos_len <= first or first < 0:
                continue
            P, D = st._pos.shape[0], st._k.shape[3]
            u = (st._k.data_ptr(), st._k.stride(1) * st._k.element_size(), first, st.c.length - first,
                 st._pos.data_ptr(), st._pos.stride(0), st.c.pos_len, st._k.shape[1], l)
            u = nv.RebaseUnit(*u) if gap is None else nv.RenumberUnit(*u, row_delta[l].data_ptr())
            groups.setdefault((D, nv.dtype_code(st._k), P), []).append(u)
        if not groups:
            continue
        inv = b.rot.inv
        if inv.device != device:   # (layers spread over devices: a copy of the frequencies on each)
            inv = cache._buf(f"rebase_inv{dev}", inv.shape, inv.dtype, device)
            inv.copy_(b.rot.inv)
        off = _offsets(cache, device)
        for (D, dt, P), us in groups.items():
            delta = cache._buf(f"rebase_delta{dev}", (len(us),), torch.int64, device)
            nsec = b.c.nsec if P == 3 else 0
            name, unit = (("rtk_pivotkv_rebase_batched", nv.RebaseUnit) if gap is None else
                          ("rtk_pivotkv_renumber_batched", nv.RenumberUnit))
            nv.check(_on_device(dev, getattr(nv.lib, name), (unit * len(us))(*us), len(us), D, dt, P, inv.data_ptr(),
                                b.sec if nsec else None, nsec, cache.video_position_limit, *(() if gap is None else (gap,)),
                                off.data_ptr(), delta.data_ptr(), nv.raw_stream(dev)), name)


def position_offset(cache, layer_idx: int) -> torch.Tensor:
    """video_position_limit: the cumulative delta the layer's region ids have been re-based by, a 0-dim int64 tensor on the
    layer's device (a view of the array the kernel advances: read without a sync, it is as current as the stream).  A stored id
    + this = the id an unbounded cache would hold.  A zero with the key off or before any move.

    With video_position_gap it grows by the renumbering's `total`, the delta of the region's LAST id: `stored last id +
    offset = the unbounded run's last id` still holds for the newest row - later chunks continue from that row - but no
    longer for every row: an older row has been moved down by less."""
    st = cache._layers[layer_idx] if 0 <= layer_idx < len(cache._layers) else None
    device = st._k.device if st is not None and st._k is not None else None
    t = cache._position_offsets.get(device) if device is not None else None
    if t is None or layer_idx >= t.numel():
        return torch.zeros((), dtype=torch.int64, device=device)
    return t[layer_idx]


def region_room(cache, st: _LayerStore, first: int, more: int) -> int:
    """The rows at which a buffer stops growing - the pinned rows (`first`; not known yet: what the layer holds), a full
    window or budget with its slack and `more` (the in-flight chunk).  0 with both off, and 0 while `kvcache_compression` is
    off: text, question and decode rows grow a buffer as they always did (by doubling), so the plateau holds only if the
    caller's `reserve_tokens` covers them on top of pinned + rows + slack + one chunk."""
    b = bound(cache)
    return 0 if b is None or not cache.kvcache_compression else max(first, 0) + sum(b) + more


def _streams(first: int, *ts):
    """Dense tensors of ONE shape - [1, H, cap, D], [1, H, cap] or [P, cap] - as H (P) byte streams of cap rows each, from
    row `first` on.  (The shape is read once: this runs per layer on the host, in front of every move.)"""
    shape = ts[0].shape
    ax = min(len(shape), 3) - 1
    row = ts[0].element_size() * (shape[3] if len(shape) == 4 else 1)
    return [(t.data_ptr(), shape[ax] * row, shape[ax - 1], row, first) for t in ts]


def _plan(cache, key: str, cannot: str, check=lambda *layer: None):
    """{device index: [(layer, store, first, n, ids, streams)]} of the layers whose region [first, first + n) holds more than
    rows + slack rows - layers are bounded independently: each has its own count, a skipped layer none.  `streams`: the
    moving tensors, the id buffer last if the layer keeps ids (`ids`).  ValueError for a layer that cannot be moved, then
    whatever the policy's own `check` of the layer raises."""
    rows, slack = bound(cache)
    fp8 = cache.kv_cache_dtype is not None
    by_device = {}
    for l, st in enumerate(cache._layers):
        first = st.archive_at if fp8 else st.pinned
        if st._k is None or first < 0:
            continue
        n = st.len8 if fp8 else st.c.length - first
        if n <= rows + slack:
            continue
        ids = st._pos is not None and st.c.pos_len > 0
        if st.c.cap == 0 or (ids and st.c.pos_len != st.c.length + st.len8):
            raise ValueError(f"{key}: layer {l} {cannot} - its buffers are not the cache's own dense blocks, "
                             f"or it keeps ids for {st.c.pos_len} of its {st.c.length + st.len8} rows")
        check(l, st, first, n, ids)
        # K and V from `first` on; with fp8 rows the archive [0, len8): codes of D bytes a row, one fp32 scale a row
        streams = _streams(0, st.k8, st.v8) + _streams(0, st.ks8, st.vs8) if fp8 else _streams(first, st._k, st._v)
        if ids:    # in sequence order: the region's ids begin at `first`
            streams += _streams(first, st._pos)
        by_device.setdefault(st._k.get_device(), []).append((l, st, first, n, ids, streams))
    return by_device


def _commit(cache, by_device, dropped):
    """The bookkeeping once every launch is issued: each planned layer is down to the bound's rows."""
    rows, fp8 = bound(cache)[0], cache.kv_cache_dtype is not None
    dropped.extend([0] * (len(cache._layers) - len(dropped)))
    for layers in by_device.values():
        for l, st, _, n, ids, _ in layers:
            d = n - rows
            if fp8:
                st.len8 -= d
            else:
                st.c.length -= d
            if ids:
                st.c.pos_len -= d
            cache.update_num_evicted_tokens(d, l)
            dropped[l] += d
    cache._epoch += 1
    for br in cache._branches or ():   # (noted on the branches: this cache may be released before they look)
        if br._fork_dead is None:
            br._fork_dead = "epoch"


def _launch(dev: int, name: str, units, n: int):
    nv.check(_on_device(dev, getattr(nv.lib, name), units, n, nv.raw_stream(dev)), name)


def slide_window(cache):
    """Drop the oldest rows of every layer whose video region holds more than W + slack rows, down to W: K, V and the ids of
    all such layers (the archive's codes, scales and ids with fp8 rows) move down in place in ONE rtk_pivotkv_slide_batched
    call (per device; a call is one kernel launch per 96 moving tensors: 28 layers x (K, V, ids) is one, 28 x 5 archive
    tensors two).  get_prev_temporal_idx still reads the last stored id."""
    W = cache.video_window_rows
    by_device = _plan(cache, "video_window_rows", "cannot slide")
    if by_device and cache.video_position_limit is not None:
        _rebase_rotary(cache)   # (raises before the move, not between the move and the re-base)
    for dev, layers in by_device.items():
        units = []
        for _, st, first, n, ids, streams in layers:
            d = n - W
            units += [s + (d, W) for s in streams]
            if ids:    # the ids of later 16-bit rows follow the region's and move with them
                units[-1] = streams[-1] + (d, st.c.pos_len - first - d)
        _launch(dev, "rtk_pivotkv_slide_batched", (nv.SlideUnit * len(units))(*[nv.SlideUnit(*u) for u in units]), len(units))
    if by_device:
        _commit(cache, by_device, cache.window_dropped)
        rebase_positions(cache, by_device)


def evict_budget(cache):
    """Evict every layer whose video region holds n > B + slack rows down to B: the newest row (get_prev_temporal_idx reads
    its id: the ids of every later chunk stay those of an unbounded cache) and the B - 1 best-scored others survive (ties to
    the oldest), in sequence order.  A row's score is the fp32 score its chunk's selection saw for it (`keep_scores`) - a
    column sum of row-stochastic softmaxes averaged over heads, which averages 1 over any chunk whatever its length, so
    rows of different chunks compare directly.  Per device ONE rtk_pivotkv_budget_select_batched call writes
    each layer's ascending survivor list, ONE rtk_pivotkv_squeeze_batched call moves K, V, ids and scores of all such layers
    down in place (the archive's codes, scales, ids and scores with fp8 rows).  Pinned rows never move, ids are not
    rescaled again; the scored rows shrink with the region.  ValueError: a region row without a score - text or decode rows
    appended behind the video and not rewound.  (With fp8 rows such rows live in the 16-bit buffers, but their ids lie
    between the archive's: the survivors' ids are then no contiguous block, and the eviction raises all the same.  So the
    id unit covers exactly [first, first + n) = [first, pos_len): no 16-bit row's id lies behind the region's at an
    eviction, and there is nothing for rtk_pivotkv_slide_batched to do.)"""
    B, fp8 = cache.video_budget_rows, cache.kv_cache_dtype is not None

    def scored(l, st, first, n, ids):
        if st.sc is None or st.sc_len != n or (ids and st.c.pos_len != first + n):
            raise ValueError(f"video_budget_rows: layer {l} holds {n} video rows"
                             f"{'' if fp8 else ' and other rows'} behind its pinned rows and scores for "
                             f"{st.sc_len if st.sc is not None else 0} of them - text or decode rows were appended after the "
                             "video and left in place.  Rewind to `video_end` before the stream goes on (a question's "
                             "rows carry no score and cannot take part in the eviction)")
    by_device = _plan(cache, "video_budget_rows", "cannot be evicted", scored)
    if by_device and cache.video_position_limit is not None:
        _rebase_rotary(cache)   # (raises before the move, not between the move and the re-base)
    for dev, layers in by_device.items():
        idx = cache._buf(f"budget_idx{dev}", (len(layers), B), torch.int32, layers[0][1]._k.device)
        sel = (nv.BudgetSelectUnit * len(layers))()
        units = []
        for i, (_, st, _, n, _, streams) in enumerate(layers):
            ip = idx[i].data_ptr()
            sel[i].score, sel[i].idx, sel[i].n, sel[i].keep = st.sc.data_ptr(), ip, n, B
            units += [s + (B, n, ip) for s in streams + [(st.sc.data_ptr(), 0, 1, 4, 0)]]
        _launch(dev, "rtk_pivotkv_budget_select_batched", sel, len(layers))
        _launch(dev, "rtk_pivotkv_squeeze_batched", (nv.SqueezeUnit * len(units))(*[nv.SqueezeUnit(*u) for u in units]), len(units))
    if by_device:
        _commit(cache, by_device, cache.budget_dropped)
        for layers in by_device.values():
            for _, st, *_ in layers:
                st.sc_len = st.sc_seen = B
        rebase_positions(cache, by_device)


def keep_scores(cache, b: _Batch, layers):
    """video_budget_rows: the scores of the rows a flush has just committed, `score[keep_idx[r]]` as the selection left
    them (key-patch rows at 1.0), into the layers' score stores at those rows - one rtk_pivotkv_keep_scores_batched
    launch per flush, whichever route flushed (so also per `flush_every_layers` group)."""
    if cache.video_budget_rows is None:
        return
    keep, fp8 = b.keep, cache.kv_cache_dtype is not None
    units = (nv.KeepScoresUnit * len(layers))()
    for u, l in zip(units, layers):
        st, sl = cache._layers[l], b.slot(l)
        at = (st.len8 if fp8 else st.c.length - st.pinned) - keep    # region row of the first kept row
        if st.sc is None or st.sc.numel() < at + keep:
            cap = max(at + keep, 2 * (st.sc.numel() if st.sc is not None else 0), 1024, region_room(cache, st, 0, b.L))
            sc = torch.empty(cap, dtype=torch.float32, device=b.device)
            if st.sc is not None and st.sc_len:
                sc[:st.sc_len].copy_(st.sc[:st.sc_len])
            st.sc = sc
        u.score, u.keep_idx = b.score[sl].data_ptr(), b.keep_idx[sl].data_ptr()
        u.dst, u.keep = st.sc.data_ptr() + 4 * at, keep
        if st.sc_len == at:   # (else: unscored rows lie in between - text that was not rewound; `evict_budget` raises)
            st.sc_len = at + keep
    _launch(b.dev_index, "rtk_pivotkv_keep_scores_batched", units, len(layers))


def row_scores(cache, layer_idx: int) -> torch.Tensor:
    """video_budget_rows: a copy of the scores the layer's video region keeps, fp32, in region order (deferred work is
    flushed first).  Empty for a layer without video rows; ValueError with the budget off."""
    if cache.video_budget_rows is None:
        raise ValueError("PivotKVCache.row_scores: no scores are kept without video_budget_rows")
    cache._flush()
    st = cache._layers[layer_idx] if layer_idx < len(cache._layers) else None
    if st is None or st.sc is None:
        return torch.empty(0, dtype=torch.float32)
    return st.sc[:st.sc_len].clone()


def observe(cache, st: _LayerStore, q: torch.Tensor):
    """video_budget_rescore: the last min(W, L) rows of every head of the chunk's ROTATED queries q [1, Hq, L, D] into the
    layer's buffer [Hq, W, D], on the current stream - every route by which a compressing chunk enters calls this where it
    returns (a slice copy: the prepare and prologue kernels are not touched)."""
    W = cache.video_budget_observe_rows
    _, Hq, L, D = q.shape
    if st.oq is None or st.oq.shape != (Hq, W, D) or st.oq.dtype != q.dtype or st.oq.device != q.device:
        st.oq = torch.empty((Hq, W, D), dtype=q.dtype, device=q.device)
    st.oq_rows = min(W, L)
    st.oq[:, :st.oq_rows].copy_(q[0, :, L - st.oq_rows:])
    st.oq_new = True


def observed_queries(cache, layer_idx: int) -> torch.Tensor:
    """video_budget_rescore: a copy [Hq, Wc, D] of the rotated query rows the layer's next re-scoring observes with (its
    newest chunk's last Wc = min(video_budget_observe_rows, L)); empty before the first chunk; ValueError with the key off."""
    if cache.video_budget_rescore is None:
        raise ValueError("PivotKVCache.observed_queries: no queries are kept without video_budget_rescore")
    st = cache._layers[layer_idx] if 0 <= layer_idx < len(cache._layers) else None
    if st is None or st.oq is None:
        return torch.empty(0)
    return st.oq[:, :st.oq_rows].clone()


def rescore_groups(who, groups, alpha, q_rows, scratch, room=0, sized_rows=None):
    """rtk_pivotkv_rescore_batched for `groups`: {(device index, Hq, Hkv, Wc, D, dtype code): [(q, k, first, score, n), ..]},
    one call per group on the device's current stream - q the unit's query buffer [Hq, q_rows, D] (the first Wc rows of
    each head count), k the layer's key buffer [1, Hkv, cap, D] whose rows [first, first + n) are scored, score its fp32 row.
    A key with a seventh element "fp8" is a group over e4m3 archive rows (archive_rescore): k is then (codes uint8
    [1, Hkv, cap8, D], scales fp32 [1, Hkv, cap8]) and the call is rtk_pivotkv_rescore_fp8k_batched; the dtype code is the
    queries'.
    A unit's scratch is sized for max(room, the group's largest n) region rows and `sized_rows` query rows (None: Wc);
    `scratch(dev, device, stride, units)` answers with a uint8 buffer of at least units * stride + 256 bytes.  ValueError
    under `who`'s name for a shape the kernel does not serve, raised for every group before the first launch."""
    strides = {}
    for key, es in groups.items():
        _, Hq, Hkv, Wc, D, dt = key[:6]
        rows, most = sized_rows or Wc, max(room, max(e[4] for e in es))
        strides[key] = nv.lib.rtk_pivotkv_rescore_workspace_bytes(Hq, Hkv, rows, most, D, dt)
        if strides[key] == 0:
            raise ValueError(f"{who}: rtk_pivotkv_rescore_batched does not serve Hq {Hq}, Hkv {Hkv}, {rows} query rows, "
                             f"{most} region rows, head_dim {D}")
    for key, es in groups.items():
        (dev, Hq, Hkv, Wc, D, dt), fp8, stride = key[:6], key[6:] == ("fp8",), strides[key]
        ws = scratch(dev, es[0][0].device, stride, len(es))
        if fp8:
            name = "rtk_pivotkv_rescore_fp8k_batched"
            units = (nv.RescoreFp8kUnit * len(es))(*[
                nv.RescoreFp8kUnit(q.data_ptr(), k8.data_ptr() + first * D, k8.stride(1), ks.data_ptr() + first * 4, ks.stride(1),
                                   score.data_ptr(), n) for q, (k8, ks), first, score, n in es])
        else:
            name = "rtk_pivotkv_rescore_batched"
            units = (nv.RescoreUnit * len(es))(*[
                nv.RescoreUnit(q.data_ptr(), k.data_ptr() + first * k.shape[3] * k.element_size(), k.stride(1), score.data_ptr(), n)
                for q, k, first, score, n in es])
        nv.check(_on_device(dev, getattr(nv.lib, name), units, len(es), Hq, Hkv, Wc, D, dt, alpha, q_rows * D, D,
                            (ws.data_ptr() + 255) & ~255, stride, nv.raw_stream(dev)), name)


def rescore_budget(cache):
    """video_budget_rescore = alpha (not in the reference, which processes a finished video; a rule of this project's own,
    answer quality not evaluated).  Called by `after_forward` after the flush and in front of `evict_budget` - so before any
    re-base or renumbering: the keys are read as they lie, rotated, at their current ids.  For every layer whose region
    holds scored rows only (sc_len == n, what the eviction demands too) and whose newest chunk left its queries, with n_old
    the region rows that existed at the last re-scoring, Q the layer's observed queries [Hq, Wc, D] and K the region's keys:

        p_h[i, .] = softmax over j < n_old of (Q[h, i] . K[h // G, j] / sqrt(D))      no mask; rows >= n_old are never read
        obs[j]    = (n_old / (Hq Wc)) sum_h sum_i p_h[i, j]                           averages 1 over the old rows
        score[j]  = fmaf(alpha, obs[j], (1 - alpha) * score[j])  in fp32, j < n_old;  newer rows keep their arrival score

    ONE rtk_pivotkv_rescore_batched call per device and (Hq, Hkv, Wc, D, dtype) group.  With fp8 rows (archive_rescore) a
    layer's region is its archive - first = archive_at, n = len8 - K[g, j] = dtype(float(code) * scale) of the archive's
    key rows, and the call is rtk_pivotkv_rescore_fp8k_batched; everything else is the same.  n_old == 0 (the first chunk) does
    nothing; afterwards n_old is the region's rows (`evict_budget` sets it to the budget).  A layer with question or decode
    rows left behind its video is skipped - the eviction raises for it as it always did.  The scratch is one buffer per
    device, sized once for a full region with its slack and a chunk: no buffer is replaced after warm-up."""
    alpha, W = cache.video_budget_rescore, cache.video_budget_observe_rows
    fp8 = cache.kv_cache_dtype is not None
    groups, layers = {}, []
    for l, st in enumerate(cache._layers):
        first = st.archive_at if fp8 else st.pinned
        if st._k is None or first < 0 or st.sc is None or st.oq is None or not st.oq_new or st.c.cap == 0:
            continue
        n = st.len8 if fp8 else st.c.length - first
        if n <= 0 or st.sc_len != n:
            continue
        st.oq_new = False
        n_old, st.sc_seen = min(st.sc_seen, n), n
        if n_old == 0:
            continue
        k, Hq = st._k, st.oq.shape[0]
        key = (k.get_device(), Hq, k.shape[1], st.oq_rows, k.shape[3], nv.dtype_code(k))
        if fp8:   # the archive from its row 0: codes and scales
            groups.setdefault(key + ("fp8",), []).append((st.oq, (st.k8, st.ks8), 0, st.sc, n_old))
        else:
            groups.setdefault(key, []).append((st.oq, k, first, st.sc, n_old))
        layers.append(l)
    if not groups:
        return
    L = cache._batch.L if cache._batch is not None else 0
    rescore_groups("video_budget_rescore", groups, alpha, W,
                   lambda dev, device, stride, _: cache._buf(f"rescore_ws{dev}", (len(cache._layers) * stride + 256,),
                                                             torch.uint8, device),
                   room=sum(bound(cache)) + L, sized_rows=W)
    done = cache.budget_rescored
    done.extend([0] * (len(cache._layers) - len(done)))
    for l in layers:
        done[l] += 1

"""The question-focused decode cache of PivotKVCache (not in the reference; a rule of this project's own - what it does to
answer quality has not been evaluated).  PivotKV chooses a video's rows before any question exists; once the question is
known most of those rows get almost no attention from it, yet every generated token reads all of them in every layer.
The functions take the cache (longvideo_cache binds them as methods).

`watch_question(rows)` arms a capture: from then on every UNCOMPRESSED segment that enters a layer - `update` with
compression off when cache_kwargs carries `query_states`, and `append_pre_rope` - leaves the last min(rows, Lq) rotated query
rows of every head in a per-layer buffer [Hq, rows, D] (`capture`: a slice copy where the route returns, exactly as
_video_bound.observe does for compressing chunks; the prepare, prologue and append kernels are not touched).  A later
segment overwrites an earlier one, decode tokens count.  It records `video_end` as it is at arming time.

`focus(keep_rows)` returns a small cache of its own.  Per layer, with `first` the layer's pinned rows, `ve` its length at the
recorded video_end, n = ve - first, Q the watched queries [Hq, Wc, D] and K the stored rotated keys of rows [first, ve):

    p_h[i, .] = softmax over j < n of (Q[h, i] . K[h // G, j] / sqrt(D))         no mask
    obs[j]    = (n / (Hq Wc)) sum_h sum_i p_h[i, j]                              fp32, averages 1 over the region
    keep      = min(keep_rows, n)
    idx       = ascending list of: row n - 1 always, and of rows [0, n - 1) the keep - 1 with the highest obs, ties to the
                lowest index

obs is rtk_pivotkv_rescore_batched with alpha = 1 into a zeroed fp32 score row (fmaf(1, obs, 0 * 0) is obs exactly), idx is
rtk_pivotkv_budget_select_batched - both as they are: one re-scoring call per device and shape group, one selection call
per device.  Then ONE rtk_pivotkv_focus_gather_batched call per device moves, out of place, K, V and ids of every layer:
rows [0, first), rows first + idx[.], rows [ve, length) - the question and whatever was decoded - into the new cache's
buffers.  K bits, V bits and ids are unchanged: keys stay rotated at their ids, and holes in the ids are what the budget
already leaves.  The parent is only read: lengths, counters, marks, branches, scores and `video_end` stay valid.

An fp8 parent (kv_cache_dtype="fp8_e4m3") is served with longvideo_kwargs["archive_rescore"] = True; the focused cache is
then an fp8 cache itself.  A layer's region is its archive: first = archive_at, n = len8 as recorded at `video_end`, and
K[g, j] = dtype(float(code) * scale) of the archive's key rows (rtk_pivotkv_rescore_fp8k_batched: the codes are dequantised
where the kernel loads a key - scores taken on e4m3 keys are another rule than scores taken on 16-bit keys, and what that
does to answer quality has not been evaluated).  The same gather call moves more streams per layer: the codes of K and V
(row bytes D) and their scales (row bytes 4) as archive rows idx[.] into an archive reserved for exactly `keep` rows, the ids
as rows [0, archive_at), archive_at + idx[.], [archive_at + len8, pos_len), and ALL the layer's 16-bit rows - the pinned
rows and whatever lies behind `video_end` - as they lie (head rows of a unit that gathers nothing)."""
import torch

from . import _native as nv
from ._cache_state import _on_device
from ._video_bound import rescore_groups


class _Watch:
    """An armed capture: the rows asked for, the `video_end` recorded at arming, and per layer the buffer [Hq, rows, D]
    with the rows in use."""

    __slots__ = ("rows", "mark", "q", "q_rows")

    def __init__(self, rows, mark):
        self.rows, self.mark, self.q, self.q_rows = rows, mark, {}, {}


def _is_int(x, least):
    return isinstance(x, int) and not isinstance(x, bool) and x >= least


def _refuse_focused(cache, who: str):
    if cache.focused_from is not None:
        raise NotImplementedError(f"PivotKVCache.{who}: this cache is a focused cache (PivotKVCache.focus) - it holds the rows "
                                  "one question reads and serves text and decode rows only; call the parent")


def refuse_compression(cache, who: str):
    """What every row-writing entry point of a focused cache checks first: the call does not compress."""
    if cache.kvcache_compression:
        raise NotImplementedError(f"{who}: a focused cache (PivotKVCache.focus) does not compress video chunks - feed the "
                                  "video to the parent (or set kvcache_compression = False)")


def watch_question(cache, rows: int = 64) -> None:
    """Arm the capture (see the module docstring).  ValueError for `rows` that is not an int >= 1 (a bool is not an int) and
    for a cache without `video_end` (no compressed chunk has been flushed); NotImplementedError on a focused cache and on a
    branch.  Arming again drops what was captured."""
    if not _is_int(rows, 1):
        raise ValueError(f"PivotKVCache.watch_question: rows must be an int >= 1, got {rows!r}")
    _refuse_focused(cache, "watch_question")
    if cache.forked_from is not None:
        raise NotImplementedError("PivotKVCache.watch_question: not served on a branch (PivotKVCache.fork) - focusing a "
                                  "branch is not built")
    ve = cache.video_end
    if ve is None:
        raise ValueError("PivotKVCache.watch_question: the cache has no `video_end` - no compressed chunk has been flushed, "
                         "there are no video rows to focus")
    cache._watch = _Watch(rows, ve)


def unwatch_question(cache) -> None:
    """Disarm and free the buffers; nothing is captured afterwards."""
    cache._watch = None


def capture(cache, layer_idx: int, q: torch.Tensor):
    """The last min(rows, Lq) rows of every head of the segment's ROTATED queries q [1, Hq, Lq, D] into the layer's buffer,
    on the current stream."""
    w = cache._watch
    _, Hq, L, D = q.shape
    buf = w.q.get(layer_idx)
    if buf is None or buf.shape != (Hq, w.rows, D) or buf.dtype != q.dtype or buf.device != q.device:
        buf = w.q[layer_idx] = torch.empty((Hq, w.rows, D), dtype=q.dtype, device=q.device)
    n = w.q_rows[layer_idx] = min(w.rows, L)
    buf[:, :n].copy_(q[0, :, L - n:])


def watched_queries(cache, layer_idx: int) -> torch.Tensor:
    """A copy [Hq, Wc, D] of the rotated query rows `focus` would observe with in this layer (the last uncompressed
    segment's last Wc = min(rows, Lq)); empty before any segment; ValueError while not armed."""
    w = cache._watch
    if w is None:
        raise ValueError("PivotKVCache.watched_queries: no queries are kept without watch_question")
    buf = w.q.get(layer_idx)
    if buf is None:
        return torch.empty(0)
    return buf[:, :w.q_rows[layer_idx]].clone()


def watched_bytes(cache) -> int:
    return sum(t.numel() * t.element_size() for t in cache._watch.q.values())


def _plan(cache, w, keep_rows):
    """[(layer, store, first, ve, n, keep, tail, ids, Q, Wc)] of the layers that own rows - ValueError for what cannot be
    focused, before anything is launched.  With fp8 rows the region is the archive: first = archive_at, n = len8, and `tail`
    counts the 16-bit rows behind `video_end`."""
    who, fp8 = "PivotKVCache.focus", cache.kv_cache_dtype is not None
    ve = cache.video_end
    if ve is None or ve.serial != w.mark.serial or cache._mark_is_dead(ve.serial) or ve.epoch != cache._epoch \
            or cache._flushes != ve.flushes or cache._compressed_in_forward or len(cache._layers) != ve.n_layers:
        raise ValueError(f"{who}: `video_end` is no longer the mark recorded by watch_question - a chunk, a slide, an "
                         "eviction or a rewind below it happened since.  Rewind to `video_end`, call watch_question and "
                         "feed the question again")
    plan = []
    for l, (st, m) in enumerate(zip(cache._layers, ve.layers)):
        if st._k is None:
            continue
        first, length = (st.archive_at if fp8 else st.pinned), st.c.length
        n, tail = (m.len8 if fp8 else m.length - first), length - m.length
        if first < 0 or n < 1 or not m.has_kv or (fp8 and (st.k8 is None or st.len8 != n or first > m.length)):
            raise ValueError(f"{who}: layer {l} holds no video rows behind its pinned rows")
        if tail < 1:
            raise ValueError(f"{who}: nothing lies behind `video_end` in layer {l} - feed the question first")
        ids = st._pos is not None and st.c.pos_len > 0
        if st.c.cap == 0 or (ids and st.c.pos_len != length + st.len8):
            raise ValueError(f"{who}: layer {l} cannot be focused - its buffers are not the cache's own dense blocks, or it "
                             f"keeps ids for {st.c.pos_len} of its {length + st.len8} rows")
        Q, k = w.q.get(l), st._k
        if Q is None:
            raise ValueError(f"{who}: layer {l} has rows behind `video_end` but no watched queries - the question did not "
                             "enter it through `update` (with query_states) or `append_pre_rope` after watch_question")
        if Q.dtype != k.dtype or Q.device != k.device or Q.shape[2] != k.shape[3] or Q.shape[0] % k.shape[1]:
            raise ValueError(f"{who}: layer {l}: the watched queries {tuple(Q.shape)} {Q.dtype} do not go with keys "
                             f"{tuple(k.shape)} {k.dtype}")
        plan.append((l, st, first, m.length, n, min(keep_rows, n), tail, ids, Q, w.q_rows[l]))
    if not plan:
        raise ValueError(f"{who}: the cache holds no rows")
    return plan


def focus(cache, keep_rows: int, reserve_tokens=None):
    """The focused cache of the question watched since `watch_question` (see the module docstring): a standalone
    PivotKVCache that owns all its rows - not a view, not a branch - built from this cache's config, its buffers sized by
    `reserve_tokens` (default: its rows + 1024).  Per layer it holds rows [0, first), first + idx[.], [ve, length) of this
    cache; `num_evicted_tokens[l]` is this cache's plus n - keep, `get_prev_temporal_idx` reads the last stored id, which is
    unchanged.  It takes text and decode rows through both uncompressed routes, has `mark` / `rewind` / `crop` down to its
    own focus point and serves every attention route its rows would in this cache; it raises NotImplementedError for a
    compressing `update` / `update_pre_rope`, for `fork`, `focus` and `watch_question`.  It carries no score store, no
    window, no budget and no position limit; `position_offset` answers with copies of this cache's values.
    `focus_scores(l)` / `focus_kept(l)` / `focus_dropped`: obs [n], idx [keep] and the per-layer n - keep.

    This cache is not written to.  ValueError, before any launch: keep_rows not an int >= 1; kv_cache_dtype set without
    archive_rescore (with it the archive's key rows are scored as they lie and the focused cache is an fp8 cache, its
    archive reserved for exactly `keep` rows - see the module docstring); not armed, or a layer with rows behind `video_end` and no watched queries;
    `video_end` no longer the mark recorded at arming; nothing behind `video_end`; a shape the re-scoring does not serve.
    NotImplementedError: defer_rerotation, a branch, a focused cache."""
    who = "PivotKVCache.focus"
    if not _is_int(keep_rows, 1):
        raise ValueError(f"{who}: keep_rows must be an int >= 1, got {keep_rows!r}")
    if reserve_tokens is not None and not _is_int(reserve_tokens, 1):
        raise ValueError(f"{who}: reserve_tokens must be an int >= 1 (or None: the focused rows + 1024), got {reserve_tokens!r}")
    _refuse_focused(cache, "focus")
    if cache.forked_from is not None:
        raise NotImplementedError(f"{who}: not served on a branch (PivotKVCache.fork) - focusing a branch is not built; focus "
                                  "the parent")
    if cache.defer_rerotation:
        raise NotImplementedError(f"{who}: a cache with defer_rerotation (the sharded prefill's block caches) holds un-rotated "
                                  "keys and provisional ids until `finalize`; it has no restore points")
    fp8 = cache.kv_cache_dtype is not None
    if fp8 and not cache.archive_rescore:
        raise ValueError(f"{who} does not serve kv_cache_dtype={cache.kv_cache_dtype!r}: the archive's e4m3 key rows are not "
                         "scored again, it is not built - unless asked for: set archive_rescore=True")
    w = cache._watch
    if w is None:
        raise ValueError(f"{who}: the cache is not armed - call watch_question before the question is fed")
    cache._flush()
    cache._shift_latch_check()
    plan = _plan(cache, w, keep_rows)
    groups, by_device = {}, {}
    for p in plan:
        l, st, first, ve, n, keep, tail, ids, Q, Wc = p
        k = st._k
        key = (k.get_device(), Q.shape[0], k.shape[1], Wc, k.shape[3], nv.dtype_code(k)) + (("fp8",) if fp8 else ())
        groups.setdefault(key, []).append(p)
        by_device.setdefault(k.get_device(), []).append(p)

    # ---- what the question's queries see of the region, and the rows that stay: per device, on the current stream ----
    score, kept = {}, {}
    for dev, ps in by_device.items():
        device = ps[0][1]._k.device
        sc = torch.zeros((len(ps), max(p[4] for p in ps)), dtype=torch.float32, device=device)
        ix = torch.empty((len(ps), max(p[5] for p in ps)), dtype=torch.int32, device=device)
        for i, p in enumerate(ps):
            score[p[0]], kept[p[0]] = sc[i, :p[4]], ix[i, :p[5]]
    rescore_groups(who, {key: [(Q, (st.k8, st.ks8), 0, score[l], n) if fp8 else (Q, st._k, first, score[l], n)
                               for l, st, first, _, n, _, _, _, Q, _ in ps] for key, ps in groups.items()}, 1.0, w.rows,
                   lambda dev, device, stride, units: torch.empty(units * stride + 256, dtype=torch.uint8, device=device))
    for dev, ps in by_device.items():
        sel = (nv.BudgetSelectUnit * len(ps))()
        for u, p in zip(sel, ps):
            u.score, u.idx, u.n, u.keep = score[p[0]].data_ptr(), kept[p[0]].data_ptr(), p[4], p[5]
        nv.check(_on_device(dev, nv.lib.rtk_pivotkv_budget_select_batched, sel, len(ps), nv.raw_stream(dev)),
                 "rtk_pivotkv_budget_select_batched")

    # ---- the focused cache: buffers of its own, filled by one gather call per device ---------------------------------
    rows = max((p[1].c.length if fp8 else p[2]) + p[5] + (0 if fp8 else p[6]) for p in plan)
    fc = type(cache)(cache.config, reserve_tokens=reserve_tokens if reserve_tokens is not None else rows + 1024)
    fc.attention_kernel, fc.decode_attention = cache.attention_kernel, cache.decode_attention
    fc.multi_token_attention = cache.multi_token_attention
    fc.kv_cache_dtype = cache.kv_cache_dtype
    fc.kvcache_compression = False
    fc._warned = True
    fc._store(len(cache._layers) - 1)
    nev = cache.num_evicted_tokens
    fc.num_evicted_tokens = list(nev)
    fc.focus_dropped = [0] * len(cache._layers)
    for dev, ps in by_device.items():
        units = []
        for l, pst, first, ve, n, keep, tail, ids, _, _ in ps:
            st, k = fc._layers[l], pst._k
            H, D = k.shape[1], k.shape[3]
            length = pst.c.length if fp8 else first + keep + tail      # the focused layer's 16-bit rows
            total = length + (keep if fp8 else 0)                      # ... and its rows in sequence order: its ids
            cap = max(fc.reserve_tokens, length)
            st.k = torch.empty((1, H, cap, D), dtype=k.dtype, device=k.device)
            st.v = torch.empty((1, H, cap, D), dtype=k.dtype, device=k.device)
            st.length, st.pinned = length, pst.pinned
            row, ix = D * k.element_size(), kept[l].data_ptr()
            region = (first, first, n, keep, ve, tail, ix)   # rows [0, first), first + idx[.], [ve, ve + tail)
            # (source, destination, streams, row bytes, then head, first, n, keep, tail_src, tail, idx)
            if fp8:
                st.k8, st.v8 = (torch.empty((1, H, keep, D), dtype=torch.uint8, device=k.device) for _ in range(2))
                st.ks8, st.vs8 = (torch.empty((1, H, keep), dtype=torch.float32, device=k.device) for _ in range(2))
                st.len8, st.archive_at = keep, first
                archive, as_they_lie = (0, 0, n, keep, 0, 0, ix), (length, 0, 0, 0, 0, 0, None)
                moves = [(pst.k8, st.k8, H, D) + archive, (pst.v8, st.v8, H, D) + archive,
                         (pst.ks8, st.ks8, H, 4) + archive, (pst.vs8, st.vs8, H, 4) + archive,
                         (pst._k, st._k, H, row) + as_they_lie, (pst._v, st._v, H, row) + as_they_lie]
                region = (first, first, n, keep, first + n, pst.c.pos_len - first - n, ix)
            else:
                moves = [(pst._k, st._k, H, row) + region, (pst._v, st._v, H, row) + region]
            if ids:
                P = pst._pos.shape[0]
                st.pos = torch.empty((P, cap + (keep if fp8 else 0)), dtype=torch.int64, device=pst._pos.device)
                st.pos_len, st.pos_ndim = total, pst.pos_ndim
                moves.append((pst._pos, st._pos, P, 8) + region)
            for src, dst, streams, rb, *rest in moves:   # (stream strides: rows of a stream x row bytes)
                units.append(nv.FocusUnit(src.data_ptr(), dst.data_ptr(), src.shape[-2 if src.dim() == 4 else -1] * rb,
                                          dst.shape[-2 if dst.dim() == 4 else -1] * rb, streams, rb, *rest))
            fc.update_num_evicted_tokens(n - keep, l)
            fc.focus_dropped[l] = n - keep
        nv.check(_on_device(dev, nv.lib.rtk_pivotkv_focus_gather_batched, (nv.FocusUnit * len(units))(*units), len(units),
                            nv.raw_stream(dev)), "rtk_pivotkv_focus_gather_batched")
    fc._pos_layers = cache._pos_layers
    if hasattr(cache, "_seen_tokens"):
        fc._seen_tokens = cache._seen_tokens
    fc._flushes = cache._flushes
    fc._position_offsets = {d: t.clone() for d, t in cache._position_offsets.items()}
    fc._focus_scores, fc._focus_kept = score, kept
    fc.focused_from = w.mark
    # the focused cache's own restore point: its `video_end` and crop floor
    fc.last_compressed_mark = fc._take_mark(True)
    return fc


def focus_scores(cache, layer_idx: int) -> torch.Tensor:
    """A focused cache: a copy of obs [n] of the layer, fp32 (empty for a layer without rows); ValueError on any other cache."""
    if cache.focused_from is None:
        raise ValueError("PivotKVCache.focus_scores: this cache is not a focused cache (PivotKVCache.focus)")
    t = cache._focus_scores.get(layer_idx)
    return torch.empty(0, dtype=torch.float32) if t is None else t.clone()


def focus_kept(cache, layer_idx: int) -> torch.Tensor:
    """A focused cache: a copy of idx [keep] of the layer, int32 region rows, ascending; ValueError on any other cache."""
    if cache.focused_from is None:
        raise ValueError("PivotKVCache.focus_kept: this cache is not a focused cache (PivotKVCache.focus)")
    t = cache._focus_kept.get(layer_idx)
    return torch.empty(0, dtype=torch.int32) if t is None else t.clone()

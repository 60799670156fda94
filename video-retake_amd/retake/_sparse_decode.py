"""The page-sparse decode route of PivotKVCache (not in the reference; a rule of this project's own - what it does to answer
quality has not been evaluated).  Every generated token reads every stored video row in every layer; `focus` answers that
by copying the rows one question reads into a second cache, once, one list per layer.  This route copies nothing: the
rows stay where they lie, a small index of per-page key bounds sits beside them, and each decode call picks - per kv head
and per token - the pages whose upper bound on the logit is highest (after Quest, Tang et al. 2024).  The functions take
the cache as their first argument: `sparse_decode(cache, keep_rows)`.  They are not bound as methods - PivotKVCache keeps
exactly the names it had (tests/test_cache_surface_cpu.py pins them); the state they keep is the instance's `_sparse`,
`sparse_attention_calls` and `page_summary_calls`.

Per layer, with `first` the layer's pinned rows, `ve` its length at the recorded `video_end`, n = ve - first region rows and
pages = ceil(n / 32) (a page is one key tile of the packed decode kernel; page p is region rows [32 p, min(32 p + 32, n))):

    summ[g, p, 0 / 1, d] = max / min over the rows r of page p of K[g, first + r, d]          model dtype, exact
    ub[g, p]             = max over the packed rows (hh, i) of kv head g of
                           sum_d max(q[d] * summ[g, p, 0, d], q[d] * summ[g, p, 1, d])          fp32, no scale
    keep_pages           = min(ceil(keep_rows / 32), pages)
    list[g]              = ascending: page pages - 1 always, and of the others the keep_pages - 1 with the highest ub,
                           ties to the lowest index
    out                  = the packed decode kernel's arithmetic over
                           [rows [0, first) | pages list[g][0], list[g][1], ... | rows [ve, Lk)]

`sparse_decode(cache, keep_rows)` arms the route: it records `video_end` as `watch_question` does and builds the summaries of
every layer with ONE rtk_pivotkv_page_summary_batched call per device (1/16 of K's bytes).  While armed, a `cache.attention`
call with rows behind `video_end` that the library serves - bf16 / fp16, head_dim 128, (Hq / Hkv) * Lq <= 16, the views of
the layer's own buffers - is ONE rtk_attention_decode_sparse call (bound, selection, paged attention, combine) and counts
in `sparse_attention_calls`; every other call takes the existing routes, bit for bit.  The index survives
`rewind(video_end)`: the next question pays nothing.  `dense_decode(cache)` disarms and frees.

kv_cache_dtype="fp8_e4m3": `sparse_decode(cache, keep_rows, archive=True)` arms the route over the fp8 ARCHIVE.  The region
is the archive as recorded at `video_end` - n = len8 rows, page p is archive rows [32 p, min(32 p + 32, n)) - and the 16-bit
buffer holds the pinned rows and everything behind the video; as in rtk_attention_decode_fp8kv every archive row is visible
to every query row and the 16-bit rows follow the archive and carry the diagonal:

    summ[g, p, 0 / 1, d] = max / min over the rows j of page p of K[g, j, d] = dtype(float(code) * scale)    exact (rule 5 of the
                           fp8 rows): 16-bit values of the keys the attention really uses, so ub bounds their logits
    out                  = the packed decode kernel's arithmetic over [archive pages list[g][0], list[g][1], ... | 16-bit rows]

with ub, keep_pages and list as above.  Arming is ONE rtk_pivotkv_page_summary_fp8k_batched call per device over the K codes
and scales (16 bytes of summaries per (kv head, row) beside 132 of K codes + scale: about 12 % of the K archive, 6 % of
K + V); a served call is ONE rtk_attention_decode_sparse_fp8kv call.  The key is independent of `archive_rescore`.

Not served (refused at arming, before any launch): kv_cache_dtype without archive=True (and archive=True without
kv_cache_dtype), a branch, a focused cache, defer_rerotation, an fp32 model, head_dim != 128.  Not built: the wide kernel, the sharded path, incremental index updates
while the video grows (a chunk after arming makes the next routed call raise: arm again)."""
import torch

from . import _native as nv
from ._cache_state import _on_device

PAGE = nv.PAGE_ROWS


class _Sparse:
    """An armed route: keep_rows, the `video_end` recorded at arming, and per layer the summaries [Hkv, pages, 2, D], the
    geometry (first, ve, pages) and the workspace of the layer's last routed call (ub | lists | partials).  `archive`: the
    pages are the fp8 archive's; the geometry is then (16-bit rows at `video_end`, len8 at `video_end`, pages)."""

    __slots__ = ("keep_rows", "mark", "summ", "geom", "ws", "last", "archive")

    def __init__(self, keep_rows, mark, archive=False):
        self.keep_rows, self.mark, self.summ, self.geom, self.ws, self.last = keep_rows, mark, {}, {}, {}, {}
        self.archive = archive


def _is_int(x, least):
    return isinstance(x, int) and not isinstance(x, bool) and x >= least


def _mark_moved(cache, mark) -> bool:
    ve = cache.video_end
    return ve is None or ve.serial != mark.serial or cache._mark_is_dead(ve.serial) or ve.epoch != cache._epoch \
        or cache._flushes != ve.flushes or cache._compressed_in_forward or len(cache._layers) != ve.n_layers


def sparse_decode(cache, keep_rows: int = 8192, archive: bool = False) -> None:
    """Arm the page-sparse decode route (see the module docstring).  ValueError, before any launch: keep_rows not an int
    >= 1 (a bool is not an int), archive not a bool, a cache without `video_end`, attention_kernel other than "hip",
    kv_cache_dtype set without archive=True (the pages of an fp8 cache are its archive's: an opt-in of its own), archive=True
    on a cache without kv_cache_dtype.  NotImplementedError: a branch, a focused cache, defer_rerotation, an fp32 model or
    head_dim other than 128.  Arming again rebuilds the index."""
    who = "sparse_decode"
    if not _is_int(keep_rows, 1):
        raise ValueError(f"{who}: keep_rows must be an int >= 1, got {keep_rows!r}")
    if not isinstance(archive, bool):
        raise ValueError(f"{who}: archive must be a bool, got {archive!r}")
    if cache.focused_from is not None:
        raise NotImplementedError(f"{who}: this cache is a focused cache (PivotKVCache.focus) - it already holds the rows one "
                                  "question reads")
    if cache.forked_from is not None:
        raise NotImplementedError(f"{who}: not served on a branch (PivotKVCache.fork) - the paged kernel reads one buffer; "
                                  "branches and BranchGroup are not built")
    if cache.defer_rerotation:
        raise NotImplementedError(f"{who}: a cache with defer_rerotation (the sharded prefill's block caches) holds un-rotated "
                                  "keys until `finalize`; the sharded path is not built")
    if cache.kv_cache_dtype is not None and not archive:
        raise ValueError(f"{who} does not serve kv_cache_dtype={cache.kv_cache_dtype!r}: page bounds over the fp8 archive are "
                         "not built unless asked for - pass archive=True")
    if archive and cache.kv_cache_dtype is None:
        raise ValueError(f"{who}: archive=True needs a cache with kv_cache_dtype set - this cache keeps its video rows in the "
                         "16-bit buffers, which archive=False indexes")
    if cache.attention_kernel != "hip":
        raise ValueError(f"{who} needs attention_kernel=\"hip\": the route lives in PivotKVCache.attention, got "
                         f"{cache.attention_kernel!r}")
    ve = cache.video_end
    if ve is None:
        raise ValueError(f"{who}: the cache has no `video_end` - no compressed chunk has been flushed, there are no video "
                         "rows to index")
    cache._flush()
    cache._shift_latch_check()
    if _mark_moved(cache, ve):
        raise ValueError(f"{who}: `video_end` does not describe the cache's rows any more (a chunk, a slide, an eviction or a "
                         "rewind below it since) - finish the prefill first")
    if archive:
        cache._sparse = _arm_archive(cache, keep_rows, ve, who)
        return
    plan = []
    for l, (st, m) in enumerate(zip(cache._layers, ve.layers)):
        k = st._k
        if k is None or not m.has_kv:
            continue
        first, n = st.pinned, m.length - st.pinned
        if first < 0 or n < 1:
            continue   # a layer without video rows: its calls take the existing routes
        if k.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"{who} needs a bfloat16 or float16 model, got {k.dtype} in layer {l}")
        if k.shape[3] != 128:
            raise NotImplementedError(f"{who} needs head_dim 128, got {k.shape[3]} in layer {l}")
        if st.c.cap == 0 or k.stride(3) != 1 or k.stride(2) != k.shape[3]:
            raise ValueError(f"{who}: layer {l}'s buffers are not the cache's own dense blocks")
        plan.append((l, st, first, m.length, n))
    if not plan:
        raise ValueError(f"{who}: no layer holds video rows behind its pinned rows")
    sp = _Sparse(keep_rows, ve)
    by_device = {}
    for p in plan:
        by_device.setdefault(p[1]._k.get_device(), []).append(p)
    for dev, ps in by_device.items():
        units = (nv.PageSummaryUnit * len(ps))()
        k0 = ps[0][1]._k
        for u, (l, st, first, length, n) in zip(units, ps):
            k = st._k
            if k.shape[1] != k0.shape[1] or k.dtype != k0.dtype:
                raise ValueError(f"{who}: layer {l} differs from layer {ps[0][0]} in kv heads or dtype")
            pages = (n + PAGE - 1) // PAGE
            s = sp.summ[l] = torch.empty((k.shape[1], pages, 2, k.shape[3]), dtype=k.dtype, device=k.device)
            sp.geom[l] = (first, length, pages)
            u.k, u.k_stride_h, u.first, u.n, u.summ, u.summ_stride_h = k.data_ptr(), k.stride(1), first, n, s.data_ptr(), s.stride(0)
        nv.check(_on_device(dev, nv.lib.rtk_pivotkv_page_summary_batched, units, len(ps), k0.shape[1], k0.shape[3],
                            nv.dtype_code(k0), nv.raw_stream(dev)), "rtk_pivotkv_page_summary_batched")
        cache.page_summary_calls += 1
    cache._sparse = sp


def _arm_archive(cache, keep_rows, ve, who):
    """The index over the fp8 archive of every layer: ONE rtk_pivotkv_page_summary_fp8k_batched call per device over the K
    codes and scales from archive row 0."""
    plan = []
    for l, (st, m) in enumerate(zip(cache._layers, ve.layers)):
        k = st._k
        if k is None or not m.has_kv or st.k8 is None or m.len8 < 1 or st.len8 < m.len8:
            continue   # a layer without archived rows: its calls take the existing routes
        if k.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"{who} needs a bfloat16 or float16 model, got {k.dtype} in layer {l}")
        if k.shape[3] != 128:
            raise NotImplementedError(f"{who} needs head_dim 128, got {k.shape[3]} in layer {l}")
        k8, ks8 = st.k8, st.ks8
        if st.c.cap == 0 or k.stride(3) != 1 or k.stride(2) != k.shape[3] or k8.stride(3) != 1 or k8.stride(2) != k8.shape[3] \
                or ks8.stride(2) != 1 or k8.shape[1] != k.shape[1] or k8.shape[3] != k.shape[3]:
            raise ValueError(f"{who}: layer {l}'s buffers are not the cache's own dense blocks")
        plan.append((l, st, m.length, m.len8))
    if not plan:
        raise ValueError(f"{who}: no layer holds archived video rows")
    sp = _Sparse(keep_rows, ve, archive=True)
    by_device = {}
    for p in plan:
        by_device.setdefault(p[1]._k.get_device(), []).append(p)
    for dev, ps in by_device.items():
        units = (nv.PageSummaryFp8kUnit * len(ps))()
        k0 = ps[0][1]._k
        for u, (l, st, length, n) in zip(units, ps):
            k = st._k
            if k.shape[1] != k0.shape[1] or k.dtype != k0.dtype:
                raise ValueError(f"{who}: layer {l} differs from layer {ps[0][0]} in kv heads or dtype")
            pages = (n + PAGE - 1) // PAGE
            s = sp.summ[l] = torch.empty((k.shape[1], pages, 2, k.shape[3]), dtype=k.dtype, device=k.device)
            sp.geom[l] = (length, n, pages)
            u.k8, u.k8_stride_h, u.k_scale, u.scale_stride_h = st.k8.data_ptr(), st.k8.stride(1), st.ks8.data_ptr(), st.ks8.stride(1)
            u.n, u.summ, u.summ_stride_h = n, s.data_ptr(), s.stride(0)
        nv.check(_on_device(dev, nv.lib.rtk_pivotkv_page_summary_fp8k_batched, units, len(ps), k0.shape[1], k0.shape[3],
                            nv.dtype_code(k0), nv.raw_stream(dev)), "rtk_pivotkv_page_summary_fp8k_batched")
        cache.page_summary_calls += 1
    return sp


def dense_decode(cache) -> None:
    """Disarm the route and free the index and its workspaces; every call takes the existing routes again."""
    cache._sparse = None


def sparse_bytes(cache) -> dict:
    sp = cache._sparse
    nb = lambda ts: sum(t.numel() * t.element_size() for t in ts)   # noqa: E731
    return {"page_summaries": nb(sp.summ.values()), "sparse_workspace": nb(sp.ws.values())}


def route(cache, q, k, v, scaling, query_offset, layer_idx):
    """What PivotKVCache.attention asks first while armed: the sparse call's output [1, Lq, Hq, D], or None - take the
    existing routes.  ValueError for a call without layer_idx and for a `video_end` that is no longer the recorded one."""
    sp = cache._sparse
    who = "PivotKVCache.attention (sparse_decode armed)"
    if layer_idx is None:
        raise ValueError(f"{who} needs layer_idx: the route reads the layer's pinned rows and `video_end`")
    geom = sp.geom.get(layer_idx)
    if geom is None or q.dim() != 4 or k.dim() != 4 or q.shape[0] != 1:
        return None
    if sp.archive:
        return _route_archive(cache, sp, who, geom, q, k, v, scaling, query_offset, layer_idx)
    first, ve, pages = geom
    _, Hq, Lq, D = q.shape
    _, Hkv, Lk, _ = k.shape
    if Lk <= ve:
        return None
    if _mark_moved(cache, sp.mark):
        raise ValueError(f"{who}: `video_end` is no longer the mark recorded by sparse_decode - a chunk, a slide, an eviction "
                         "or a rewind below it happened since, and the page index no longer describes the rows.  Call "
                         "sparse_decode again (or dense_decode)")
    st, summ = cache._layers[layer_idx], sp.summ[layer_idx]
    if k.data_ptr() != st._k.data_ptr() or v.data_ptr() != st._v.data_ptr() or k.stride() != v.stride() or k.stride(3) != 1 \
            or q.stride(3) != 1 or not (q.dtype == k.dtype == v.dtype == summ.dtype) or Hkv != summ.shape[0] or D != summ.shape[3] \
            or Hq % Hkv:
        return None
    q_off = Lk - Lq if query_offset is None else int(query_offset)
    if q_off < ve - 1 or q_off < Lk - Lq:
        return None
    keep_pages = min((sp.keep_rows + PAGE - 1) // PAGE, pages)
    code = nv.dtype_code(q)
    need = nv.lib.rtk_attention_decode_sparse_workspace_bytes(Hq, Hkv, Lq, Lk, first, ve, keep_pages, D, code)
    if not need:
        return None   # outside the packed envelope: the existing routes
    ws = sp.ws.get(layer_idx)
    if ws is None or ws.numel() < need:
        ws = sp.ws[layer_idx] = torch.empty(need, dtype=torch.uint8, device=q.device)
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=q.device)
    scale = float(D) ** -0.5 if scaling is None else float(scaling)
    rc = nv.lib.rtk_attention_decode_sparse(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2),
                                            nv.ptr(out), Hq, Hkv, Lq, Lk, q_off, D, code, scale, first, ve, nv.ptr(summ),
                                            summ.stride(0), keep_pages, nv.ptr(ws), ws.numel(),
                                            nv.raw_stream(q.device.index))
    if rc == nv.RTK_EUNSUPPORTED:
        return None
    nv.check(rc, "rtk_attention_decode_sparse")
    sp.last[layer_idx] = (Hkv, pages, keep_pages)
    cache.sparse_attention_calls += 1
    return out


def _route_archive(cache, sp, who, geom, q, k, v, scaling, query_offset, layer_idx):
    """`route` on an fp8 cache: k / v are the layer's 16-bit views, the archive precedes them; query_offset counts over
    archive + views, as PivotKVCache.attention states."""
    ve16, n8, pages = geom
    _, Hq, Lq, D = q.shape
    _, Hkv, Lk, _ = k.shape
    if Lk <= ve16:
        return None
    if _mark_moved(cache, sp.mark):
        raise ValueError(f"{who}: `video_end` is no longer the mark recorded by sparse_decode - a chunk, a slide, an eviction "
                         "or a rewind below it happened since, and the page index no longer describes the rows.  Call "
                         "sparse_decode again (or dense_decode)")
    st, summ = cache._layers[layer_idx], sp.summ[layer_idx]
    if st.len8 != n8 or k.data_ptr() != st._k.data_ptr() or v.data_ptr() != st._v.data_ptr() or k.stride() != v.stride() \
            or k.stride(3) != 1 or q.stride(3) != 1 or not (q.dtype == k.dtype == v.dtype == summ.dtype) or Hkv != summ.shape[0] \
            or D != summ.shape[3] or Hq % Hkv:
        return None
    q_off = Lk - Lq if query_offset is None else int(query_offset) - n8   # in 16-bit rows
    if q_off < Lk - Lq:
        return None
    keep_pages = min((sp.keep_rows + PAGE - 1) // PAGE, pages)
    code = nv.dtype_code(q)
    need = nv.lib.rtk_attention_decode_sparse_fp8kv_workspace_bytes(Hq, Hkv, Lq, Lk, n8, keep_pages, D, code)
    if not need:
        return None   # outside the packed envelope: the existing routes
    ws = sp.ws.get(layer_idx)
    if ws is None or ws.numel() < need:
        ws = sp.ws[layer_idx] = torch.empty(need, dtype=torch.uint8, device=q.device)
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=q.device)
    scale = float(D) ** -0.5 if scaling is None else float(scaling)
    rc = nv.lib.rtk_attention_decode_sparse_fp8kv(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2),
                                                  nv.ptr(st.k8), nv.ptr(st.v8), nv.ptr(st.ks8), nv.ptr(st.vs8), n8, st.k8.stride(1),
                                                  st.ks8.stride(1), nv.ptr(out), Hq, Hkv, Lq, Lk, q_off, D, code, scale,
                                                  nv.ptr(summ), summ.stride(0), keep_pages, nv.ptr(ws), ws.numel(),
                                                  nv.raw_stream(q.device.index))
    if rc == nv.RTK_EUNSUPPORTED:
        return None
    nv.check(rc, "rtk_attention_decode_sparse_fp8kv")
    sp.last[layer_idx] = (Hkv, pages, keep_pages)
    cache.sparse_attention_calls += 1
    return out


def _armed(cache, who):
    sp = cache._sparse
    if sp is None:
        raise ValueError(f"{who}: the cache is not armed (sparse_decode)")
    return sp


def page_summaries(cache, layer_idx: int) -> torch.Tensor:
    """A copy [Hkv, pages, 2, D] of the layer's summaries (kmax at index 0, kmin at 1); empty for a layer without video
    rows; ValueError while not armed."""
    t = _armed(cache, "page_summaries").summ.get(layer_idx)
    return torch.empty(0) if t is None else t.clone()


def _last(cache, layer_idx, who):
    sp = _armed(cache, who)
    last = sp.last.get(layer_idx)
    return (None, None) if last is None else (sp.ws[layer_idx], last)


def sparse_bounds(cache, layer_idx: int) -> torch.Tensor:
    """A copy [Hkv, pages] fp32 of ub of the layer's last routed call; empty before one."""
    ws, last = _last(cache, layer_idx, "sparse_bounds")
    if ws is None:
        return torch.empty(0, dtype=torch.float32)
    Hkv, pages, _ = last
    return ws[:Hkv * pages * 4].view(torch.float32).view(Hkv, pages).clone()


def sparse_pages(cache, layer_idx: int) -> torch.Tensor:
    """A copy [Hkv, keep_pages] int32 of the page lists of the layer's last routed call, ascending per kv head; empty before
    one."""
    ws, last = _last(cache, layer_idx, "sparse_pages")
    if ws is None:
        return torch.empty(0, dtype=torch.int32)
    Hkv, pages, keep = last
    at = (Hkv * pages * 4 + 15) // 16 * 16
    return ws[at:at + Hkv * keep * 4].view(torch.int32).view(Hkv, keep).clone()

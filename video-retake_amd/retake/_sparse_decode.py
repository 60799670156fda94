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

Several new tokens: `sparse_decode(cache, keep_rows, wide=True)` also routes a call with 16 < (Hq / Hkv) * Lq <= 64 packed
rows - the verification call of assisted generation (num_assistant_tokens + 1 rows), a few-token continuation, a short
follow-up after `rewind(video_end)` - as ONE rtk_attention_decode_sparse_wide call, under the narrow route's other
conditions; it counts in `sparse_attention_calls` and in `sparse_wide_calls(cache)`.  The key is its own opt-in (it does
not need `multi_token_attention`; without it every call goes exactly where it went, bit for bit) and serves every G the
library serves.  The rule: ALL Lq rows of the call share ONE list per kv head.  ub[g, p] above is the max over the packed
rows of EVERY position, so a page that any one draft row needs is ranked by that row - and a verification call's output is
not what Lq one-token sparse calls, each with a list of its own, would give.  What that does to answer quality and to
draft acceptance has not been evaluated (there are no weights here).  `crop()` of rows behind `video_end` (a rejected
draft) and `rewind(video_end)` leave the index armed and valid: no new summary call.

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
kv_cache_dtype), a branch, a focused cache, defer_rerotation, an fp32 model, head_dim != 128, archive=True together with wide=True.  Not built: the wide kernel over the fp8 archive, branches, the sharded path, incremental index updates
while the video grows (a chunk after arming makes the next routed call raise: arm again)."""
import torch

from . import _native as nv
from ._cache_state import _on_device

PAGE = nv.PAGE_ROWS
NARROW_ROWS = 16   # packed rows of the narrow kernel (DEC_R): a call with more takes the wide entry points


class _Sparse:
    """An armed route: keep_rows, the `video_end` recorded at arming, and per layer the summaries [Hkv, pages, 2, D], the
    geometry (first, ve, pages) and the workspace of the layer's last routed call (ub | lists | partials).  `archive`: the
    pages are the fp8 archive's; the geometry is then (16-bit rows at `video_end`, len8 at `video_end`, pages).  `wide`: calls
    of 17 to 64 packed rows are routed too; `wide_calls` counts them."""

    __slots__ = ("keep_rows", "mark", "summ", "geom", "ws", "last", "archive", "wide", "wide_calls")

    def __init__(self, keep_rows, mark, archive=False, wide=False):
        self.keep_rows, self.mark, self.summ, self.geom, self.ws, self.last = keep_rows, mark, {}, {}, {}, {}
        self.archive, self.wide, self.wide_calls = archive, wide, 0


class _Rows16:
    """The kind archive=False: the region is rows [pinned, length at `video_end`) of the layer's 16-bit buffers."""
    Unit, summary = nv.PageSummaryUnit, "rtk_pivotkv_page_summary_batched"
    query, call = "rtk_attention_decode_sparse_workspace_bytes", "rtk_attention_decode_sparse"
    wide_query, wide_call = "rtk_attention_decode_sparse_wide_workspace_bytes", "rtk_attention_decode_sparse_wide"
    none = "no layer holds video rows behind its pinned rows"

    @staticmethod
    def region(st, m):
        """(region rows, geometry without the pages) at arming; None: a layer without video rows"""
        first, n = st.pinned, m.length - st.pinned
        return None if first < 0 or n < 1 else (n, (first, m.length))

    own = staticmethod(lambda st: True)   # the layout of the buffers only this kind reads

    @staticmethod
    def fill(u, st, geom, n):
        u.k, u.k_stride_h, u.first, u.n = st._k.data_ptr(), st._k.stride(1), geom[0], n

    rows16 = staticmethod(lambda geom: geom[1])          # the 16-bit rows at `video_end`
    views = staticmethod(lambda st, geom: True)          # what a routed call's layer must still hold
    before = staticmethod(lambda geom: 0)                # the rows query_offset counts before k's
    least = staticmethod(lambda geom: geom[1] - 1)       # the q_offset from which every query row sees the region whole
    region_args = staticmethod(lambda geom: geom[:2])    # of the workspace query, behind Lk
    archive_args = staticmethod(lambda st, geom: ())     # of the call, behind the kv strides
    tail_args = region_args                              # of the call, behind scale


class _Archive8:
    """The kind archive=True: the region is the fp8 archive as recorded at `video_end`, from archive row 0."""
    Unit, summary = nv.PageSummaryFp8kUnit, "rtk_pivotkv_page_summary_fp8k_batched"
    query, call = "rtk_attention_decode_sparse_fp8kv_workspace_bytes", "rtk_attention_decode_sparse_fp8kv"
    none = "no layer holds archived video rows"

    @staticmethod
    def region(st, m):
        return None if st.k8 is None or m.len8 < 1 or st.len8 < m.len8 else (m.len8, (m.length, m.len8))

    @staticmethod
    def own(st):
        k, k8, ks8 = st._k, st.k8, st.ks8
        return k8.stride(3) == 1 and k8.stride(2) == k8.shape[3] and ks8.stride(2) == 1 and k8.shape[1] == k.shape[1] \
            and k8.shape[3] == k.shape[3]

    @staticmethod
    def fill(u, st, geom, n):
        u.k8, u.k8_stride_h, u.k_scale, u.scale_stride_h = st.k8.data_ptr(), st.k8.stride(1), st.ks8.data_ptr(), st.ks8.stride(1)
        u.n = n

    rows16 = staticmethod(lambda geom: geom[0])
    views = staticmethod(lambda st, geom: st.len8 == geom[1])
    before = staticmethod(lambda geom: geom[1])          # query_offset counts over archive + views; q_offset in 16-bit rows
    least = staticmethod(lambda geom: 0)                 # every archive row is visible to every query row
    region_args = staticmethod(lambda geom: geom[1:2])
    archive_args = staticmethod(lambda st, geom: (nv.ptr(st.k8), nv.ptr(st.v8), nv.ptr(st.ks8), nv.ptr(st.vs8), geom[1],
                                                  st.k8.stride(1), st.ks8.stride(1)))
    tail_args = staticmethod(lambda geom: ())


def _is_int(x, least):
    return isinstance(x, int) and not isinstance(x, bool) and x >= least


def _mark_moved(cache, mark) -> bool:
    ve = cache.video_end
    return ve is None or ve.serial != mark.serial or cache._mark_is_dead(ve.serial) or ve.epoch != cache._epoch \
        or cache._flushes != ve.flushes or cache._compressed_in_forward or len(cache._layers) != ve.n_layers


def _check_mark(cache, mark, who, then):
    if _mark_moved(cache, mark):
        raise ValueError(f"{who}: {then}")


def sparse_decode(cache, keep_rows: int = 8192, archive: bool = False, wide: bool = False) -> None:
    """Arm the page-sparse decode route (see the module docstring).  ValueError, before any launch: keep_rows not an int
    >= 1 (a bool is not an int), archive or wide not a bool, archive=True together with wide=True (the wide paged kernel
    over the fp8 archive is not built), a cache without `video_end`, attention_kernel other than "hip",
    kv_cache_dtype set without archive=True (the pages of an fp8 cache are its archive's: an opt-in of its own), archive=True
    on a cache without kv_cache_dtype.  NotImplementedError: a branch, a focused cache, defer_rerotation, an fp32 model or
    head_dim other than 128.  Arming again rebuilds the index: ONE summary call of the kind per device."""
    who = "sparse_decode"
    if not _is_int(keep_rows, 1):
        raise ValueError(f"{who}: keep_rows must be an int >= 1, got {keep_rows!r}")
    if not isinstance(archive, bool):
        raise ValueError(f"{who}: archive must be a bool, got {archive!r}")
    if not isinstance(wide, bool):
        raise ValueError(f"{who}: wide must be a bool, got {wide!r}")
    if archive and wide:
        raise ValueError(f"{who}: archive=True together with wide=True is not served - the wide paged kernel over the fp8 "
                         "archive is not built")
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
    _check_mark(cache, ve, who, "`video_end` does not describe the cache's rows any more (a chunk, a slide, an eviction or a "
                "rewind below it since) - finish the prefill first")
    kind = _Archive8 if archive else _Rows16
    by_device = {}
    for l, (st, m) in enumerate(zip(cache._layers, ve.layers)):
        k = st._k
        region = None if k is None or not m.has_kv else kind.region(st, m)
        if region is None:
            continue   # a layer without rows to index: its calls take the existing routes
        if k.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"{who} needs a bfloat16 or float16 model, got {k.dtype} in layer {l}")
        if k.shape[3] != 128:
            raise NotImplementedError(f"{who} needs head_dim 128, got {k.shape[3]} in layer {l}")
        if st.c.cap == 0 or k.stride(3) != 1 or k.stride(2) != k.shape[3] or not kind.own(st):
            raise ValueError(f"{who}: layer {l}'s buffers are not the cache's own dense blocks")
        by_device.setdefault(k.get_device(), []).append((l, st) + region)
    if not by_device:
        raise ValueError(f"{who}: {kind.none}")
    sp = _Sparse(keep_rows, ve, archive, wide)
    for dev, ps in by_device.items():
        units = (kind.Unit * len(ps))()
        k0 = ps[0][1]._k
        for u, (l, st, n, geom) in zip(units, ps):
            k = st._k
            if k.shape[1] != k0.shape[1] or k.dtype != k0.dtype:
                raise ValueError(f"{who}: layer {l} differs from layer {ps[0][0]} in kv heads or dtype")
            pages = (n + PAGE - 1) // PAGE
            s = sp.summ[l] = torch.empty((k.shape[1], pages, 2, k.shape[3]), dtype=k.dtype, device=k.device)
            sp.geom[l] = geom + (pages,)
            kind.fill(u, st, geom, n)
            u.summ, u.summ_stride_h = s.data_ptr(), s.stride(0)
        nv.check(_on_device(dev, getattr(nv.lib, kind.summary), units, len(ps), k0.shape[1], k0.shape[3], nv.dtype_code(k0),
                            nv.raw_stream(dev)), kind.summary)
        cache.page_summary_calls += 1
    cache._sparse = sp


def dense_decode(cache) -> None:
    """Disarm the route and free the index and its workspaces; every call takes the existing routes again."""
    cache._sparse = None


def sparse_wide_calls(cache) -> int:
    """The routed calls of more than 16 packed rows since arming (each also counts in `sparse_attention_calls`);
    ValueError while not armed."""
    return _armed(cache, "sparse_wide_calls").wide_calls


def sparse_bytes(cache) -> dict:
    sp = cache._sparse
    nb = lambda ts: sum(t.numel() * t.element_size() for t in ts)   # noqa: E731
    return {"page_summaries": nb(sp.summ.values()), "sparse_workspace": nb(sp.ws.values())}


def route(cache, q, k, v, scaling, query_offset, layer_idx):
    """What PivotKVCache.attention asks first while armed: the sparse call's output [1, Lq, Hq, D], or None - take the
    existing routes.  ValueError for a call without layer_idx and for a `video_end` that is no longer the recorded one.
    On an fp8 cache k / v are the layer's 16-bit views and the archive precedes them; query_offset counts over archive +
    views, as PivotKVCache.attention states."""
    sp = cache._sparse
    who = "PivotKVCache.attention (sparse_decode armed)"
    if layer_idx is None:
        raise ValueError(f"{who} needs layer_idx: the route reads the layer's pinned rows and `video_end`")
    geom = sp.geom.get(layer_idx)
    if geom is None or q.dim() != 4 or k.dim() != 4 or q.shape[0] != 1:
        return None
    kind = _Archive8 if sp.archive else _Rows16
    pages = geom[2]
    _, Hq, Lq, D = q.shape
    _, Hkv, Lk, _ = k.shape
    if Lk <= kind.rows16(geom):   # no row behind `video_end`
        return None
    _check_mark(cache, sp.mark, who, "`video_end` is no longer the mark recorded by sparse_decode - a chunk, a slide, an "
                "eviction or a rewind below it happened since, and the page index no longer describes the rows.  Call "
                "sparse_decode again (or dense_decode)")
    st, summ = cache._layers[layer_idx], sp.summ[layer_idx]
    if not kind.views(st, geom) or k.data_ptr() != st._k.data_ptr() or v.data_ptr() != st._v.data_ptr() or k.stride() != v.stride() \
            or k.stride(3) != 1 or q.stride(3) != 1 or not (q.dtype == k.dtype == v.dtype == summ.dtype) or Hkv != summ.shape[0] \
            or D != summ.shape[3] or Hq % Hkv:
        return None
    q_off = Lk - Lq if query_offset is None else int(query_offset) - kind.before(geom)
    if q_off < kind.least(geom) or q_off < Lk - Lq:
        return None
    keep_pages = min((sp.keep_rows + PAGE - 1) // PAGE, pages)
    code = nv.dtype_code(q)
    wide = sp.wide and (Hq // Hkv) * Lq > NARROW_ROWS
    query, call = (kind.wide_query, kind.wide_call) if wide else (kind.query, kind.call)
    need = getattr(nv.lib, query)(Hq, Hkv, Lq, Lk, *kind.region_args(geom), keep_pages, D, code)
    if not need:
        return None   # outside the packed envelope: the existing routes
    ws = sp.ws.get(layer_idx)
    if ws is None or ws.numel() < need:
        ws = sp.ws[layer_idx] = torch.empty(need, dtype=torch.uint8, device=q.device)
    out = torch.empty((1, Lq, Hq, D), dtype=q.dtype, device=q.device)
    scale = float(D) ** -0.5 if scaling is None else float(scaling)
    rc = getattr(nv.lib, call)(nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2),
                                    *kind.archive_args(st, geom), nv.ptr(out), Hq, Hkv, Lq, Lk, q_off, D, code, scale,
                                    *kind.tail_args(geom), nv.ptr(summ), summ.stride(0), keep_pages, nv.ptr(ws), ws.numel(),
                                    nv.raw_stream(q.device.index))
    if rc == nv.RTK_EUNSUPPORTED:
        return None
    nv.check(rc, call)
    sp.last[layer_idx] = (Hkv, pages, keep_pages)
    cache.sparse_attention_calls += 1
    sp.wide_calls += wide
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

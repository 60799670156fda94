"""The native attention front end, in place of what the reference hands to torch / flash_attn (qwen2_vl.py:88-117,
:188-219, :303-358; llava_onevision.py:118-139): `chunk_attention` (one HIP launch over [compressed prefix | chunk]), the
fp8 row helpers, and `native_attention`, the patches' switch, which derives the causal offset from HF's mask.  A cache is
reached through `cache.attention` / `cache.archive_len` only."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as nv


def chunk_attention(query_states, key_states, value_states, scaling=None, workspace=None, query_offset=None, archive=None,
                    packed_gqa=False, route=None, shared=None, packed_wide=False):
    """Attention of a chunk's queries over [compressed prefix | current chunk] in one HIP launch (rtk_attention_forward):
    what the reference's attention patches hand to torch / flash_attn after the cache update (qwen2_vl.py:88-117,
    :188-219, :303-358; llava_onevision.py:118-139).

    query_states [1, Hq, Lq, D], key_states / value_states [1, Hkv, Lk, D] with a contiguous head_dim and any head / row
    strides - they are read where they are (the transposed projection output, the `[:P0 + L]` view of the cache buffer):
    no repeat_kv, no .contiguous(), no mask.  One unpadded sequence; query row i sees keys j <= query_offset + i.  The
    default, Lk - Lq, is bottom-right causal: the queries are the last Lq of the Lk positions (what flash-attn computes).  A
    larger offset restates the 4-D additive mask HF builds over the UNCOMPRESSED positions, which the patches slice to the
    keys the compressed cache holds: its width T gives query_offset = T - Lq (see native_attention).  Returns [1, Lq, Hq, D] (contiguous: `reshape(1, Lq, -1)` feeds o_proj), or None - nothing was
    touched, take the existing route - when the library declines the shape (RTK_EUNSUPPORTED).

    workspace: optional dict the key-split scratch is kept in between calls (PivotKVCache.attention passes its own).

    archive: optional (k8, v8, k_scale, v_scale) - e4m3 codes uint8 [1, Hkv, L8, D] and fp32 scales [1, Hkv, L8] of rows that
    PRECEDE key_states / value_states in the sequence (kv_cache_dtype="fp8_e4m3"; rtk_attention_forward_fp8kv, bf16 / fp16
    with head_dim 128 only).  Every query row sees all of them; query_offset then counts over the L8 + Lk keys (default
    L8 + Lk - Lq).

    packed_gqa: try the GQA-packed few-row kernel first (rtk_attention_decode, or rtk_attention_decode_fp8kv with an
    archive: bf16 / fp16, head_dim 128, (Hq / Hkv) * Lq <= 16).  A shape it declines (RTK_EUNSUPPORTED) takes the call above
    in this same invocation, so it returns the bits the default returns.  Its partials are kept in `workspace` under a key
    of their own.  route: optional list; the call appends "packed" or "chunk", whichever kernel produced the result.

    shared: optional (ks, vs) - rows [1, Hkv, Ls, D] of the same dtype that live in ANOTHER buffer (their own head / row
    strides, contiguous head_dim) and precede key_states / value_states in the sequence, after the archive: the keys are
    [archive | shared | key_states] (rtk_attention_forward_shared / rtk_attention_decode_shared, bf16 / fp16 with head_dim
    128 only; a branch of PivotKVCache.fork reads its parent's rows this way).  Every query row sees all of them;
    query_offset counts over the L8 + Ls + Lk keys.  Combines with archive= and packed_gqa= as above.

    packed_wide: after the packed kernel and before the chunk kernel, try the wide packed kernel (rtk_attention_decode_wide,
    _wide_fp8kv, _wide_shared: bf16 / fp16, head_dim 128, (Hq / Hkv) * Lq <= 64 - the verification step of assisted
    generation, a few-token continuation).  A shape it declines takes the chunk kernel as above; `route` receives "wide".
    True asks for the kernel wherever the library serves it; the cache passes wide_dispatch(...), the shapes at which it
    measured faster than the chunk kernel.
    Its bits are neither the chunk kernel's nor those of Lq one-row packed calls: the fp32 sums are grouped differently."""
    nv.require_device(query_states, key_states, value_states)
    if query_states.dim() != 4 or key_states.dim() != 4 or value_states.dim() != 4 or query_states.shape[0] != 1:
        raise ValueError("chunk_attention takes [1, H, L, D] tensors (one unpadded sequence)")
    if key_states.shape != value_states.shape or key_states.stride() != value_states.stride():
        raise ValueError("key_states and value_states must share shape and strides")
    if not (query_states.dtype == key_states.dtype == value_states.dtype):
        raise ValueError("query, key and value states must share a dtype")
    _, Hq, Lq, D = query_states.shape
    _, Hkv, Lk, Dk = key_states.shape
    if Dk != D:
        raise ValueError("query and key head_dim differ")
    if query_states.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return None
    if query_states.stride(3) != 1 or key_states.stride(3) != 1:
        return None
    code = nv.dtype_code(query_states)
    scale = float(D) ** -0.5 if scaling is None else float(scaling)
    a8 = _check_archive(archive, Hkv, D) if archive is not None else (None, None, None, None, 0, 0, 0)
    L8 = a8[4]
    s16 = _check_shared(shared, Hkv, D, key_states.dtype, "key_states") if shared is not None else (None, None, 0, 0, 0)
    if s16 is None:
        return None
    Ls = s16[2]
    q_off = L8 + Ls + Lk - Lq if query_offset is None else int(query_offset)
    stream = nv.raw_stream(query_states.device.index)
    out = torch.empty((1, Lq, Hq, D), dtype=query_states.dtype, device=query_states.device)
    qkv = (nv.ptr(query_states), query_states.stride(1), query_states.stride(2), nv.ptr(key_states), nv.ptr(value_states),
           key_states.stride(1), key_states.stride(2))
    if shared is not None:    # (no shared rows included: the library then runs the two-segment call itself)
        qkv += s16 + a8
        shape = (Hq, Hkv, Lq, Lk, L8, Ls, D, code)
        sfx = "_shared"
    elif archive is not None:   # (an empty archive included: the library then runs the 16-bit call itself)
        qkv += a8
        shape = (Hq, Hkv, Lq, Lk, L8, D, code)
        sfx = "_fp8kv"
    else:
        shape = (Hq, Hkv, Lq, Lk, D, code)
        sfx = ""
    routes = (("packed", "rtk_attention_decode", "rtk_attention_decode_workspace_bytes", "attention_decode_ws"),) \
        if packed_gqa else ()
    if packed_wide:
        routes += (("wide", "rtk_attention_decode_wide", "rtk_attention_decode_wide_workspace_bytes", "attention_decode_ws"),)
    for tag, fn, query, ws_tag in routes + (("chunk", "rtk_attention_forward", "rtk_attention_workspace_bytes", "attention_ws"),):
        need = getattr(nv.lib, query + sfx)(*shape)
        ws = _scratch(workspace, ws_tag, query_states.device, stream, need)
        rc = getattr(nv.lib, fn + sfx)(*qkv, nv.ptr(out), Hq, Hkv, Lq, Lk, q_off - L8 - Ls, D, code, scale, nv.ptr(ws), need, stream)
        if rc == nv.RTK_EUNSUPPORTED:
            continue
        nv.check(rc, fn + sfx)
        if route is not None:
            route.append(tag)
        return out
    return None


WIDE_DISPATCH_GROUPS = (4, 8)   # Hq / Hkv, inclusive: where the wide packed call measured faster than the chunk-kernel call


def wide_dispatch(Hq: int, Hkv: int, Lq: int) -> bool:
    """Whether multi_token_attention="packed" (PivotKVCache.attention) sends a call of this shape to the wide packed kernel:
    inside its envelope, 16 < (Hq / Hkv) * Lq <= 64, AND at a geometry where the call measured faster than the chunk-kernel
    call it replaces (tools/bench_attention.py --wide, profiles/wide_decode_bench.json): 4 <= Hq / Hkv <= 8.  What the chunk
    kernel pays there is one pass over the keys per query head of a kv head; at Hq / Hkv = 1 and 2 there is little to save
    and the wide call measured 0.95-0.99x and 0.72x, at Hq 16 / Hkv 1 0.44x.  The C entry points serve those shapes all the
    same, and so does chunk_attention(packed_wide=True), which asks for them explicitly."""
    G = Hq // max(Hkv, 1)
    return WIDE_DISPATCH_GROUPS[0] <= G <= WIDE_DISPATCH_GROUPS[1] and 16 < G * Lq <= 64


def _check_archive(archive, Hkv, D):
    k8, v8, ks8, vs8 = archive
    nv.require_device(k8, v8, ks8, vs8)
    if k8.dtype != torch.uint8 or v8.dtype != torch.uint8 or ks8.dtype != torch.float32 or vs8.dtype != torch.float32:
        raise ValueError("archive = (codes uint8, codes uint8, scales float32, scales float32)")
    if k8.dim() != 4 or k8.shape[:2] != (1, Hkv) or k8.shape[3] != D or v8.shape != k8.shape or v8.stride() != k8.stride() \
            or ks8.shape != k8.shape[:3] or vs8.shape != ks8.shape or vs8.stride() != ks8.stride():
        raise ValueError("archive codes must be [1, Hkv, L8, D] and scales [1, Hkv, L8], K and V laid out alike")
    if k8.stride(3) != 1 or k8.stride(2) != D or ks8.stride(2) != 1:
        raise ValueError("archive rows must be dense (D codes per row, one scale per row)")
    return (nv.ptr(k8), nv.ptr(v8), nv.ptr(ks8), nv.ptr(vs8), k8.shape[2], k8.stride(1), ks8.stride(1))


def _check_shared(shared, Hkv, D, dtype, whose):
    """(ks, vs) -> the library's (ks, vs, Ls, stride_h, stride_l), or None: rows it does not take (decline the call).
    whose: what `dtype` is the dtype of, for the message."""
    ks, vs = shared
    nv.require_device(ks, vs)
    if ks.dim() != 4 or ks.shape[:2] != (1, Hkv) or ks.shape[3] != D or vs.shape != ks.shape or vs.stride() != ks.stride():
        raise ValueError("shared keys / values must be [1, Hkv, Ls, D], laid out alike")
    if ks.dtype != dtype or vs.dtype != dtype:
        raise ValueError(f"shared keys / values must have the dtype of {whose}")
    if ks.stride(3) != 1:
        return None
    return (nv.ptr(ks), nv.ptr(vs), ks.shape[2], ks.stride(1), ks.stride(2))


def _scratch(workspace, tag, device, stream, need):
    """`need` bytes of scratch, kept in the dict `workspace` (if any) under (tag, device, stream) - per stream: calls on two
    streams may overlap.  None for need 0."""
    if not need:
        return None
    key = (tag, device.index, stream)
    ws = None if workspace is None else workspace.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        if workspace is not None:
            workspace[key] = ws
    return ws


def group_decode_attention(queries, owns, shared, archive, scaling=None, workspace=None):
    """ONE new token of each of B sequences that share [archive | shared] and differ in their own rows, in one HIP launch
    that reads every archive and shared row once (rtk_attention_decode_group): the decode step of B forks of one
    PivotKVCache (retake/branch_group.py).

    queries: B tensors [1, Hq, 1, D]; owns: B pairs (k, v) of views [1, Hkv, Lk_b, D] - branch b's OWN rows, the new
    token's included, any head / row strides, contiguous head_dim; shared: (ks, vs) [1, Hkv, Ls, D] or None; archive:
    (k8, v8, k_scale, v_scale) as chunk_attention takes it, or None.  Branch b's query sees every archive row, every shared
    row and every one of its own rows.  Returns [B, 1, Hq, D]; row b's bits depend neither on the other branches nor on
    b's place among them.  None - nothing was touched - when the library declines the call (RTK_EUNSUPPORTED: more than 8
    branches or B * Hq / Hkv > 32 packed rows, float32, head_dim other than 128, a layout it does not take).

    workspace: optional dict the partials are kept in between calls."""
    B = len(queries)
    if B < 1 or len(owns) != B:
        raise ValueError("group_decode_attention takes one query and one (k, v) pair per branch, at least one branch")
    q0, k0 = queries[0], owns[0][0]
    if q0.dim() != 4 or k0.dim() != 4:
        raise ValueError("group_decode_attention takes [1, Hq, 1, D] queries and [1, Hkv, Lk, D] keys / values")
    _, Hq, _, D = q0.shape
    Hkv = k0.shape[1]
    for q, (k, v) in zip(queries, owns):
        nv.require_device(q, k, v)
        if q.shape != (1, Hq, 1, D) or k.dim() != 4 or k.shape[:2] != (1, Hkv) or k.shape[3] != D:
            raise ValueError("group_decode_attention takes [1, Hq, 1, D] queries and [1, Hkv, Lk, D] keys / values")
        if k.shape != v.shape or k.stride() != v.stride():
            raise ValueError("a branch's keys and values must share shape and strides")
        if k.shape[2] < 1:
            raise ValueError("every branch needs own rows: at least the new token's")
        if not (q.dtype == k.dtype == v.dtype == q0.dtype) or q.device != q0.device:
            raise ValueError("queries, keys and values must share a dtype and a device")
    if q0.dtype not in (torch.bfloat16, torch.float16) or any(q.stride(3) != 1 or k.stride(3) != 1 for q, (k, _) in zip(queries, owns)):
        return None
    code = nv.dtype_code(q0)
    scale = float(D) ** -0.5 if scaling is None else float(scaling)
    a8 = _check_archive(archive, Hkv, D) if archive is not None else (None, None, None, None, 0, 0, 0)
    s16 = _check_shared(shared, Hkv, D, q0.dtype, "the queries") if shared is not None else (None, None, 0, 0, 0)
    if s16 is None:
        return None
    if B > nv.DECODE_GROUP_MAX:   # (the library says so itself, but its array holds no more)
        return None
    brs = (nv.DecodeBranch * B)()
    rows = (nv.C.c_int * B)()
    for b, (q, (k, v)) in enumerate(zip(queries, owns)):
        br = brs[b]
        br.q, br.q_stride_h = q.data_ptr(), q.stride(1)
        br.k, br.v, br.kv_stride_h, br.kv_stride_l, br.Lk = k.data_ptr(), v.data_ptr(), k.stride(1), k.stride(2), k.shape[2]
        rows[b] = k.shape[2]
    need = nv.lib.rtk_attention_decode_group_workspace_bytes(rows, B, Hq, Hkv, a8[4], s16[2], D, code)
    stream = nv.raw_stream(q0.device.index)
    ws = _scratch(workspace, "attention_group_ws", q0.device, stream, need)
    out = torch.empty((B, 1, Hq, D), dtype=q0.dtype, device=q0.device)
    rc = nv.lib.rtk_attention_decode_group(brs, B, *s16, *a8, nv.ptr(out), Hq, Hkv, D, code, scale, nv.ptr(ws), need, stream)
    if rc == nv.RTK_EUNSUPPORTED:
        return None
    nv.check(rc, "rtk_attention_decode_group")
    return out


def fp8_quantize_rows(x: torch.Tensor):
    """x [1, Hkv, L, 128] (bf16 / fp16, dense rows, any head stride) -> (codes uint8 [1, Hkv, L, 128], scales fp32
    [1, Hkv, L]) by the rule of include/retake_hip.h "FP8 rows of the compressed cache", on the device
    (rtk_pivotkv_archive_batched in copy mode with the identity selection).  Tools and diagnostics; the cache's flush
    fills its archive with the same kernel."""
    nv.require_device(x)
    if x.dim() != 4 or x.shape[0] != 1 or x.stride(3) != 1 or x.stride(2) != x.shape[3]:
        raise ValueError("fp8_quantize_rows takes [1, Hkv, L, D] with dense rows")
    _, H, L, D = x.shape
    codes = torch.empty((1, H, L, D), dtype=torch.uint8, device=x.device)
    scales = torch.empty((1, H, L), dtype=torch.float32, device=x.device)
    if L == 0:
        return codes, scales
    dummy_c, dummy_s = torch.empty_like(codes), torch.empty_like(scales)   # (the kernel archives a K and a V per unit)
    units = (nv.ArchiveUnit * 1)()
    u = units[0]
    u.k_src, u.k_src_stride_h, u.v_src, u.v_src_stride_h = x.data_ptr(), x.stride(1), x.data_ptr(), x.stride(1)
    u.k8, u.v8, u.dst_stride_h = codes.data_ptr(), dummy_c.data_ptr(), L * D
    u.k_scale, u.v_scale, u.scale_stride_h = scales.data_ptr(), dummy_s.data_ptr(), L
    with torch.cuda.device(x.device):
        nv.check(nv.lib.rtk_pivotkv_archive_batched(units, 1, H, D, L, 0, nv.dtype_code(x), nv.COMPACT_K_COPY, None, 1.0, None, 0,
                                                    nv.round_mode(x.dtype), nv.stream()), "rtk_pivotkv_archive_batched")
    return codes, scales


def fp8_dequantize_rows(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None):
    """codes uint8 [1, Hkv, L, 128] + scales fp32 [1, Hkv, L] (dense rows, any head stride) -> [1, Hkv, L, 128] of `dtype`
    (rtk_fp8kv_dequant), written into `out` (dense rows, any head stride) when given."""
    nv.require_device(codes, scales)
    _, H, L, D = codes.shape
    if out is None:
        out = torch.empty((1, H, L, D), dtype=dtype, device=codes.device)
    if L:
        with torch.cuda.device(codes.device):
            nv.check(nv.lib.rtk_fp8kv_dequant(nv.ptr(codes), codes.stride(1), nv.ptr(scales), scales.stride(1), nv.ptr(out),
                                              out.stride(1), H, L, D, nv.dtype_code(out), nv.stream()), "rtk_fp8kv_dequant")
    return out


def native_attention(module, cache, query_states, key_states, value_states, attention_mask, *, output_attentions=False,
                     scaling=None):
    """What the attention patches call after the prologue / cache update: the chunk's attention through `cache.attention`
    iff the cache was built with attention_kernel="hip", the batch is one sequence on the GPU, no dropout is active, no
    attention weights are wanted and the layer has no active sliding window.  [1, Lq, Hq, D], or None = take the patch's
    existing route (nothing was touched).

    attention_mask: the patch's additive mask [1, 1, Lq, T >= Lk], or "causal" for the flash-attn patch (no mask operand,
    bottom-right causal).  The mask's VALUES are not read: the switch asserts one unpadded sequence - the only case the
    reference supports (`assert bsz == 1`, longvideo_cache.py:246) - whose HF mask is 0 where j <= (T - Lq) + i and -inf
    elsewhere (every recorded mask is: tests/test_attention_cpu.py).  Its WIDTH is: HF builds it over the uncompressed
    positions and the patches slice it to the keys of the compressed cache, so row i sees keys j <= (T - Lq) + i, which for
    T > Lk is more than bottom-right causal over the Lk keys - the native route returns what the patch's own route would.
    A missing or differently shaped mask means something else on each patch's route: that call is declined."""
    if getattr(cache, "attention_kernel", None) != "hip":
        return None
    fp8 = getattr(cache, "kv_cache_dtype", None) is not None
    branch = getattr(cache, "forked_from", None) is not None

    def decline(why):
        # with fp8 rows the patch's own route would read the 16-bit rows only and silently miss the archive
        if fp8:
            raise NotImplementedError(f"kv_cache_dtype={cache.kv_cache_dtype!r}: the native chunk attention is the only "
                                      f"route that reads the fp8 rows, and it does not serve this call: {why}")
        if branch:   # likewise the rows a branch shares with its parent
            raise NotImplementedError("a branch (PivotKVCache.fork): the native chunk attention is the only route that reads "
                                      f"the parent's rows, and it does not serve this call: {why}")
        return None

    if output_attentions:
        return decline("attention weights are wanted (output_attentions)")
    if query_states.shape[0] != 1 or not query_states.is_cuda:
        return decline("a padded batch or CPU tensors (one unpadded sequence on the GPU only)")
    if module.training and getattr(module, "attention_dropout", 0.0):
        return decline("attention dropout is active")
    cfg = getattr(module, "config", None)
    if (getattr(cfg, "use_sliding_window", False) and getattr(cfg, "sliding_window", None) is not None
            and module.layer_idx >= getattr(cfg, "max_window_layers", 0)):
        return decline("the layer has an active sliding window")
    layer_idx = getattr(module, "layer_idx", None)
    Lq = query_states.shape[2]
    Lk = key_states.shape[2] + (cache.archive_len(layer_idx) if fp8 else 0) \
        + (cache.shared_len(layer_idx) if branch else 0)   # keys of the whole sequence
    if isinstance(attention_mask, str):
        if attention_mask != "causal":
            return decline(f"attention mask {attention_mask!r}")
        offset = Lk - Lq
    else:
        if attention_mask is None or attention_mask.dim() != 4 or tuple(attention_mask.shape[:3]) != (1, 1, Lq) \
                or attention_mask.shape[3] < Lk:
            return decline("a missing attention mask, or one that is not [1, 1, Lq, T >= Lk] (a padded batch)")
        offset = attention_mask.shape[3] - Lq
    return cache.attention(query_states, key_states, value_states, scaling=scaling, query_offset=offset, layer_idx=layer_idx)


ATTENTION_KERNELS = (None, "hip")
KV_CACHE_DTYPES = (None, "fp8_e4m3")

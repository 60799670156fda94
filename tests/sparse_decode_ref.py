"""The page-sparse decode rule (include/retake_hip.h "Page-sparse decode"; retake/_sparse_decode.py) in numpy / float64
torch: summaries and selection exact, bound and attention in float64.  Tensors come in as they lie on any device; everything
is computed on the CPU.  Below the rule: what the GPU tests of the paged calls and of the armed cache share."""
import numpy as np
import torch

PAGE = 32


def pages_of(n):
    return -(-n // PAGE)


def _ord16(x):
    """The order-preserving integer key of a sign-magnitude 16-bit float (bf16 / fp16 bits as int64 in [0, 65536))."""
    return np.where(x & 0x8000, x ^ 0xffff, x ^ 0x8000)


def summaries(K, first, n):
    """K [Hkv, L, D] (bf16 / fp16) -> [Hkv, pages, 2, D] of K's dtype: max and min over the existing rows of each page of
    rows [first, first + n), exact - on the ordered bit patterns, so of -0 and +0 the max is +0 and the min -0."""
    bits = K[:, first:first + n].cpu().contiguous().view(torch.int16).numpy().astype(np.int64) & 0xffff
    key = _ord16(bits)
    Hkv, _, D = key.shape
    out = np.empty((Hkv, pages_of(n), 2, D), dtype=np.int64)
    for p in range(pages_of(n)):
        rows = key[:, PAGE * p:min(PAGE * p + PAGE, n)]
        out[:, p, 0], out[:, p, 1] = rows.max(axis=1), rows.min(axis=1)
    back = np.where(out & 0x8000, out ^ 0x8000, out ^ 0xffff)   # the inverse of _ord16
    return torch.from_numpy(back.astype(np.uint16).view(np.int16)).view(K.dtype)


def bound_terms(q, summ):
    """q [Hq, Lq, D], summ [Hkv, pages, 2, D] -> float64 terms [Hkv, R, pages, D], R = G Lq packed rows (hh, i):
    max(q kmax, q kmin) per channel."""
    Hq, Lq, D = q.shape
    Hkv = summ.shape[0]
    qq = q.double().cpu().view(Hkv, (Hq // Hkv) * Lq, 1, D)
    s = summ.double().cpu()
    return torch.maximum(qq * s[:, None, :, 0], qq * s[:, None, :, 1])


def bound(q, summ):
    """(ub float64 [Hkv, pages], bar [Hkv, pages]): the bound, and the derived bar of an fp32 sum of the 128 exact products in
    any order - 128 * 2^-24 * sum_d |term_d|, the largest over the packed rows."""
    t = bound_terms(q, summ)
    return t.sum(-1).max(dim=1).values, 128 * 2.0 ** -24 * t.abs().sum(-1).max(dim=1).values


def select(ub, keep_pages):
    """ub [Hkv, pages] (the DEVICE's fp32 values, for an exact comparison) -> int32 [Hkv, keep_pages]: the last page always,
    of the others the keep_pages - 1 with the highest ub, ties to the lowest index, ascending."""
    ub = ub.detach().cpu().float().numpy()
    Hkv, pages = ub.shape
    out = np.empty((Hkv, keep_pages), dtype=np.int32)
    for g in range(Hkv):
        order = np.argsort(-ub[g, :pages - 1].astype(np.float64), kind="stable")[:keep_pages - 1]
        out[g] = np.sort(np.concatenate([order, [pages - 1]]))
    return torch.from_numpy(out)


def gathered_rows(first, ve, Lk, lst):
    """Physical row numbers of [rows [0, first) | the existing rows of pages lst[0], lst[1], .. | rows [ve, Lk)] for one kv
    head's list (any ints: clamped into [0, pages - 1] as the kernel does)."""
    n = ve - first
    rows = list(range(first))
    for p in lst:
        p = min(max(int(p), 0), pages_of(n) - 1)
        rows += range(first + PAGE * p, first + min(PAGE * p + PAGE, n))
    return torch.tensor(rows + list(range(ve, Lk)), dtype=torch.long)


def gather(K, V, first, ve, Lk, lists):
    """K / V [1, Hkv, >= Lk, D] -> ([1, Hkv, L', D], ...) per the lists [Hkv, keep_pages]; every head must name as many rows
    (true whenever the partial last page is in every list or in none)."""
    idx = [gathered_rows(first, ve, Lk, lists[g]).to(K.device) for g in range(K.shape[1])]
    assert len({len(i) for i in idx}) == 1
    pick = lambda T: torch.stack([T[0, g, idx[g]] for g in range(T.shape[1])])[None].contiguous()   # noqa: E731
    return pick(K), pick(V)


# ---- shared by tests/test_attention_paged*_gpu.py and tests/test_sparse_decode*_gpu.py ----
def dev():
    return torch.device("cuda:0")


def code(t):
    import retake._native as nv

    return nv.dtype_code(t)


def with_slack(rows, slack, fill=0):
    """[1, Hkv, L, ...] -> a buffer [1, Hkv, L + slack, ...] holding `rows`, `fill` behind them."""
    buf = torch.full((1, rows.shape[1], rows.shape[2] + slack) + tuple(rows.shape[3:]), fill, dtype=rows.dtype, device=rows.device)
    buf[:, :, :rows.shape[2]] = rows
    return buf


def call_painted(name, need, call):
    """A native call, call(workspace pointer) -> rc, over a workspace of exactly `need` bytes with 64 painted bytes behind it,
    which must stay as they were."""
    import retake._native as nv

    assert need, nv.lib.rtk_last_error()
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev())
    ws[need:] = 0x5a
    nv.check(call(nv.ptr(ws)), name)
    torch.cuda.synchronize()
    assert (ws[need:] == 0x5a).all(), "the call wrote behind its workspace"


def dequant(codes, scales, dtype):
    from retake.native_attention import fp8_dequantize_rows

    return fp8_dequantize_rows(codes.contiguous(), scales.contiguous(), dtype)


def gather_archive(archive, n, lists):
    """(k8, v8, k_scale, v_scale) [1, Hkv, >= n, ..] -> the same four over the existing rows of the pages each kv head's list
    names, in list order (any ints: clamped into [0, pages - 1] as the kernel does); every head must name as many rows."""
    idx = [gathered_rows(0, n, n, lst).to(archive[0].device) for lst in lists]
    assert len({len(i) for i in idx}) == 1
    return tuple(torch.stack([t[0, g].index_select(0, i) for g, i in enumerate(idx)])[None].contiguous() for t in archive)


def token(d, route, seed, **kw):
    """One decode token of test_focus_gpu's driver through the route -> [(rotated q, K view, V view)] per layer."""
    return d.feed(d.cache, seed, d.text_ids(1), route, **kw)

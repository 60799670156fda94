"""Yardsticks for the native chunk attention (tests/test_attention_gpu.py, tools/bench_attention.py): float64 truth, the
reference's eager expression, and the input sets.  Torch on the device the tensors live on."""
import math

import numpy as np
import torch

import synth


def causal_visible(Lq: int, Lk: int, rows: torch.Tensor, device) -> torch.Tensor:
    """bool [len(rows), Lk]: key j is visible to query row i iff j <= (Lk - Lq) + i."""
    return torch.arange(Lk, device=device)[None, :] <= (Lk - Lq) + rows[:, None]


def attention_fp64(q, k, v, scale=None, row_chunk=None):
    """softmax(q k^T * scale, bottom-right causal) v in float64 on the given (already rounded) inputs.
    q [1, Hq, Lq, D], k / v [1, Hkv, Lk, D] -> [1, Lq, Hq, D] float64.  Chunked over query rows so the logits fit."""
    _, Hq, Lq, D = q.shape
    _, Hkv, Lk, _ = k.shape
    G = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    kd, vd = k[0].double(), v[0].double()
    out = torch.empty((1, Lq, Hq, D), dtype=torch.float64, device=q.device)
    if row_chunk is None:
        row_chunk = max(1, min(Lq, (1 << 26) // max(1, Lk)))   # logits of one head chunk: <= 512 MB of float64
    for h in range(Hq):
        kh, vh = kd[h // G], vd[h // G]
        for r0 in range(0, Lq, row_chunk):
            rows = torch.arange(r0, min(Lq, r0 + row_chunk), device=q.device)
            s = (q[0, h, r0:r0 + row_chunk].double() @ kh.T) * scale
            s.masked_fill_(~causal_visible(Lq, Lk, rows, q.device), -math.inf)
            out[0, r0:r0 + row_chunk, h] = torch.softmax(s, dim=-1) @ vh
    return out


def eager_bytes(Hq: int, Lq: int, Lk: int) -> int:
    return Hq * Lq * Lk * 4


def attention_eager_reference(q, k, v, scale=None):
    """The reference's eager expression (qwen2_vl.py:88-117) on [1, H, L, D] tensors of the model dtype: repeat_kv, matmul in
    the dtype, / sqrt(D), additive causal mask, softmax in float32, cast back, matmul in the dtype -> [1, Lq, Hq, D]."""
    _, Hq, Lq, D = q.shape
    _, Hkv, Lk, _ = k.shape
    G = Hq // Hkv
    kk = k[:, :, None].expand(1, Hkv, G, Lk, D).reshape(1, Hq, Lk, D)
    vv = v[:, :, None].expand(1, Hkv, G, Lk, D).reshape(1, Hq, Lk, D)
    w = torch.matmul(q, kk.transpose(2, 3))
    w = w / math.sqrt(D) if scale is None else w * scale
    rows = torch.arange(Lq, device=q.device)
    mask = torch.zeros((Lq, Lk), dtype=q.dtype, device=q.device)
    mask.masked_fill_(~causal_visible(Lq, Lk, rows, q.device), torch.finfo(q.dtype).min)
    w = w + mask[None, None]
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    return torch.matmul(w, vv).transpose(1, 2).contiguous()


def make_inputs(kind: str, seed: int, Hq: int, Hkv: int, Lq: int, Lk: int, D: int, dtype, device):
    """q [1, Hq, Lq, D], k / v [1, Hkv, Lk, D] of `dtype` on `device`.
      "synth"   tests/synth.py::qkv_chunk (1.7 * N(0, 1)): the queries of one call, the keys / values of another
      "peaked"  the same with q scaled x8: rows dominated by a few keys, large steps of the running maximum
      "rising"  keys ordered so that every row's largest logit is its LAST visible key: key j = c_j * u with u > 0
                elementwise, c_j growing in j, and every query positive elementwise, so the logits are non-decreasing in j
                in any precision (rounding is monotone) - the running maximum moves at every tile."""
    q0 = synth.qkv_chunk(seed, Hq, 1, Lq, D)[0]
    _, k0, v0 = synth.qkv_chunk(seed + 1, 1, Hkv, Lk, D)
    if kind == "peaked":
        q0 = q0 * 8.0
    elif kind == "rising":
        rng = np.random.default_rng(seed + 1000)
        u = np.abs(rng.standard_normal(D)).astype(np.float32) + 0.1
        u /= np.linalg.norm(u)
        ramp = np.linspace(1.0, 12.0, Lk, dtype=np.float32)
        k0 = np.broadcast_to(ramp[None, None, :, None] * u[None, None, None, :], k0.shape)
        q0 = 0.3 * np.abs(q0) + 4.0 * u[None, None, None, :]
    elif kind != "synth":
        raise ValueError(kind)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)   # noqa: E731
    return to(q0), to(k0), to(v0)


def half_ulp(dtype, magnitude: float) -> float:
    """Half a unit in the last place of `dtype` at `magnitude`: the rounding of the output store itself."""
    bits = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}[dtype]
    if magnitude <= 0:
        return 0.0
    return 0.5 * 2.0 ** (math.floor(math.log2(magnitude)) - (bits - 1))

"""Host restatement of the RoPE arithmetic of csrc/common.cuh (rope_elem, rotate_words) and csrc/rope.hip
(rope_table_kernel, rope_shift_kernel): numpy / CPU torch only, no call into the library.

  tables    angle = fp32(fp32(id) * inv_freq[d mod D/2]) with the id of position row row[d] (make_rowsel); cos / sin = the
            float64 libm value rounded to fp32, * fp32(scaling) rounded to fp32, rounded to the table dtype
            (round_mode 0 / 1 / 2 = fp32 / bf16 / fp16) - what test_native_rope_tables_are_correctly_rounded asserts.
  rotate    out = rd(rd(x * cos) + rd(rotate_half(x) * sin)), one rounding per op in the tensor dtype.
  shift     o1 = x1 c - x2 s, o2 = x2 c + x1 s with c, s the correctly rounded fp32 cos / sin of fp32(fp32(delta) *
            inv_freq[d]), on the channels of position row 0: the float64 value of that expression (no per-op model).
  reforge   min + ((id - min) * keep / L).long()  (plain-RoPE ids of the kept tokens).

The error bounds of tests/test_rope_ref_cpu.py and tests/test_rope_gpu.py are derived here, not measured (u = unit
roundoff of the tensor dtype):
  rotate    |out - truth| <= 4 u (|x1 cos64| + |x2 sin64|) for 16-bit tensors: one table rounding, two product roundings
            and the sum's rounding (|sum| <= |a| + |b|), with margin for the fp32 steps behind the table; 6 u for fp32,
            whose tables carry two fp32 roundings (libm -> fp32, * scaling) and an fp32 scaling.
  shift     |out - truth| <= (u + 2^-21) (|x1 c| + |x2 s|): the store's rounding plus at most four fp32 roundings, doubled.
  plus one subnormal of the dtype as a floor.
"""
from __future__ import annotations

import numpy as np
import torch

UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
SUBNORMAL = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -149}
TABLE_DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def round_mode(dtype) -> int:
    return 1 if dtype == torch.bfloat16 else (2 if dtype == torch.float16 else 0)


def rowsel(D: int, P: int, sections=None) -> np.ndarray:
    """row[d]: the position row that feeds channel d (all 0 for P = 1; two repetitions of the sections for P = 3)."""
    if P == 1:
        return np.zeros(D, dtype=np.int64)
    assert P == 3 and sections and 2 * sum(sections) == D
    nsec = len(sections)
    return np.array([(rep * nsec + i) % 3 for rep in range(2) for i, s in enumerate(sections) for _ in range(s)], dtype=np.int64)


def angles(ids: np.ndarray, inv_freq: np.ndarray, D: int, sections=None) -> np.ndarray:
    """ids [P, n] int64 -> the fp32 angles [n, D]."""
    ids = np.asarray(ids, dtype=np.int64)
    row = rowsel(D, ids.shape[0], sections)
    f = np.asarray(inv_freq, dtype=np.float32)[np.arange(D) % (D // 2)]
    p = ids[row, :].T.astype(np.float32)                     # [n, D]: fp32(id) each channel sees
    return (p * f[None, :]).astype(np.float32)


def _round(x32: np.ndarray, mode: int) -> np.ndarray:
    """fp32 values rounded (to nearest even) to the table dtype, held in fp32."""
    if mode == 0:
        return x32
    return torch.from_numpy(np.ascontiguousarray(x32)).to(TABLE_DTYPE[mode]).float().numpy()


def tables(ids, inv_freq, D: int, scaling: float, mode: int, sections=None):
    """-> (cos, sin) [n, D] fp32 arrays holding values of the table dtype."""
    ang = angles(ids, inv_freq, D, sections).astype(np.float64)
    s32 = np.float32(scaling)
    c = (np.cos(ang).astype(np.float32) * s32).astype(np.float32)
    s = (np.sin(ang).astype(np.float32) * s32).astype(np.float32)
    return _round(c, mode), _round(s, mode)


def rotate_half(x):
    h = x.shape[-1] // 2
    if isinstance(x, np.ndarray):
        return np.concatenate([-x[..., h:], x[..., :h]], axis=-1)
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def rotate(x: torch.Tensor, cos: np.ndarray, sin: np.ndarray) -> torch.Tensor:
    """x [..., n, D] (CPU, fp32 / bf16 / fp16), cos / sin [n, D] from `tables` -> the forward rotation, one rounding per op."""
    if x.dtype == torch.float32:   # separate products and a separate add: no fused multiply-add
        xn = x.numpy()
        a = (xn * cos).astype(np.float32)
        b = (rotate_half(xn) * sin).astype(np.float32)
        return torch.from_numpy((a + b).astype(np.float32))
    c, s = torch.from_numpy(cos).to(x.dtype), torch.from_numpy(sin).to(x.dtype)   # exact: the values are of that dtype
    return (x * c) + (rotate_half(x) * s)


def rotate_truth(x: torch.Tensor, ang32: np.ndarray, scaling: float):
    """float64 truth of the forward rotation at the SAME fp32 angles, and the magnitude |x1 cos64| + |x2 sin64| its error
    bound scales with."""
    xd = x.double().numpy()
    a = ang32.astype(np.float64)
    c, s = np.cos(a) * float(scaling), np.sin(a) * float(scaling)
    rh = rotate_half(xd)
    return xd * c + rh * s, np.abs(xd * c) + np.abs(rh * s)


def rotate_bound(dtype, mag: np.ndarray) -> np.ndarray:
    return (6.0 if dtype == torch.float32 else 4.0) * UNIT_ROUNDOFF[dtype] * mag + SUBNORMAL[dtype]


def shift(x: torch.Tensor, delta: int, inv_freq: np.ndarray, P: int = 1, sections=None):
    """x [..., n, D] rotated by `delta` temporal steps on the channels of position row 0 -> (float64 result, magnitude
    |x1 c| + |x2 s| of the touched channels; untouched channels: the value itself, magnitude 0)."""
    D = x.shape[-1]
    h = D // 2
    ang = (np.float32(delta) * np.asarray(inv_freq, dtype=np.float32)).astype(np.float32).astype(np.float64)   # [h]
    c = np.cos(ang).astype(np.float32).astype(np.float64)
    s = np.sin(ang).astype(np.float32).astype(np.float64)
    xd = x.double().numpy()
    x1, x2 = xd[..., :h], xd[..., h:]
    on = rowsel(D, P, sections)[:h] == 0
    o1 = np.where(on, x1 * c - x2 * s, x1)
    o2 = np.where(on, x2 * c + x1 * s, x2)
    m1 = np.where(on, np.abs(x1 * c) + np.abs(x2 * s), 0.0)
    m2 = np.where(on, np.abs(x2 * c) + np.abs(x1 * s), 0.0)
    return np.concatenate([o1, o2], axis=-1), np.concatenate([m1, m2], axis=-1)


def shift_bound(dtype, mag: np.ndarray) -> np.ndarray:
    return (UNIT_ROUNDOFF[dtype] + 2.0 ** -21) * mag + SUBNORMAL[dtype]


def reforge_ids(ids: torch.Tensor, keep: int, L: int) -> torch.Tensor:
    """The plain-RoPE ids [keep] int64 of a chunk's kept tokens -> their reforged ids."""
    mn = ids.min()
    return mn + ((ids - mn) * (keep / L)).long()

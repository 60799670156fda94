"""The e4m3 row format of the compressed video K / V rows, in torch on the CPU: the SPECIFICATION the HIP kernels are
held to (include/retake_hip.h "FP8 rows of the compressed cache").

For one row of one kv head (the last axis; values of the model dtype taken to fp32; finite, and the row's largest
magnitude 0 or >= 2^-117, so that the scale is a normal fp32 number - the range the kernels support):
  1. amax = max |x_d|;
  2. amax == 0: scale = 1;
  3. otherwise amax = m 2^E, m in [0.5, 1) (frexp); e = E - 9 if m <= 0.875 else E - 8; scale = 2^e, so that
     amax / scale lies in (224, 448];
  4. code_d = round-to-nearest-even of x_d 2^-e (exact) to OCP e4m3fn; nothing saturates;
  5. dequantised value = dtype(float(code_d) * scale).
"""
import torch


def row_exponent(x: torch.Tensor) -> torch.Tensor:
    """e of rule 3 per row (int32, shape x.shape[:-1]); 0 for an all-zero row."""
    amax = x.detach().to("cpu", torch.float32).abs().amax(dim=-1)
    m, E = torch.frexp(amax)
    e = E - torch.where(m <= 0.875, 9, 8).to(E.dtype)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def quantize(x: torch.Tensor):
    """x [..., D] (bf16 / fp16 / fp32 holding such values) -> (codes uint8 [..., D], scale fp32 [...])."""
    xf = x.detach().to("cpu", torch.float32)
    e = row_exponent(xf)
    scaled = torch.ldexp(xf, (-e).unsqueeze(-1).expand_as(xf))   # exact: a power of two, results within +-448
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    scale = torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)
    return codes, scale


def dequantize(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    f = codes.detach().to("cpu").view(torch.float8_e4m3fn).to(torch.float32)
    return (f * scale.detach().to("cpu", torch.float32).unsqueeze(-1)).to(dtype)


def exhaustive_rows(dtype: torch.dtype) -> torch.Tensor:
    """Every 16-bit pattern of `dtype` with |x| <= 448 (NaN and inf excluded), 127 per row of 128; element 127 of every
    row is 448, which pins the row's scale to 1 - the codes are then the plain e4m3 conversion of the values."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = v[v.float().abs() <= 448]
    n = (v.numel() + 126) // 127
    flat = torch.zeros(n * 127, dtype=dtype)
    flat[:v.numel()] = v
    rows = torch.zeros(n, 128, dtype=dtype)
    rows[:, :127] = flat.view(n, 127)
    rows[:, 127] = 448
    return rows

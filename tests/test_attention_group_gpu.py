"""rtk_attention_decode_group on the GPU, through native_attention.group_decode_attention: ONE query row of each of B
branches over [archive | shared 16-bit rows | the branch's own rows], in one launch.

  truth        every branch's output against float64 on the same inputs (archive dequantised by fp8_dequantize_rows), held
               to the bar tests/test_attention_gpu.py applies to the 16-bit kernels: max(2 E, half an ulp of the output
               dtype at the output's magnitude), E the eager expression's error on the same tensors;
  composition  (an invariance of the call, besides the truth test) a branch's bits are those of the group of that branch
               alone, and the reversed group gives the reversed outputs;
  twin         the existing per-branch call, chunk_attention(shared=, archive=, packed_gqa=True), is run on every case and
               its float64 error printed beside the group's (profiles/group_decode_parity_stats.txt is this output);
  refusals     before any launch, with the output buffer untouched.

The shared rows live in a buffer of their own with NaN past Ls; each branch's own rows in a buffer of its own with NaN past
Lk_b and around every row, head and row strides differing from branch to branch.  Own rows cycle through 1, 33, 130 and 600
(RTK_DECODE_GROUP_OWN_KEYS = 512: 600 takes two own splits, so the shorter branches leave empty partials); Ls 1056 splits
the shared range."""
import ctypes as C
import functools

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

D = 128
OWN = (1, 33, 130, 600)
LS, L8S = (0, 1, 32, 45, 160, 1056), (0, 45, 64)
BF16, F16 = torch.bfloat16, torch.float16


def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _common(seed, Hkv, Ls, L8, dtype):
    """The rows every branch shares: the archive of the first L8 rows (None without one), the shared rows as views of a
    NaN-padded buffer (None without any) and the dense [dequantised archive | shared] rows.  Made once, never written."""
    import retake.longvideo_cache as lc

    _, k, v = ar.make_inputs("synth", seed, 2, Hkv, 1, max(1, L8 + Ls), D, dtype, dev())
    k, v = k[:, :, :L8 + Ls], v[:, :, :L8 + Ls]
    archive, dense = None, (k, v)
    if L8:
        ck, sk = lc.fp8_quantize_rows(k[:, :, :L8].contiguous())
        cv, sv = lc.fp8_quantize_rows(v[:, :, :L8].contiguous())
        archive = (ck, cv, sk, sv)
        dense = tuple(torch.cat([lc.fp8_dequantize_rows(c, s, dtype), t[:, :, L8:]], dim=2) for c, s, t in ((ck, sk, k), (cv, sv, v)))
    shared = None
    if Ls:
        shared = []
        for t in (k, v):
            buf = torch.full((1, Hkv, Ls + 7, D), float("nan"), dtype=dtype, device=dev())   # rows past Ls must never be read
            buf[:, :, :Ls].copy_(t[:, :, L8:])
            shared.append(buf[:, :, :Ls])
        shared = tuple(shared)
    return archive, shared, dense


@functools.lru_cache(maxsize=None)
def _branch(b, Hq, Hkv, dtype):
    """Branch b's query [1, Hq, 1, D] and own rows, Lk_b = OWN[b % 4], as views of NaN-filled buffers of
    [1, Hkv, Lk_b + 3 + b, D + 8 b] elements: other head and row strides for every b."""
    Lk = OWN[b % len(OWN)]
    q, k, v = ar.make_inputs("synth", 100 + 3 * b, Hq, Hkv, 1, Lk, D, dtype, dev())
    own = []
    for t in (k, v):
        buf = torch.full((1, Hkv, Lk + 3 + b, D + 8 * b), float("nan"), dtype=dtype, device=dev())
        buf[:, :, :Lk, :D].copy_(t)
        own.append(buf[:, :, :Lk, :D])
    return q, tuple(own)


@functools.lru_cache(maxsize=None)
def _truth(b, Hq, Hkv, Ls, L8, dtype):
    """float64 over [dequantised archive | shared | own_b], the eager expression's error E on the same tensors, the bar."""
    _, _, dense = _common(5, Hkv, Ls, L8, dtype)
    q, own = _branch(b, Hq, Hkv, dtype)
    k, v = (torch.cat([c, o], dim=2) for c, o in zip(dense, own))
    ref = ar.attention_fp64(q, k, v)
    e = (ar.attention_eager_reference(q, k, v).double() - ref).abs().max().item()
    return ref, e, max(2.0 * e, ar.half_ulp(dtype, ref.abs().max().item()))


def _group(members, Hq, Hkv, Ls, L8, dtype):
    import retake.native_attention as na

    archive, shared, _ = _common(5, Hkv, Ls, L8, dtype)
    qs, owns = zip(*(_branch(b, Hq, Hkv, dtype) for b in members))
    out = na.group_decode_attention(list(qs), list(owns), shared, archive)
    assert out is not None and out.shape == (len(members), 1, Hq, D) and out.dtype == dtype
    return out


def _truth_case(Hq, Hkv, B, Ls, L8, dtype):
    import retake.longvideo_cache as lc

    archive, shared, _ = _common(5, Hkv, Ls, L8, dtype)
    out = _group(range(B), Hq, Hkv, Ls, L8, dtype)
    assert torch.isfinite(out.float()).all(), (Hq, B, Ls, L8)
    for b in range(B):
        ref, e, bar = _truth(b, Hq, Hkv, Ls, L8, dtype)
        q, own = _branch(b, Hq, Hkv, dtype)
        route = []
        twin = lc.chunk_attention(q, own[0], own[1], archive=archive, shared=shared, packed_gqa=True, route=route)
        assert twin is not None and route == ["packed"]
        err = (out[b:b + 1].double() - ref).abs().max().item()
        terr = (twin.double() - ref).abs().max().item()
        print(f"fp64[group {str(dtype)[6:]} Hq {Hq}/{Hkv} B {B} b {b} Lk {own[0].shape[2]} Ls {Ls} L8 {L8}]: "
              f"native {err:.3e}  per-branch call {terr:.3e}  eager E {e:.3e}  bar {bar:.3e}")
        assert err <= bar, (Hq, B, b, Ls, L8, err, bar)


# ---------------------------------------------------------------------------------------------------
# truth (+ the twin's figures)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L8", L8S)
@pytest.mark.parametrize("Hq,Hkv,B", [(14, 2, 1), (14, 2, 2), (14, 2, 3), (14, 2, 4), (4, 2, 8), (8, 2, 8)],
                         ids=["G7-B1-R7", "G7-B2-R14", "G7-B3-R21", "G7-B4-R28", "G2-B8-R16", "G4-B8-R32"])
def test_truth(Hq, Hkv, B, L8):
    for Ls in LS:
        _truth_case(Hq, Hkv, B, Ls, L8, BF16)


def test_truth_fp16():
    _truth_case(14, 2, 2, 45, 45, F16)


# ---------------------------------------------------------------------------------------------------
# composition, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L8", L8S)
def test_composition_bitwise(L8):
    for Ls in LS:
        whole = _group(range(4), 14, 2, Ls, L8, BF16)
        for i in range(4):
            alone = _group([i], 14, 2, Ls, L8, BF16)
            assert torch.equal(_bits(whole[i]), _bits(alone[0])), ("alone", i, Ls, L8)
        back = _group([3, 2, 1, 0], 14, 2, Ls, L8, BF16)
        assert torch.equal(_bits(back.flip(0)), _bits(whole)), ("reversed", Ls, L8)


# ---------------------------------------------------------------------------------------------------
# refusals, nothing launched
# ---------------------------------------------------------------------------------------------------
def _c_call(qs, owns, shared, out, Hq, Hkv, Dh, code, ws="sized", lk=None, s_off=0):
    """The C call itself.  ws: "sized" = what the query asks for, else (tensor or None, bytes)."""
    import retake._native as nv

    B = len(qs)
    brs, rows = (nv.DecodeBranch * B)(), (C.c_int * B)()
    for b, (q, (k, v)) in enumerate(zip(qs, owns)):
        br = brs[b]
        br.q, br.q_stride_h, br.k, br.v = q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr()
        br.kv_stride_h, br.kv_stride_l, br.Lk = k.stride(1), k.stride(2), k.shape[2] if lk is None else lk
        rows[b] = br.Lk
    Ls = shared[0].shape[2] if shared else 0
    need = nv.lib.rtk_attention_decode_group_workspace_bytes(rows, B, Hq, Hkv, 0, Ls, Dh, code)
    if ws == "sized":
        ws = (torch.empty(max(need, 16), dtype=torch.uint8, device=dev()), need)
    s = (C.c_void_p(shared[0].data_ptr() + s_off), C.c_void_p(shared[1].data_ptr() + s_off), Ls, shared[0].stride(1),
         shared[0].stride(2)) if shared else (None, None, 0, 0, 0)
    rc = nv.lib.rtk_attention_decode_group(brs, B, *s, None, None, None, None, 0, 0, 0, nv.ptr(out), Hq, Hkv, Dh, code,
                                           Dh ** -0.5, nv.ptr(ws[0]), ws[1], nv.stream())
    return rc, need, nv.lib.rtk_last_error()


def test_refusals():
    import retake._native as nv
    import retake.native_attention as na

    _, shared, _ = _common(5, 2, 45, 0, BF16)

    def inputs(Hq, B, dtype=BF16):
        return zip(*(_branch(b, Hq, 2, dtype) for b in range(B)))

    def refused(rc_want, word, qs, owns, Hq, code=nv.RTK_BF16, Dh=D, sh=shared, need0=True, **kw):
        out = torch.full((len(qs), 1, Hq, Dh), 7.0, dtype=torch.float32, device=dev())   # (large enough for any dtype)
        rc, need, msg = _c_call(qs, owns, sh, out, Hq, 2, Dh, code, **kw)
        torch.cuda.synchronize()
        assert rc == rc_want and word in msg, (rc, msg)
        assert need0 == (need == 0), (need, msg)
        assert (out == 7.0).all(), "a refused call wrote the output"

    # 35 packed rows; 9 branches
    qs, owns = inputs(14, 5)
    refused(nv.RTK_EUNSUPPORTED, b"packed rows", qs, owns, 14)
    assert na.group_decode_attention(list(qs), list(owns), shared, None) is None
    qs, owns = inputs(4, 9)
    refused(nv.RTK_EUNSUPPORTED, b"9 branches", qs, owns, 4)
    assert na.group_decode_attention(list(qs), list(owns), shared, None) is None
    # float32; head_dim 64
    qs, owns = inputs(4, 2)
    refused(nv.RTK_EUNSUPPORTED, b"dtype", qs, owns, 4, code=nv.RTK_F32)
    q32 = [q.float() for q in qs]
    o32 = [(k.float(), v.float()) for k, v in owns]
    assert na.group_decode_attention(q32, o32, tuple(t.float() for t in shared), None) is None
    refused(nv.RTK_EUNSUPPORTED, b"head_dim", qs, owns, 4, Dh=64, sh=None)
    q64 = [q[..., :64].contiguous() for q in qs]
    o64 = [(k[..., :64].contiguous(), v[..., :64].contiguous()) for k, v in owns]
    assert na.group_decode_attention(q64, o64, None, None) is None
    # a branch without own rows
    refused(nv.RTK_EINVAL, b"Lk 0", qs, owns, 4, lk=0)
    with pytest.raises(ValueError, match="own rows"):
        na.group_decode_attention(list(qs), [(k[:, :, :0], v[:, :, :0]) for k, v in owns], shared, None)
    # a short workspace; a misaligned shared pointer
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    refused(nv.RTK_EWORKSPACE, b"workspace too small", qs, owns, 4, need0=False, ws=(ws, 64))
    refused(nv.RTK_EWORKSPACE, b"workspace too small", qs, owns, 4, need0=False, ws=(None, 0))
    refused(nv.RTK_EUNSUPPORTED, b"layout of the shared rows", qs, owns, 4, need0=False, s_off=2)
    # ... and the same inputs, unharmed, are served
    out = torch.empty((2, 4, D), dtype=BF16, device=dev())
    rc, need, _ = _c_call(qs, owns, shared, out, 4, 2, D, nv.RTK_BF16)
    assert rc == 0 and need > 0
    assert torch.equal(_bits(out), _bits(na.group_decode_attention(list(qs), list(owns), shared, None).view(2, 4, D)))

"""Kernel-level operators over device tensors — the Python mirror of the reference's
``kernel::*_cuda`` launchers (include/kernel/cuda/*.cuh), each a thin call into libsli.so.

Tensors are torch tensors on the HIP device (PyTorch here is only the device-memory and stream
plumbing); every function launches on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import DT_F8E4M3, DT_F16, DT_F32, DT_I8, DT_MXFP4, call

_DT = {torch.float32: DT_F32, torch.float16: DT_F16, torch.int8: DT_I8, torch.float8_e4m3fn: DT_F8E4M3}
_KV_NAMES = {"f32": DT_F32, "f16": DT_F16, "f8": DT_F8E4M3, "fp8": DT_F8E4M3, "e4m3": DT_F8E4M3}


def _kv_dt(cache, kv_dtype):
    """Cache dtype code: the tensor's own, or kv_dtype="f8" for E4M3 codes held in a uint8 tensor."""
    if kv_dtype is None:
        return _DT[cache.dtype]
    dt = _KV_NAMES[kv_dtype]
    if dt == DT_F8E4M3:
        if cache.dtype not in (torch.uint8, torch.float8_e4m3fn):
            raise ValueError("an f8 cache is a uint8 or float8_e4m3fn tensor")
    elif _DT.get(cache.dtype) != dt:
        raise ValueError("kv_dtype does not match the cache tensor")
    return dt


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("operands must be contiguous device tensors")


def matmul(x, w, y=None, scale: float = 1.0, row_scale=None):
    """matmul_kernel_cuda (matmul_kernel.cuh:6-7): y = scale * W @ x, W [rows, cols] f32/f16/int8."""
    rows, cols = w.shape
    if x.numel() != cols:
        raise ValueError("Tensor with Wrong Dim!")  # matmul_kernel.cpp:8
    y = torch.empty(rows, device=x.device, dtype=torch.float32) if y is None else y
    _dev(x, w, y, row_scale)
    call("sli_matmul", _p(x), _p(w), _DT[w.dtype], _p(row_scale), _p(y), rows, cols, scale, _s())
    return y


def mxfp4_bytes(rows: int, cols: int) -> tuple[int, int]:
    """(data bytes, scale bytes) of a [rows, cols] MXFP4 tensor (sli.h); cols % 32 != 0 raises SliError."""
    d, s = ctypes.c_size_t(0), ctypes.c_size_t(0)
    call("sli_mxfp4_bytes", rows, cols, ctypes.byref(d), ctypes.byref(s))
    return d.value, s.value


def quant_mxfp4(w, data=None, scales=None):
    """fp32 [rows, cols] -> (data uint8 [rows, cols/2], scales uint8 [rows, cols/32]), the rule of sli.h."""
    rows, cols = w.shape
    mxfp4_bytes(rows, cols)
    data = torch.empty(rows, cols // 2, device=w.device, dtype=torch.uint8) if data is None else data
    scales = torch.empty(rows, cols // 32, device=w.device, dtype=torch.uint8) if scales is None else scales
    _dev(w, data, scales)
    if w.dtype != torch.float32:
        raise ValueError("quant_mxfp4 takes fp32")
    call("sli_quant_mxfp4", _p(w), _p(data), _p(scales), rows, cols, _s())
    return data, scales


def dequant_mxfp4(data, scales, out=None):
    """(data, scales) -> fp32 [rows, cols], exact."""
    rows, cols = data.shape[0], data.shape[1] * 2
    if scales.shape != (rows, cols // 32):
        raise ValueError("Tensor with Wrong Dim!")
    out = torch.empty(rows, cols, device=data.device, dtype=torch.float32) if out is None else out
    _dev(data, scales, out)
    call("sli_dequant_mxfp4", _p(data), _p(scales), _p(out), rows, cols, _s())
    return out


def matmul_mxfp4(x, data, scales, y=None, scale: float = 1.0):
    """y = scale * W @ x for MXFP4 weights (data uint8 [rows, cols/2], scales uint8 [rows, cols/32]), x fp32."""
    rows, cols = data.shape[0], data.shape[1] * 2
    if x.numel() != cols or scales.shape != (rows, cols // 32):
        raise ValueError("Tensor with Wrong Dim!")
    y = torch.empty(rows, device=x.device, dtype=torch.float32) if y is None else y
    _dev(x, data, scales, y)
    call("sli_matmul_mxfp4", _p(x), _p(data), _p(scales), _p(y), rows, cols, scale, _s())
    return y


def quant_f8(x, out=None):
    """fp32 -> FP8 E4M3 codes (uint8, same shape), the rule of sli.h: nearest, ties to even, |v| > 448 saturates."""
    if x.dtype != torch.float32:
        raise ValueError("quant_f8 takes fp32")
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8) if out is None else out
    _dev(x, out)
    call("sli_quant_f8", _p(x), _p(out), x.numel(), _s())
    return out


def dequant_f8(codes, out=None):
    """FP8 E4M3 codes (uint8 or float8_e4m3fn) -> fp32, exact; the NaN codes give NaN."""
    if codes.dtype not in (torch.uint8, torch.float8_e4m3fn):
        raise ValueError("dequant_f8 takes uint8 or float8_e4m3fn codes")
    out = torch.empty(codes.shape, device=codes.device, dtype=torch.float32) if out is None else out
    _dev(codes, out)
    call("sli_dequant_f8", _p(codes), _p(out), codes.numel(), _s())
    return out


def matmul_batch(x, w, y=None):
    """Batched projection for B <= 8 sequences on MFMA (bgemm.h): y[b] = W @ x[b]; x [B, cols] fp32, W
    [rows, cols] fp16, y [B, rows] fp32. No reference counterpart (the reference is batch 1)."""
    batch, cols = x.shape
    rows = w.shape[0]
    if w.shape[1] != cols:
        raise ValueError("Tensor with Wrong Dim!")
    y = torch.empty(batch, rows, device=x.device, dtype=torch.float32) if y is None else y
    nbytes = _lib.load().sli_matmul_batch_workspace_bytes(rows, cols, batch)
    if nbytes == 0:
        raise ValueError("unsupported batched shape (cols % 32 != 0 or batch > 8)")
    ws = torch.empty(nbytes // 4 + 1, device=x.device, dtype=torch.float32)
    _dev(x, w, y, ws)
    call("sli_matmul_batch", _p(x), _p(w), _DT[w.dtype], _p(y), rows, cols, batch, _p(ws), ws.numel() * 4, _s())
    return y


def matmul_batch_i8(x, w, row_scale=None, tiled: bool = False, y=None):
    """The batched projection from int8 weights: y[b][r] = (W[r] . x[b]) * row_scale[r]; x [B, cols] fp32, W
    [rows, cols] int8, row_scale [rows] fp32 or None (1), y [B, rows] fp32. tiled=True first re-lays W into the
    model's fragment layout (inside the workspace) and streams that image, the path a batched int8 model runs."""
    batch, cols = x.shape
    rows = w.shape[0]
    if w.shape[1] != cols or w.dtype != torch.int8 or (row_scale is not None and row_scale.numel() != rows):
        raise ValueError("Tensor with Wrong Dim!")
    y = torch.empty(batch, rows, device=x.device, dtype=torch.float32) if y is None else y
    nbytes = _lib.load().sli_matmul_batch_i8_workspace_bytes(rows, cols, batch, int(tiled))
    if nbytes == 0:
        raise ValueError("unsupported batched shape (cols % 32 != 0 or batch > 8)")
    ws = torch.empty(nbytes // 4 + 1, device=x.device, dtype=torch.float32)
    _dev(x, w, row_scale, y, ws)
    call("sli_matmul_batch_i8", _p(x), _p(w), _p(row_scale), _p(y), rows, cols, batch, int(tiled), _p(ws),
         ws.numel() * 4, _s())
    return y


def matmul_batch_mxfp4(x, data, scales, tiled: bool = False, y=None):
    """The batched projection from MXFP4 weights: y[b][r] = sum_c x[b][c] * code(W[r][c]) * 2^(scale[r][c / 32] - 127);
    x [B, cols] fp32, data uint8 [rows, cols / 2] and scales uint8 [rows, cols / 32] (quant_mxfp4's layout), y [B, rows]
    fp32. tiled=True first re-lays data and scales into the model's fragment-layout images (inside the workspace) and
    streams those, the path a batched MXFP4 model runs."""
    batch, cols = x.shape
    rows = data.shape[0]
    if (data.dtype != torch.uint8 or scales.dtype != torch.uint8 or cols % 32 or data.shape != (rows, cols // 2)
            or scales.shape != (rows, cols // 32)):
        raise ValueError("Tensor with Wrong Dim!")
    y = torch.empty(batch, rows, device=x.device, dtype=torch.float32) if y is None else y
    nbytes = _lib.load().sli_matmul_batch_mxfp4_workspace_bytes(rows, cols, batch, int(tiled))
    if nbytes == 0:
        raise ValueError("unsupported batched shape (cols % 32 != 0 or batch > 8)")
    ws = torch.empty(nbytes // 4 + 1, device=x.device, dtype=torch.float32)
    _dev(x, data, scales, y, ws)
    call("sli_matmul_batch_mxfp4", _p(x), _p(data), _p(scales), _p(y), rows, cols, batch, int(tiled), _p(ws),
         ws.numel() * 4, _s())
    return y


def rmsnorm(x, w, eps: float, y=None):
    """rmsnorm_kernel_cuda (rms_kernel.cuh:6-7)."""
    y = torch.empty_like(x) if y is None else y
    _dev(x, w, y)
    call("sli_rmsnorm", _p(x), _p(w), _p(y), x.numel(), eps, _s())
    return y


def rope_cache(head_dim: int, max_len: int, theta: float, device="cuda"):
    """rope_cache_cal_cuda (rope_kernel.cuh:5-6): (sin, cos) tables [max_len, head_dim/2]."""
    s = torch.empty(max_len, head_dim // 2, device=device, dtype=torch.float32)
    c = torch.empty_like(s)
    call("sli_rope_cache", head_dim, max_len, _p(s), _p(c), theta, _s())
    return s, c


def rope(q, k, pos, sin_c, cos_c, head_dim: int):
    """rope_kernel_cuda (rope_kernel.cuh:7-8), in place on q and k. pos: int or int32 device tensor."""
    _dev(q, k, sin_c, cos_c)
    pos_dev = pos if isinstance(pos, torch.Tensor) else None
    call("sli_rope", _p(q), _p(k), 0 if pos_dev is not None else int(pos), _p(pos_dev), _p(sin_c), _p(cos_c),
         q.numel(), k.numel(), head_dim, _s())
    return q, k


def mha(q, kcache, vcache, layer: int, pos: int, max_len: int, head_dim: int, n_heads: int, n_kv_heads: int,
        out=None, workspace=None, kv_dtype=None):
    """mha_kernel_cuda (mha_kernel.cuh:6-21) over a reference-layout [L, T, KV] cache: f32, f16, or FP8 E4M3 as a
    float8_e4m3fn tensor or as uint8 codes with kv_dtype="f8"."""
    out = torch.empty(n_heads * head_dim, device=q.device, dtype=torch.float32) if out is None else out
    nbytes = _lib.load().sli_mha_workspace_bytes(max_len, n_heads, head_dim)
    if workspace is None:
        workspace = torch.empty(max(nbytes // 4, 1), device=q.device, dtype=torch.float32)
    _dev(q, kcache, vcache, out, workspace)
    call("sli_mha", _p(q), _p(kcache), _p(vcache), _kv_dt(kcache, kv_dtype), _p(out), layer, pos, max_len, head_dim,
         n_heads, n_kv_heads, _p(workspace), workspace.numel() * 4, _s())
    return out


def mha_strided(q, k, v, pos: int, max_len: int, head_dim: int, n_heads: int, n_kv_heads: int, pos_stride: int,
                head_stride: int, out=None, workspace=None, kv_dtype=None):
    """The same attention over ONE layer's cache with explicit strides in elements (sli_mha_strided): the engine's
    head-major [Hkv, T, hd] is pos_stride=head_dim, head_stride=max_len * head_dim."""
    out = torch.empty(n_heads * head_dim, device=q.device, dtype=torch.float32) if out is None else out
    nbytes = _lib.load().sli_mha_workspace_bytes(max_len, n_heads, head_dim)
    if workspace is None:
        workspace = torch.empty(max(nbytes // 4, 1), device=q.device, dtype=torch.float32)
    _dev(q, k, v, out, workspace)
    call("sli_mha_strided", _p(q), _p(k), _p(v), _kv_dt(k, kv_dtype), _p(out), pos, max_len, head_dim, n_heads,
         n_kv_heads, pos_stride, head_stride, _p(workspace), workspace.numel() * 4, _s())
    return out


def softmax_(x):
    """softmax_kernel_cpu semantics (mha_kernel.cpp:7-20), in place."""
    _dev(x)
    call("sli_softmax", _p(x), x.numel(), _s())
    return x


def swiglu(up, gate, out=None):
    """swiglu_kernel_cuda (swiglu_kernel.cuh:5): sigmoid(gate) * up."""
    out = torch.empty_like(up) if out is None else out
    _dev(up, gate, out)
    call("sli_swiglu", _p(up), _p(gate), _p(out), up.numel(), _s())
    return out


def add(a, b, out=None):
    """add_kernel_cuda (add_kernel.cuh:6)."""
    out = torch.empty_like(a) if out is None else out
    _dev(a, b, out)
    call("sli_add", _p(a), _p(b), _p(out), a.numel(), _s())
    return out


def embedding(token, table, out=None, row_scale=None):
    """emb_kernel_cuda (emb_kernel.cuh:6-7). token: int or int32 device tensor."""
    vocab, dim = table.shape
    out = torch.empty(dim, device=table.device, dtype=torch.float32) if out is None else out
    tok_dev = token if isinstance(token, torch.Tensor) else None
    _dev(table, out, row_scale)
    call("sli_embedding", 0 if tok_dev is not None else int(token), _p(tok_dev), _p(table), _DT[table.dtype],
         _p(row_scale), _p(out), vocab, dim, _s())
    return out


# ---------------------------------------------------------------- prefill stages (sli.h "for tests and labs")
PF_ROLE_QKV, PF_ROLE_GATE_UP, PF_ROLE_RESID, PF_ROLE_LOGITS = 0, 1, 2, 3


def _pf_table(device):
    """SLI_PF_TABLE_BYTES of device memory: the group table every prefill entry fills on the stream."""
    return torch.empty(48, device=device, dtype=torch.int32)


def prefill_norm_split(x, w, eps: float):
    """pf_norm_split_kernel: x [M, D] fp32 -> (hi, lo) [M, D] fp16; w None: the plain split of x."""
    M, D = x.shape
    hi = torch.empty(M, D, device=x.device, dtype=torch.float16)
    lo = torch.empty_like(hi)
    _dev(x, w, hi, lo)
    call("sli_prefill_norm_split", _p(x), _p(w), _p(hi), _p(lo), M, D, eps, _s())
    return hi, lo


def _prefill_gemm_mxfp4(w, scales, hi, lo, p0, nv, epi):
    """sli_prefill_gemm_mxfp4: w uint8 [N, K/2] (two e2m1 codes per byte), scales uint8 [N, K/32] (e8m0)."""
    N, K = w.shape[0], w.shape[1] * 2
    M = hi.shape[0]
    if w.dtype != torch.uint8 or scales.dtype != torch.uint8 or scales.shape != (N, K // 32) or K % 32:
        raise ValueError("Tensor with Wrong Dim!")
    if hi.shape != (M, K) or lo.shape != (M, K) or hi.dtype != torch.float16 or lo.dtype != torch.float16:
        raise ValueError("Tensor with Wrong Dim!")
    state = _pf_table(w.device)
    _dev(w, scales, hi, lo)
    tl = _lib.PgemmTiling()
    call("sli_prefill_gemm_mxfp4", _p(w), _p(scales), _p(hi), _p(lo), N, K, M, p0, nv, ctypes.byref(epi), _p(state),
         ctypes.byref(tl), _s())
    return {n: getattr(tl, n) for n, _ in tl._fields_}


def _prefill_gemm(w, row_scale, hi, lo, p0, nv, epi, scales=None):
    if scales is not None:
        if row_scale is not None:
            raise ValueError("prefill GEMM: MXFP4 weights (scales=) take no row_scale")
        return _prefill_gemm_mxfp4(w, scales, hi, lo, p0, nv, epi)
    N, K = w.shape
    M = hi.shape[0]
    if hi.shape != (M, K) or lo.shape != (M, K) or hi.dtype != torch.float16 or lo.dtype != torch.float16:
        raise ValueError("Tensor with Wrong Dim!")
    if w.dtype not in (torch.float16, torch.int8):
        raise ValueError("prefill GEMM takes fp16 or int8 weights")
    state = _pf_table(w.device)
    _dev(w, row_scale, hi, lo)
    tl = _lib.PgemmTiling()
    call("sli_prefill_gemm", _p(w), _DT[w.dtype], _p(row_scale), _p(hi), _p(lo), N, K, M, p0, nv, ctypes.byref(epi),
         _p(state), ctypes.byref(tl), _s())
    return {n: getattr(tl, n) for n, _ in tl._fields_}


def prefill_gemm_qkv(w, hi, lo, q, kc, vc, sin_t, cos_t, hq: int, hkv: int, hd: int, p0: int, nv: int,
                     row_scale=None, scales=None, kv_dtype=None):
    """One pgemm_kernel launch with the q/k/v epilogue: W [(hq + 2 hkv) hd, K]; q [M, hq hd] fp32 gets every chunk
    row; kc / vc, one layer's cache [hkv, T, hd] (f16, f32, or FP8 E4M3: a float8_e4m3fn tensor, or uint8 codes with
    kv_dtype="f8"), get rows p0 + m for m < nv, p0 + m < T. Returns the tiling that ran. scales (uint8 [N, K/32]): W is
    MXFP4, uint8 [N, K/2] (the kernel's MXFP4 format); no row_scale then."""
    if kc.dtype != vc.dtype or kc.shape != vc.shape or kc.shape[0] != hkv or kc.shape[2] != hd:
        raise ValueError("Tensor with Wrong Dim!")
    T = kc.shape[1]
    if q.shape != (hi.shape[0], hq * hd) or sin_t.shape != (T, hd // 2) or cos_t.shape != (T, hd // 2):
        raise ValueError("Tensor with Wrong Dim!")
    _dev(q, kc, vc, sin_t, cos_t)
    e = _lib.PgemmEpilogue(role=PF_ROLE_QKV, q=q.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(),
                           kv_dtype=_kv_dt(kc, kv_dtype), sin_t=sin_t.data_ptr(), cos_t=cos_t.data_ptr(), hq=hq, hkv=hkv,
                           hd=hd, T=T)
    return _prefill_gemm(w, row_scale, hi, lo, p0, nv, e, scales)


def prefill_gemm_gate_up(w, hi, lo, ahi, alo, act_mode: int = 0, row_scale=None, scales=None):
    """One pgemm_kernel launch with the SwiGLU epilogue: W [2 inter, K] = [gate; up]; ahi / alo [M, inter] fp16."""
    inter = w.shape[0] // 2
    if ahi.shape != (hi.shape[0], inter) or alo.shape != ahi.shape:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(ahi, alo)
    e = _lib.PgemmEpilogue(role=PF_ROLE_GATE_UP, ahi=ahi.data_ptr(), alo=alo.data_ptr(), inter=inter,
                           act_mode=act_mode)
    return _prefill_gemm(w, row_scale, hi, lo, 0, hi.shape[0], e, scales)


def prefill_gemm_resid(w, hi, lo, y, resid=None, row_scale=None, scales=None):
    """One pgemm_kernel launch with the wo / down epilogue: y [M, ld] = (resid or 0) + W (hi + lo) * row scale."""
    if y.shape[0] != hi.shape[0] or (resid is not None and resid.shape != y.shape):
        raise ValueError("Tensor with Wrong Dim!")
    _dev(y, resid)
    e = _lib.PgemmEpilogue(role=PF_ROLE_RESID, y=y.data_ptr(), resid=resid.data_ptr() if resid is not None else None,
                           ld=y.shape[1])
    return _prefill_gemm(w, row_scale, hi, lo, 0, hi.shape[0], e, scales)


def prefill_gemm_logits(w, hi, lo, y, row_scale=None, scales=None):
    """One pgemm_kernel launch with the logits epilogue (role 3, the LM head over chunk rows): y [M, ld][:, :N] =
    W (hi + lo) * row scale for W's N >= 16 rows (any N); columns N .. ld - 1 of y are not written."""
    if y.shape[0] != hi.shape[0]:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(y)
    e = _lib.PgemmEpilogue(role=PF_ROLE_LOGITS, y=y.data_ptr(), ld=y.shape[1])
    return _prefill_gemm(w, row_scale, hi, lo, 0, hi.shape[0], e, scales)


def score_rows(logits, targets, want_top: bool = True):
    """sli_score_rows: per row of fp32 logits [M, V] (rows ``logits.stride(0)`` floats apart: a row-padded view is
    taken as it is) and int32 target, the target's log-probability, the first-max token and its log-probability (the
    rule: sli.h). Returns (logprob [M] fp32, top [M] int32, top_logprob [M] fp32), or logprob alone."""
    if logits.dim() == 1:
        logits = logits.unsqueeze(0)
    M, V = logits.shape
    if not logits.is_cuda or logits.dtype != torch.float32 or (V > 1 and logits.stride(1) != 1):
        raise ValueError("logits: fp32 device rows of contiguous elements")
    if not targets.is_cuda or targets.dtype != torch.int32 or targets.shape != (M,):
        raise ValueError("targets: an int32 device tensor of one target per row")
    _dev(targets)
    ld = logits.stride(0)
    if M == 1 or ld < V or ld % 4 or logits.data_ptr() % 16:  # the kernel reads whole float4: rows padded to 4 floats
        ld = (V + 3) // 4 * 4
        buf = torch.zeros(M, ld, device=logits.device, dtype=torch.float32)
        buf[:, :V] = logits
        logits = buf
    lp = torch.empty(M, device=logits.device, dtype=torch.float32)
    top = torch.empty(M, device=logits.device, dtype=torch.int32) if want_top else None
    tlp = torch.empty(M, device=logits.device, dtype=torch.float32) if want_top else None
    call("sli_score_rows", _p(logits), M, V, ld, _p(targets), _p(lp), _p(top), _p(tlp), _s())
    return (lp, top, tlp) if want_top else lp


def prefill_attn(q, kc, vc, M: int, p0: int, hq: int, hkv: int, hd: int, kv_dtype=None):
    """Block-causal prefill attention of chunk rows 0 .. M-1 at positions p0 + m over one layer's cache [hkv, T, hd]
    (f16 and FP8 E4M3: MFMA kernel, f32: VALU kernel; an FP8 cache is a float8_e4m3fn tensor, or uint8 codes with
    kv_dtype="f8"). q [rows, hq hd] fp32 with rows >= M (f32 cache: >= M rounded up to 64, the contract of
    sli_prefill_attn); returns (ohi, olo) [rows, hq hd] fp16."""
    rows = q.shape[0]
    if q.shape != (rows, hq * hd) or kc.shape != vc.shape or kc.shape[0] != hkv or kc.shape[2] != hd:
        raise ValueError("Tensor with Wrong Dim!")
    T = kc.shape[1]
    ohi = torch.zeros(rows, hq * hd, device=q.device, dtype=torch.float16)
    olo = torch.zeros_like(ohi)
    state = _pf_table(q.device)
    _dev(q, kc, vc)
    call("sli_prefill_attn", _p(q), _p(kc), _p(vc), _kv_dt(kc, kv_dtype), _p(ohi), _p(olo), M, rows, p0, hq, hkv, hd, T,
         _p(state), _s())
    return ohi, olo


# ---- the packed prefill of a batched model's sequences (sli_model_prefill_seqs): the packing rule and the two stages
# that read the group table
def prefill_pack(lens, seqs=None):
    """sli_prefill_pack (host only, no GPU): the chunks that prefill sequences ``seqs`` (default 0 .. len(lens)-1) with
    prompts of ``lens`` tokens. Returns (groups, chunk_rows): groups an int32 array [n, 3] of (seq, p0, nv), 16 chunk
    rows each, padding groups (nv == 0) included, chunk c's groups starting at 16 * c; chunk_rows the rows of each
    chunk (32 / 64 / 128 / 256)."""
    import numpy as np
    lens = np.ascontiguousarray(lens, np.int32)
    seqs = np.arange(lens.size, dtype=np.int32) if seqs is None else np.ascontiguousarray(seqs, np.int32)
    if seqs.shape != lens.shape or lens.ndim != 1:
        raise ValueError("prefill_pack: one length per sequence")
    cap_g = int(np.maximum(lens, 1).sum() // 16 + lens.size + 16)
    cap_c = cap_g // 16 + 1
    groups = np.zeros((cap_g, 3), np.int32)
    rows = np.zeros(cap_c, np.int32)
    n = ctypes.c_int32()
    call("sli_prefill_pack", seqs.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), lens.size,
         groups.ctypes.data_as(ctypes.c_void_p), cap_g, rows.ctypes.data_as(ctypes.c_void_p), cap_c, ctypes.byref(n))
    rows = rows[:n.value].copy()
    ng = 0 if n.value == 0 else 16 * (n.value - 1) + int(rows[-1]) // 16
    return groups[:ng].copy(), rows


def prefill_pack_from(starts, counts, seqs=None):
    """sli_prefill_pack_from (host only, no GPU): the chunks that continue sequences ``seqs`` (default 0 ..
    len(counts)-1) from positions ``starts`` with ``counts`` tokens each. Returns (groups, chunk_rows) as prefill_pack
    does; a sequence's first group starts at its start and ends at the next 16-boundary of its positions."""
    import numpy as np
    starts = np.ascontiguousarray(starts, np.int32)
    counts = np.ascontiguousarray(counts, np.int32)
    seqs = np.arange(counts.size, dtype=np.int32) if seqs is None else np.ascontiguousarray(seqs, np.int32)
    if seqs.shape != counts.shape or starts.shape != counts.shape or counts.ndim != 1:
        raise ValueError("prefill_pack_from: one start and one count per sequence")
    cap_g = int(np.maximum(counts, 1).sum() // 16 + 2 * counts.size + 16)
    cap_c = cap_g // 16 + 1
    groups = np.zeros((cap_g, 3), np.int32)
    rows = np.zeros(cap_c, np.int32)
    n = ctypes.c_int32()
    call("sli_prefill_pack_from", seqs.ctypes.data_as(ctypes.c_void_p), starts.ctypes.data_as(ctypes.c_void_p),
         counts.ctypes.data_as(ctypes.c_void_p), counts.size, groups.ctypes.data_as(ctypes.c_void_p), cap_g,
         rows.ctypes.data_as(ctypes.c_void_p), cap_c, ctypes.byref(n))
    rows = rows[:n.value].copy()
    ng = 0 if n.value == 0 else 16 * (n.value - 1) + int(rows[-1]) // 16
    return groups[:ng].copy(), rows


def kv_copy_prefix(kc, vc, src: int, dst: int, n: int):
    """sli_kv_copy_prefix: K and V rows [0, n) of every layer and kv head from sequence ``src`` to sequence ``dst`` of
    the caches kc / vc [L, B, hkv, T, hd] (contiguous device tensors of one dtype of 1, 2 or 4 bytes per element), in
    place, one launch. Every other byte of both caches is untouched."""
    if kc.shape != vc.shape or kc.dim() != 5 or kc.dtype != vc.dtype:
        raise ValueError("kv_copy_prefix: kc and vc are [L, B, hkv, T, hd] tensors of one dtype")
    if not (kc.is_cuda and vc.is_cuda and kc.is_contiguous() and vc.is_contiguous()):
        raise ValueError("kv_copy_prefix: contiguous device tensors")
    _dev(kc, vc)
    L, B, hkv, T, hd = kc.shape
    call("sli_kv_copy_prefix", _p(kc), _p(vc), kc.element_size(), L, B, hkv, T, hd, src, dst, n, _s())


def _pf_groups(groups, M):
    """(seq, p0, nv) triples -> a host array of M / 16 sli_pf_group (short lists end in padding groups)."""
    gs = [tuple(int(v) for v in g) for g in groups]
    if len(gs) > max(M // 16, 0):
        raise ValueError("more groups than the chunk holds")
    gs += [(0, 0, 0)] * (M // 16 - len(gs))
    arr = (_lib.PfGroup * max(len(gs), 1))()
    for i, (s, p0, nv) in enumerate(gs):
        arr[i] = _lib.PfGroup(s, p0, nv)
    return arr


def prefill_gemm_qkv_segs(w, hi, lo, q, kc, vc, sin_t, cos_t, hq: int, hkv: int, hd: int, groups, row_scale=None,
                          scales=None, kv_dtype=None):
    """prefill_gemm_qkv under a group table: kc / vc are one layer's cache of B sequences [B, hkv, T, hd] (f16, or FP8
    E4M3); groups a list of (seq, p0, nv), chunk rows 16 g .. being positions p0 .. p0 + 15 of sequence seq, the first
    nv written to its cache (nv 0: a padding group; missing groups are padding). Returns the tiling that ran."""
    if kc.dtype != vc.dtype or kc.shape != vc.shape or kc.dim() != 4 or kc.shape[1] != hkv or kc.shape[3] != hd:
        raise ValueError("Tensor with Wrong Dim!")
    B, T = kc.shape[0], kc.shape[2]
    M = hi.shape[0]
    if q.shape != (M, hq * hd) or sin_t.shape != (T, hd // 2) or cos_t.shape != (T, hd // 2):
        raise ValueError("Tensor with Wrong Dim!")
    if hi.shape != lo.shape or hi.dtype != torch.float16 or lo.dtype != torch.float16:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(q, kc, vc, sin_t, cos_t, hi, lo, w, row_scale, scales)
    e = _lib.PgemmEpilogue(role=PF_ROLE_QKV, q=q.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(),
                           kv_dtype=_kv_dt(kc, kv_dtype), sin_t=sin_t.data_ptr(), cos_t=cos_t.data_ptr(), hq=hq, hkv=hkv,
                           hd=hd, T=T)
    table = _pf_table(w.device)
    tl = _lib.PgemmTiling()
    gs = _pf_groups(groups, M)
    if scales is not None:
        if row_scale is not None:
            raise ValueError("prefill GEMM: MXFP4 weights (scales=) take no row_scale")
        N, K = w.shape[0], w.shape[1] * 2
        if w.dtype != torch.uint8 or scales.dtype != torch.uint8 or scales.shape != (N, K // 32) or hi.shape != (M, K):
            raise ValueError("Tensor with Wrong Dim!")
        call("sli_prefill_gemm_qkv_segs_mxfp4", _p(w), _p(scales), _p(hi), _p(lo), N, K, M, gs, B, ctypes.byref(e),
             _p(table), ctypes.byref(tl), _s())
    else:
        N, K = w.shape
        if hi.shape != (M, K) or w.dtype not in (torch.float16, torch.int8):
            raise ValueError("prefill GEMM takes fp16 or int8 weights [N, K] and hi / lo [M, K]")
        call("sli_prefill_gemm_qkv_segs", _p(w), _DT[w.dtype], _p(row_scale), _p(hi), _p(lo), N, K, M, gs, B,
             ctypes.byref(e), _p(table), ctypes.byref(tl), _s())
    return {n: getattr(tl, n) for n, _ in tl._fields_}


def prefill_attn_segs(q, kc, vc, groups, hq: int, hkv: int, hd: int, kv_dtype=None):
    """prefill_attn under a group table: q [M, hq hd] fp32, kc / vc [B, hkv, T, hd] (f16 or FP8 E4M3); group g's 16
    rows attend the cache rows 0 .. p0 + r of its sequence. Returns (ohi, olo) [M, hq hd] fp16; the rows of a padding
    group stay zero."""
    M = q.shape[0]
    if q.shape != (M, hq * hd) or kc.shape != vc.shape or kc.dim() != 4 or kc.shape[1] != hkv or kc.shape[3] != hd:
        raise ValueError("Tensor with Wrong Dim!")
    B, T = kc.shape[0], kc.shape[2]
    ohi = torch.zeros(M, hq * hd, device=q.device, dtype=torch.float16)
    olo = torch.zeros_like(ohi)
    table = _pf_table(q.device)
    _dev(q, kc, vc)
    call("sli_prefill_attn_segs", _p(q), _p(kc), _p(vc), _kv_dt(kc, kv_dtype), _p(ohi), _p(olo), M, _pf_groups(groups, M),
         B, hq, hkv, hd, T, _p(table), _s())
    return ohi, olo


BG_ROLE_QKV, BG_ROLE_GATE_UP, BG_ROLE_STORE, BG_ROLE_LOGITS = 0, 1, 2, 3


def batch_gemm_plan(rows: int, K: int, B: int, norm: bool, w_dtype=DT_F16, tiled: bool = False, plan=None):
    """The plan sli_batch_gemm would run for a [rows, K] matrix and the workspace bytes it needs, without a device:
    plan None asks the engine's planner, (tpw, splits) forces one. Returns (plan dict, bytes); bytes 0: refused.
    w_dtype DT_MXFP4: the plan and bytes of sli_batch_gemm_mxfp4."""
    p = _lib.BgemmPlan(tpw=plan[0], splits=plan[1]) if plan else _lib.BgemmPlan()
    if w_dtype == DT_MXFP4:
        nbytes = call("sli_batch_gemm_mxfp4_workspace_bytes", rows, K, B, int(norm), int(tiled), ctypes.byref(p))
    else:
        nbytes = call("sli_batch_gemm_workspace_bytes", rows, K, B, int(norm), w_dtype, int(tiled), ctypes.byref(p))
    return {n: getattr(p, n) for n, _ in p._fields_}, nbytes


def _batch_gemm_mx(x, norm_w, eps, data, scales, tiled, epi, rows, plan, ws):
    """sli_batch_gemm_mxfp4: _batch_gemm with w = the uint8 data [rows, K / 2] and scales = the block scales [rows, K / 32]."""
    B, K = x.shape
    if (K % 32 or data.dtype != torch.uint8 or scales.dtype != torch.uint8 or data.shape != (rows, K // 2)
            or scales.shape != (rows, K // 32) or x.dtype != torch.float32):
        raise ValueError("Tensor with Wrong Dim!")
    if norm_w is not None and norm_w.numel() != K:
        raise ValueError("Tensor with Wrong Dim!")
    p = _lib.BgemmPlan(tpw=plan[0], splits=plan[1]) if plan else _lib.BgemmPlan()
    q = _lib.BgemmPlan(tpw=p.tpw, splits=p.splits)
    nbytes = call("sli_batch_gemm_mxfp4_workspace_bytes", rows, K, B, int(norm_w is not None), int(tiled), ctypes.byref(q))
    if nbytes == 0:
        raise _lib.SliError(1, "sli_batch_gemm_mxfp4_workspace_bytes", (_lib.load().sli_last_error() or b"").decode())
    if ws is None:
        ws = torch.zeros(nbytes, device=x.device, dtype=torch.uint8)
    _dev(x, norm_w, data, scales, ws)
    call("sli_batch_gemm_mxfp4", _p(x), _p(norm_w), eps, _p(data), _p(scales), int(tiled), K, B, ctypes.byref(epi),
         ctypes.byref(p), _p(ws), ws.numel(), _s())
    out = {n: getattr(p, n) for n, _ in p._fields_}
    out["ws"] = ws
    return out


def _batch_gemm(x, norm_w, eps, w, row_scale, tiled, epi, rows, plan, ws, scales=None):
    """sli_batch_gemm. plan None: the engine's planner; (tpw, splits): forced. ws: a workspace of an earlier call
    with the same plan, reused as it is (its arrival counters are zero again), or None for a fresh zeroed one.
    Returns the plan that ran as a dict, with the workspace (a uint8 tensor) under "ws".
    scales given: MXFP4 weights, w is the uint8 data and scales the block scales (sli_batch_gemm_mxfp4)."""
    if scales is not None:
        if row_scale is not None:
            raise ValueError("MXFP4 weights have block scales, not a row scale: pass scales or row_scale, not both")
        return _batch_gemm_mx(x, norm_w, eps, w, scales, tiled, epi, rows, plan, ws)
    B, K = x.shape
    if w.shape != (rows, K) or w.dtype not in (torch.float16, torch.int8) or x.dtype != torch.float32:
        raise ValueError("Tensor with Wrong Dim!")
    if (norm_w is not None and norm_w.numel() != K) or (row_scale is not None and row_scale.numel() != rows):
        raise ValueError("Tensor with Wrong Dim!")
    p = _lib.BgemmPlan(tpw=plan[0], splits=plan[1]) if plan else _lib.BgemmPlan()
    q = _lib.BgemmPlan(tpw=p.tpw, splits=p.splits)
    nbytes = call("sli_batch_gemm_workspace_bytes", rows, K, B, int(norm_w is not None), _DT[w.dtype], int(tiled),
                  ctypes.byref(q))
    if nbytes == 0:
        raise _lib.SliError(1, "sli_batch_gemm_workspace_bytes", (_lib.load().sli_last_error() or b"").decode())
    if ws is None:
        ws = torch.zeros(nbytes, device=x.device, dtype=torch.uint8)
    _dev(x, norm_w, w, row_scale, ws)
    call("sli_batch_gemm", _p(x), _p(norm_w), eps, _p(w), _DT[w.dtype], _p(row_scale), int(tiled), K, B,
         ctypes.byref(epi), ctypes.byref(p), _p(ws), ws.numel(), _s())
    out = {n: getattr(p, n) for n, _ in p._fields_}
    out["ws"] = ws
    return out


# With `scales` given, every batch_gemm_* below runs MXFP4 weights: w is the uint8 data [rows, K / 2] and scales the e8m0
# block scales [rows, K / 32] (quant_mxfp4's layout); row_scale together with scales is a ValueError.
def batch_gemm_qkv(x, norm_w, eps: float, w, q, kc, vc, pos, sin_t, cos_t, hq: int, hkv: int, hd: int, row_scale=None,
                   tiled: bool = False, plan=None, kv_dtype=None, ws=None, scales=None):
    """One bgemm_kernel launch with the q/k/v epilogue (fused RMSNorm, row scale, RoPE, K/V cache write): x [B, K]
    fp32, W [(hq + 2 hkv) hd, K] fp16 or int8; q [>= B, hq hd] fp32; kc / vc one layer's cache [B, hkv, T, hd] (f32, f16,
    or E4M3 codes with kv_dtype="f8"); pos int32 [B] on the device, 0 <= pos[b] < T. Returns the plan that ran."""
    B = x.shape[0]
    if kc.shape != vc.shape or kc.dtype != vc.dtype or kc.dim() != 4 or tuple(kc.shape[:2]) != (B, hkv) or kc.shape[3] != hd:
        raise ValueError("Tensor with Wrong Dim!")
    T = kc.shape[2]
    if q.dim() != 2 or q.shape[0] < B or q.shape[1] != hq * hd or sin_t.shape != (T, hd // 2) or cos_t.shape != (T, hd // 2):
        raise ValueError("Tensor with Wrong Dim!")
    if pos.dtype != torch.int32 or pos.numel() != B:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(q, kc, vc, pos, sin_t, cos_t)
    e = _lib.BgemmEpilogue(role=BG_ROLE_QKV, q=q.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(),
                           kv_dtype=_kv_dt(kc, kv_dtype), pos=pos.data_ptr(), sin_t=sin_t.data_ptr(),
                           cos_t=cos_t.data_ptr(), hq=hq, hkv=hkv, hd=hd, T=T)
    return _batch_gemm(x, norm_w, eps, w, row_scale, tiled, e, (hq + 2 * hkv) * hd, plan, ws, scales)


def batch_gemm_gate_up(x, norm_w, eps: float, w, act, act_mode: int = 0, row_scale=None, tiled: bool = False,
                       plan=None, ws=None, scales=None):
    """One bgemm_kernel launch with the gate/up epilogue: W [2 inter, K] = [gate; up]; act [>= B, inter] fp32 gets
    sigmoid(g) * u (act_mode 0) or SiLU(g) * u (1) of the RMS-normalised x. Returns the plan that ran."""
    inter = w.shape[0] // 2
    if act.dim() != 2 or act.shape[0] < x.shape[0] or act.shape[1] != inter or act.dtype != torch.float32:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(act)
    e = _lib.BgemmEpilogue(role=BG_ROLE_GATE_UP, act=act.data_ptr(), inter=inter, act_mode=act_mode)
    return _batch_gemm(x, norm_w, eps, w, row_scale, tiled, e, 2 * inter, plan, ws, scales)


def batch_gemm_store(x, w, y, resid=None, scale: float = 1.0, row_scale=None, tiled: bool = False, plan=None, ws=None,
                     scales=None):
    """One bgemm_kernel launch with the wo / down epilogue: y [>= B, ld] = (resid or 0) + (W x) * row scale * scale for
    the W.shape[0] rows; resid [B, ld] may be y itself. Returns the plan that ran."""
    if y.dim() != 2 or y.shape[0] < x.shape[0] or y.dtype != torch.float32 or (resid is not None and resid.shape != y.shape):
        raise ValueError("Tensor with Wrong Dim!")
    _dev(y, resid)
    e = _lib.BgemmEpilogue(role=BG_ROLE_STORE, y=y.data_ptr(), resid=resid.data_ptr() if resid is not None else None,
                           scale=scale, nrows=w.shape[0], ld=y.shape[1])
    return _batch_gemm(x, None, 0.0, w, row_scale, tiled, e, w.shape[0], plan, ws, scales)


def batch_gemm_logits(x, norm_w, eps: float, w, logits, keys_out, vocab_off: int = 0, row_scale=None,
                      tiled: bool = False, plan=None, ws=None, scales=None):
    """One bgemm_kernel launch with the LM-head epilogue: logits [>= B, ld] fp32 of the RMS-normalised x and, in keys_out
    [>= B, key_ld] (int64 holding the uint64 keys), each workgroup group's largest argmax key per sequence. Returns
    the plan that ran."""
    if logits.dim() != 2 or logits.shape[0] < x.shape[0] or logits.dtype != torch.float32:
        raise ValueError("Tensor with Wrong Dim!")
    if keys_out.dim() != 2 or keys_out.shape[0] < x.shape[0] or keys_out.dtype != torch.int64:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(logits, keys_out)
    e = _lib.BgemmEpilogue(role=BG_ROLE_LOGITS, logits=logits.data_ptr(), keys_out=keys_out.data_ptr(),
                           nrows=w.shape[0], ld=logits.shape[1], vocab_off=vocab_off, key_ld=keys_out.shape[1])
    return _batch_gemm(x, norm_w, eps, w, row_scale, tiled, e, w.shape[0], plan, ws, scales)


GV_ROLE_QKV, GV_ROLE_GATE_UP, GV_ROLE_WO, GV_ROLE_DOWN, GV_ROLE_LOGITS = 0, 1, 2, 3, 4


def _gv_plan_dict(p):
    return {n: getattr(p, n) for n, _ in p._fields_}


def decode_gemv_plan(role: int, w_dtype: int, cols: int, cus: int = 0, norm=None, **shape):
    """The schedule sli_decode_gemv would run (sli_gemv_plan as a dict), nothing launched; no device is needed when
    cus != 0. shape: the integer fields of sli_gemv_epilogue the role reads (hq, hkv, hd, T, kv_dtype, inter, act_mode,
    nrows, np, max_splits, ppwg, ks, key_ld, vocab_off); merged=True stands for a non-null `part` (wo). norm: whether a
    norm weight is passed (default: as the role requires)."""
    merged = shape.pop("merged", False) or shape.get("ks", 1) > 1
    e = _lib.GemvEpilogue(role=role, **shape)
    if merged:
        e.part = 16  # only its presence is read
    if norm is None:
        norm = role in (GV_ROLE_QKV, GV_ROLE_GATE_UP, GV_ROLE_LOGITS)
    p = _lib.GemvPlan(cus=cus)
    call("sli_decode_gemv_plan", w_dtype, cols, int(norm), ctypes.byref(e), ctypes.byref(p))
    return _gv_plan_dict(p)


def _decode_gemv(x, norm_w, eps, w, row_scale, scales, epi, rows, cus):
    """sli_decode_gemv / sli_decode_gemv_mxfp4 (scales given: w is the uint8 data [rows, cols / 2]). Returns the plan
    that ran as a dict."""
    mx = scales is not None
    if mx:
        if row_scale is not None:
            raise ValueError("MXFP4 weights have block scales, not a row scale: pass scales or row_scale, not both")
        cols = w.shape[1] * 2
        if w.dtype != torch.uint8 or scales.dtype != torch.uint8 or w.shape[0] != rows or cols % 32 or \
                scales.shape != (rows, cols // 32):
            raise ValueError("Tensor with Wrong Dim!")
    else:
        cols = w.shape[1]
        if w.dim() != 2 or w.shape[0] != rows or w.dtype not in (torch.float32, torch.float16, torch.int8):
            raise ValueError("Tensor with Wrong Dim!")
        if row_scale is not None and (row_scale.numel() != rows or row_scale.dtype != torch.float32):
            raise ValueError("Tensor with Wrong Dim!")
    for t in (x, norm_w):
        if t is not None and t.dtype != torch.float32:
            raise ValueError("Tensor with Wrong Dim!")
    _dev(x, norm_w, w, row_scale, scales)
    p = _lib.GemvPlan(cus=cus)
    if mx:
        call("sli_decode_gemv_mxfp4", _p(x), _p(norm_w), eps, _p(w), _p(scales), cols, ctypes.byref(epi), ctypes.byref(p),
             _s())
    else:
        call("sli_decode_gemv", _p(x), _p(norm_w), eps, _p(w), _DT[w.dtype], _p(row_scale), cols, ctypes.byref(epi),
             ctypes.byref(p), _s())
    return _gv_plan_dict(p)


def _gv_cols(w, scales):
    return w.shape[1] * (2 if scales is not None else 1)


# With `scales` given, every decode_gemv_* below runs MXFP4 weights, as the batch_gemm_* wrappers do. cus: sli_gemv_plan.
def decode_gemv_qkv(x, norm_w, eps: float, w, q, kc, vc, pos, sin_t, cos_t, hq: int, hkv: int, hd: int, row_scale=None,
                    scales=None, kv_dtype=None, cus: int = 0):
    """One batch-1 q/k/v GEMV launch (fused RMSNorm, row scale, RoPE, K/V cache write): x [K] fp32, W [(hq + 2 hkv) hd,
    K]; q [hq hd] fp32; kc / vc one layer's cache [hkv, T, hd]; pos int32 [1] on the device, 0 <= pos < T."""
    if kc.shape != vc.shape or kc.dtype != vc.dtype or kc.dim() != 3 or kc.shape[0] != hkv or kc.shape[2] != hd:
        raise ValueError("Tensor with Wrong Dim!")
    T = kc.shape[1]
    K = _gv_cols(w, scales)
    if x.numel() != K or norm_w.numel() != K or q.numel() != hq * hd or q.dtype != torch.float32 or \
            sin_t.shape != (T, hd // 2) or cos_t.shape != (T, hd // 2) or pos.dtype != torch.int32 or pos.numel() != 1:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(q, kc, vc, pos, sin_t, cos_t)
    e = _lib.GemvEpilogue(role=GV_ROLE_QKV, q=q.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(),
                          kv_dtype=_kv_dt(kc, kv_dtype), pos=pos.data_ptr(), sin_t=sin_t.data_ptr(),
                          cos_t=cos_t.data_ptr(), hq=hq, hkv=hkv, hd=hd, T=T)
    return _decode_gemv(x, norm_w, eps, w, row_scale, scales, e, (hq + 2 * hkv) * hd, cus)


def decode_gemv_gate_up(x, norm_w, eps: float, w, act, act_mode: int = 0, parts=None, row_scale=None, scales=None,
                        cus: int = 0):
    """One batch-1 gate/up GEMV launch: W [2 inter, K] = [gate; up]; act [inter] fp32. parts [np, K] (np 2 or 4): the
    staged input is x + parts[0] + ... (the K-split wo's consumer), then normalised."""
    inter = w.shape[0] // 2
    K = _gv_cols(w, scales)
    if x.numel() != K or norm_w.numel() != K or act.numel() < inter or act.dtype != torch.float32:
        raise ValueError("Tensor with Wrong Dim!")
    if parts is not None and (parts.dim() != 2 or parts.shape[1] != K or parts.dtype != torch.float32):
        raise ValueError("Tensor with Wrong Dim!")
    _dev(act, parts)
    e = _lib.GemvEpilogue(role=GV_ROLE_GATE_UP, act=act.data_ptr(), inter=inter, act_mode=act_mode,
                          parts=parts.data_ptr() if parts is not None else None,
                          np=parts.shape[0] if parts is not None else 0)
    return _decode_gemv(x, norm_w, eps, w, row_scale, scales, e, 2 * inter, cus)


def decode_gemv_wo(w, y=None, x=None, resid=None, part=None, pos=None, ppwg: int = 0, hd: int = 0, ks: int = 1,
                   kpart=None, row_scale=None, scales=None, cus: int = 0):
    """One batch-1 wo GEMV launch. x given: a plain input, y [>= nrows] = (resid or 0) + W x. part [heads, max_splits,
    hd + 4] given (with pos int32 [1], ppwg, hd): the input is merged from the attention's split partials. ks 2 or 4:
    the K-split launch, kpart [ks, nrows] gets the per-column-block sums and y / resid are not used."""
    nrows = w.shape[0]
    K = _gv_cols(w, scales)
    e = _lib.GemvEpilogue(role=GV_ROLE_WO, nrows=nrows, ks=ks)
    if part is not None:
        if part.dim() != 3 or part.dtype != torch.float32 or part.shape[2] != hd + 4 or part.shape[0] * hd != K or \
                pos is None or pos.dtype != torch.int32 or pos.numel() != 1 or x is not None:
            raise ValueError("Tensor with Wrong Dim!")
        e.part, e.pos, e.max_splits, e.ppwg, e.hq, e.hd = part.data_ptr(), pos.data_ptr(), part.shape[1], ppwg, \
            part.shape[0], hd
    elif x is None or x.numel() != K:
        raise ValueError("Tensor with Wrong Dim!")
    if ks > 1:
        if kpart is None or kpart.shape != (ks, nrows) or kpart.dtype != torch.float32:
            raise ValueError("Tensor with Wrong Dim!")
        e.kpart = kpart.data_ptr()
    else:
        if y is None or y.numel() < nrows or y.dtype != torch.float32 or (resid is not None and resid.numel() < nrows):
            raise ValueError("Tensor with Wrong Dim!")
        e.y = y.data_ptr()
        e.resid = resid.data_ptr() if resid is not None else None
    _dev(y, resid, part, pos, kpart)
    return _decode_gemv(x, None, 0.0, w, row_scale, scales, e, nrows, cus)


def decode_gemv_down(x, w, y, resid=None, parts=None, row_scale=None, scales=None, cus: int = 0):
    """One batch-1 down GEMV launch: y [>= nrows] = (resid or 0) + W x; parts [np, nrows] (np 2 or 4): the residual
    is resid + parts[0] + ... in that order (the K-split wo's consumer)."""
    nrows = w.shape[0]
    if x.numel() != _gv_cols(w, scales) or y.numel() < nrows or y.dtype != torch.float32 or \
            (resid is not None and resid.numel() < nrows):
        raise ValueError("Tensor with Wrong Dim!")
    if parts is not None and (parts.dim() != 2 or parts.shape[1] != nrows or parts.dtype != torch.float32):
        raise ValueError("Tensor with Wrong Dim!")
    _dev(y, resid, parts)
    e = _lib.GemvEpilogue(role=GV_ROLE_DOWN, y=y.data_ptr(), resid=resid.data_ptr() if resid is not None else None,
                          nrows=nrows, parts=parts.data_ptr() if parts is not None else None,
                          np=parts.shape[0] if parts is not None else 0)
    return _decode_gemv(x, None, 0.0, w, row_scale, scales, e, nrows, cus)


def decode_gemv_logits(x, norm_w, eps: float, w, logits, keys, vocab_off: int = 0, row_scale=None, scales=None,
                       cus: int = 0):
    """One batch-1 LM-head GEMV launch: logits [>= nrows] fp32 of the RMS-normalised x and, in keys [key_ld] (int64
    holding the uint64 keys), each workgroup's largest argmax key."""
    nrows = w.shape[0]
    K = _gv_cols(w, scales)
    if x.numel() != K or norm_w.numel() != K or logits.numel() < nrows or logits.dtype != torch.float32 or \
            keys.dtype != torch.int64 or keys.dim() != 1:
        raise ValueError("Tensor with Wrong Dim!")
    _dev(logits, keys)
    e = _lib.GemvEpilogue(role=GV_ROLE_LOGITS, logits=logits.data_ptr(), keys=keys.data_ptr(), nrows=nrows,
                          vocab_off=vocab_off, key_ld=keys.numel())
    return _decode_gemv(x, norm_w, eps, w, row_scale, scales, e, nrows, cus)


def argmax(logits, out=None):
    """argmaxLayer::forward (argmax.cpp:7-17) on device: first index of the maximum."""
    out = torch.empty(1, device=logits.device, dtype=torch.int32) if out is None else out
    _dev(logits, out)
    call("sli_argmax", _p(logits), logits.numel(), _p(out), _s())
    return out


def sample(logits, temperature: float, top_k: int, top_p: float, seed: int, pos, seq0: int = 0, out=None):
    """sli_sample: one seeded temperature / top-k / top-p draw per row (the rule: sli.h). logits [V] or [rows, V]
    fp32, the rows ``logits.stride(0)`` floats apart (a row-padded view, or an ``expand``-ed row with stride 0: many
    draws from one distribution). pos: int32 device tensor [rows] (spaced ``pos.stride(0)``), row r drawing as sequence
    seq0 + r at position pos[r]. Returns the int32 tokens [rows]."""
    if logits.dim() == 1:
        logits = logits.unsqueeze(0)
    rows, vocab = logits.shape
    if not logits.is_cuda or logits.dtype != torch.float32 or (vocab > 1 and logits.stride(1) != 1):
        raise ValueError("logits: fp32 device rows of contiguous elements")
    if not pos.is_cuda or pos.dtype != torch.int32 or pos.dim() != 1 or pos.shape[0] < rows:
        raise ValueError("pos: an int32 device tensor of one position per row")
    out = torch.empty(rows, device=logits.device, dtype=torch.int32) if out is None else out
    _dev(out)
    prm = _lib.Sampling(temperature, top_k, top_p, seed & 0xFFFFFFFF)
    call("sli_sample", _p(logits), logits.stride(0) if rows > 1 else vocab, rows, vocab, ctypes.byref(prm), seq0,
         _p(pos), pos.stride(0) if rows > 1 else 1, _p(out), _s())
    return out


def gen_params(temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, min_p: float = 0.0,
               repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
               penalty_from: int = 0, max_pos: int = 0, stop=()) -> "_lib.GenParams":
    """One sli_gen_params block (the defaults: greedy, no penalties, no stop)."""
    stop = [int(t) for t in stop]
    if len(stop) > _lib.MAX_STOP:
        raise ValueError(f"at most {_lib.MAX_STOP} stop tokens")
    return _lib.GenParams(temperature, top_k, top_p, seed & 0xFFFFFFFF, min_p, repetition_penalty, presence_penalty,
                          frequency_penalty, penalty_from, max_pos, len(stop),
                          (ctypes.c_int32 * _lib.MAX_STOP)(*stop))


def sample_gen(logits, params, pos, hist=None, seq0: int = 0, out=None):
    """sli_sample_gen: ops.sample with one parameter block per row (``params``: a list of gen_params() blocks or of
    dicts of its keywords) and the rows' token histories (``hist``: int32 device tensor [rows, n], tokens by position;
    needed iff a row has an active penalty). Returns the int32 tokens [rows]; -1 for a row with temperature 0 and no
    penalty, whose token is the argmax."""
    if logits.dim() == 1:
        logits = logits.unsqueeze(0)
    rows, vocab = logits.shape
    if not logits.is_cuda or logits.dtype != torch.float32 or (vocab > 1 and logits.stride(1) != 1):
        raise ValueError("logits: fp32 device rows of contiguous elements")
    if not pos.is_cuda or pos.dtype != torch.int32 or pos.dim() != 1 or pos.shape[0] < rows:
        raise ValueError("pos: an int32 device tensor of one position per row")
    if len(params) != rows:
        raise ValueError("one parameter block per row")
    blocks = (_lib.GenParams * rows)(*[p if isinstance(p, _lib.GenParams) else gen_params(**p) for p in params])
    hp, hs = None, 0
    if hist is not None:
        if hist.dim() == 1:
            hist = hist.unsqueeze(0)
        if not hist.is_cuda or hist.dtype != torch.int32 or hist.shape[0] < rows or \
                (hist.shape[1] > 1 and hist.stride(1) != 1) or (rows > 1 and hist.stride(0) != hist.shape[1]):
            raise ValueError("hist: an int32 device tensor [rows, n] of contiguous rows")
        hp, hs = _p(hist), hist.shape[1]
    out = torch.empty(rows, device=logits.device, dtype=torch.int32) if out is None else out
    _dev(out)
    call("sli_sample_gen", _p(logits), logits.stride(0) if rows > 1 else vocab, rows, vocab, blocks, seq0,
         _p(pos), pos.stride(0) if rows > 1 else 1, hp, hs, _p(out), _s())
    return out

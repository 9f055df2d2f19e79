"""Building blocks of the HIP training towers (model/train_tower.py,
model/t5_train_tower.py): the one place that states how they call the library.

The training step of run_random_sampling.py (DRT/trainer/trainer.py:113-133) differentiates
HF ``BertModel`` under autograd; these functions restate the gradients of its ops on the HIP
kernels for the bf16 activations the HIP forward stores:

* ``linear_backward``   nn.Linear: dX = dY W (the NT GEMM against a transposed weight copy),
                        dW = dY^T X (``wgrad``: the TN GEMM reading both token-major operands
                        directly, deterministic split over tokens, fp32 output), db = column
                        sums of dY;
* ``layernorm_backward`` / ``gelu_backward``: thin wrappers of the C-ABI entries
                        (include/drt.h);
* ``linear`` / ``dropout`` / ``attention_forward`` / ``attention_backward``: the forward GEMM with
                        its training epilogues, the hashed dropout, and the attention pair with
                        its optional relative-position bias, dropout and bias / table gradients.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _native

LIN_GELU = 1   # drt_linear_bf16* flag bit 0


def _ws(nbytes: int, dev) -> Optional[torch.Tensor]:
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev) if nbytes else None


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def transpose_bf16(x: torch.Tensor, cols_pad: int = 0) -> torch.Tensor:
    """x [R, C] bf16 -> x^T [C, R + pad] with zero padding columns (k-contiguous GEMM operand)."""
    lib = _native.load()
    R, C = x.shape
    y = torch.empty((C, R + cols_pad), dtype=torch.bfloat16, device=x.device)
    if cols_pad:
        y[:, R:].zero_()
    _native.check(lib.drt_transpose_bf16_ld(x.data_ptr(), R, C, y.data_ptr(), R + cols_pad,
                                            _native.stream_ptr(x.device)), "drt_transpose_bf16_ld")
    return y


def linear(x, w, out, bias=None, resid=None, flags=0, pre_out=None, drop=None):
    """out = act(x W^T + bias) (+ resid), ``flags`` as drt_linear_bf16 takes them (bit 0 GELU, bit 3
    ReLU); ``pre_out``: also store the pre-activation (GELU); ``drop`` = (p, seed, site):
    out = dropout(x W^T + bias) + resid in the GEMM epilogue, which needs a bias
    (drt_linear_bf16_ex)."""
    lib = _native.load()
    s = _native.stream_ptr(x.device)
    m, k = x.shape
    n = w.shape[0]
    flags |= 2 if out.dtype == torch.float32 else 0   # bit 1: fp32 output, from ``out`` itself
    nb = int(lib.drt_linear_workspace(m, n, k))
    ws = _ws(nb, x.device)
    if pre_out is not None or drop is not None:
        p, seed, site = drop if drop is not None else (0.0, 0, 0)
        _native.check(lib.drt_linear_bf16_ex(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(resid), None, out.data_ptr(),
                                             _ptr(pre_out), m, n, k, flags | (4 if drop is not None else 0), float(p),
                                             seed, site, _ptr(ws), nb, s), "drt_linear_bf16_ex")
        return out
    _native.check(lib.drt_linear_bf16_ws(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(resid), out.data_ptr(), m, n, k,
                                         flags, _ptr(ws), nb, s), "drt_linear_bf16_ws")
    return out


def dropout(y, p, seed, site, resid=None):
    """dropout(y) (+ resid) with the mask of (p, seed, site); on a gradient, the dropout backward."""
    out = torch.empty_like(y)
    _native.check(_native.load().drt_dropout_add_bf16(y.data_ptr(), _ptr(resid), y.numel(), float(p), seed, site,
                                                      out.data_ptr(), _native.stream_ptr(y.device)),
                  "drt_dropout_add_bf16")
    return out


def attention_forward(qkv, mask, B, L, heads, scale, relbias=None, drop=None):
    """(ctx bf16 [B*L, heads*64], lse fp32 [B, heads, L], keep bits or None) of the attention over the
    packed ``qkv``; ``relbias`` fp32 [heads, 2L-1] (T5); ``drop`` = (p, seed, site) with p > 0:
    dropout of the probabilities, the keep mask kept as bits (B * heads * L * L / 8 bytes) for the
    backward to read."""
    dev = qkv.device
    ctx = torch.empty((B * L, heads * 64), dtype=torch.bfloat16, device=dev)
    lse = torch.empty((B, heads, L), dtype=torch.float32, device=dev)
    p, seed, site = drop if drop is not None else (0.0, 0, 0)
    bits = torch.empty((B, heads, L, (L + 31) // 32), dtype=torch.int32, device=dev) if p > 0 else None
    _native.check(_native.load().drt_attention_forward_bf16(
        qkv.data_ptr(), _ptr(mask), _ptr(relbias), ctx.data_ptr(), lse.data_ptr(), _ptr(bits), B, L, heads, 64,
        float(scale), float(p), seed, site, _native.stream_ptr(dev)), "drt_attention_forward_bf16")
    return ctx, lse, bits


def attention_backward(qkv, ctx, dctx, lse, mask, bits, B, L, heads, scale, relbias=None, drop=None,
                       want_dbias=False):
    """(dqkv bf16 like qkv, extra) of ``attention_forward``: extra = dtable fp32 [heads, 2L-1] with
    ``relbias``, dbias fp32 [3 * heads * 64] (the q / k / v bias gradients, without a pass over dqkv)
    with ``want_dbias`` (BERT; not with ``relbias``), else None."""
    lib = _native.load()
    dev = qkv.device
    dqkv = torch.empty_like(qkv)
    p, seed, site = drop if drop is not None else (0.0, 0, 0)
    rb = relbias is not None
    shape = (heads, 2 * L - 1) if rb else (3 * heads * 64,) if want_dbias else None
    extra = torch.empty(shape, dtype=torch.float32, device=dev) if shape else None
    nb = int(lib.drt_attention_backward_workspace(B, L, heads, 64, int(rb))) if shape else 0
    ws = _ws(nb, dev)
    dbias, dtable = (None, extra) if rb else (extra, None)
    _native.check(lib.drt_attention_backward_bf16(
        qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), _ptr(mask), _ptr(relbias), _ptr(bits),
        dqkv.data_ptr(), B, L, heads, 64, float(scale), float(p), seed, site, _ptr(dbias), _ptr(dtable), _ptr(ws), nb,
        _native.stream_ptr(dev)), "drt_attention_backward_bf16")
    return dqkv, extra


def attention_varlen_forward(qkv, plan, heads, scale, drop=None, per_class=False):
    """(ctx bf16 [rows, heads*64], lse fp32 [heads, T], keep bits [heads, T, W] or None) of the attention
    over the packed ``qkv`` [rows >= T, 3 heads*64] of ``plan`` (model/packing.py); rows past T of ctx
    are zeros.  ``drop`` = (p, seed, site): the keeps of every real (query, key) are those of
    ``attention_forward`` on the padded batch [B, plan.L]."""
    dev = qkv.device
    lib = _native.load()
    rows, T = qkv.shape[0], plan.T
    ctx = torch.empty((rows, heads * 64), dtype=torch.bfloat16, device=dev)
    if rows > T:
        ctx[T:].zero_()
    lse = torch.empty((heads, T), dtype=torch.float32, device=dev)
    p, seed, site = drop if drop is not None else (0.0, 0, 0)
    W = (plan.max_len + 31) // 32
    bits = torch.empty((heads, T, W), dtype=torch.int32, device=dev) if p > 0 else None
    s = _native.stream_ptr(dev)
    for sp, n, ml in plan.launches(per_class):
        _native.check(lib.drt_attention_varlen_train_forward_bf16(
            qkv.data_ptr(), plan.cu_seqlens.data_ptr(), sp, n, ml, plan.L, T, W, ctx.data_ptr(), lse.data_ptr(),
            _ptr(bits), heads, 64, float(scale), float(p), seed, site, s), "drt_attention_varlen_train_forward_bf16")
    return ctx, lse, bits


def attention_varlen_backward(qkv, ctx, dctx, lse, bits, plan, heads, scale, drop=None, per_class=False):
    """(dqkv bf16 like qkv with zero rows past T, dbias fp32 [3 * heads * 64]) of
    ``attention_varlen_forward``.  Every launch leaves its sequences' column sums in one [B, 3H]
    matrix; one fixed-order column sum after the last launch finishes dbias."""
    lib = _native.load()
    dev = qkv.device
    rows, T = qkv.shape[0], plan.T
    dqkv = torch.empty_like(qkv)
    if rows > T:
        dqkv[T:].zero_()
    n3 = 3 * heads * 64
    dsum = torch.zeros((plan.B, n3), dtype=torch.float32, device=dev)
    p, seed, site = drop if drop is not None else (0.0, 0, 0)
    W = (plan.max_len + 31) // 32
    s = _native.stream_ptr(dev)
    for sp, n, ml in plan.launches(per_class):
        _native.check(lib.drt_attention_varlen_backward_bf16(
            qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), plan.cu_seqlens.data_ptr(), sp, n, ml,
            plan.L, T, W, _ptr(bits), dqkv.data_ptr(), dsum.data_ptr(), heads, 64, float(scale), float(p), seed, site,
            s), "drt_attention_varlen_backward_bf16")
    dbias = torch.empty(n3, dtype=torch.float32, device=dev)
    nb = int(lib.drt_colsum_workspace(plan.B, n3))
    ws = _ws(nb, dev)
    _native.check(lib.drt_colsum_f32(dsum.data_ptr(), plan.B, n3, dbias.data_ptr(), _ptr(ws), nb, s), "drt_colsum_f32")
    return dqkv, dbias


def pack_rows(padded, plan, rows=None):
    """[rows, H] bf16 (rows >= T, default T): the real rows of ``padded`` [B * L, H] in packed order,
    zeros past T -- the inverse of ``unpack_rows`` and its backward."""
    H = padded.shape[-1]
    rows = plan.T if rows is None else rows
    out = torch.empty((rows, H), dtype=torch.bfloat16, device=padded.device)
    _native.check(_native.load().drt_pack_rows_bf16(padded.data_ptr(), plan.cu_seqlens.data_ptr(), plan.B, plan.L, H,
                                                    out.data_ptr(), rows, _native.stream_ptr(padded.device)),
                  "drt_pack_rows_bf16")
    return out


def unpack_rows(packed, plan):
    """[B * L, H] bf16 from the packed rows [>= T, H]: zeros at the pad positions."""
    H = packed.shape[-1]
    out = torch.empty((plan.B * plan.L, H), dtype=torch.bfloat16, device=packed.device)
    _native.check(_native.load().drt_unpack_rows_bf16(packed.data_ptr(), plan.cu_seqlens.data_ptr(), plan.B, plan.L, H,
                                                      out.data_ptr(), _native.stream_ptr(packed.device)),
                  "drt_unpack_rows_bf16")
    return out


def grads_out(names, grads):
    """The autograd nodes' return for the parameters ``names``: fp32 gradients, None where absent."""
    return tuple(grads[n].to(torch.float32) if n in grads else None for n in names)


def colsum(x: torch.Tensor) -> torch.Tensor:
    lib = _native.load()
    M, N = x.shape
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    nb = int(lib.drt_colsum_workspace(M, N))
    ws = _ws(nb, x.device)
    _native.check(lib.drt_colsum_bf16(x.data_ptr(), M, N, out.data_ptr(), _ptr(ws), nb,
                                      _native.stream_ptr(x.device)), "drt_colsum_bf16")
    return out


def linear_backward(dy: torch.Tensor, x: torch.Tensor, w_t: torch.Tensor, want_dx: bool = True,
                    resid: Optional[torch.Tensor] = None, gelu_pre: Optional[torch.Tensor] = None,
                    db: Optional[torch.Tensor] = None, dx_colsum: Optional[torch.Tensor] = None,
                    want_db: bool = True) -> Tuple[Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor]]:
    """Gradients of y = x W^T + b (nn.Linear, W [N, K]) for dy [T, N], x [T, K] (bf16 CUDA),
    given w_t = W^T [K, N] bf16.  Returns (dx bf16 [T, K] or None, dW fp32 [N, K], db fp32 [N]);
    ``resid`` [T, K] bf16 is added to dx in the dgrad GEMM's epilogue (a residual branch);
    ``gelu_pre`` [T, K] (x = GELU(gelu_pre)) makes dx the gradient of gelu_pre instead, the GELU
    backward applied in the same epilogue (drt_linear_bf16_ex); ``db``: the bias gradient already
    produced by dy's producer (the LayerNorm / attention backward), returned as is instead of a
    column-sum pass over dy.  ``dx_colsum`` [K] fp32 (with ``gelu_pre``): also filled with the column
    sums of dx -- the bias gradient of the GELU's linear -- from the dgrad GEMM's epilogue
    (drt_linear_dgelu_bias_bf16).  ``want_db`` False (a linear without a bias): db is None."""
    lib = _native.load()
    dev = dy.device
    s = _native.stream_ptr(dev)
    T, N = dy.shape
    K = x.shape[1]
    if N % 64 or K % 64:
        raise ValueError("linear_backward: feature sizes must be multiples of 64")
    dx = None
    if want_dx:
        dx = torch.empty((T, K), dtype=torch.bfloat16, device=dev)
        nb = int(lib.drt_linear_workspace(T, K, N))
        ws = _ws(nb, dev)
        if gelu_pre is not None and dx_colsum is not None:
            if resid is not None:
                raise ValueError("linear_backward: gelu_pre and resid are exclusive")
            nb = int(lib.drt_linear_dgelu_bias_workspace(T, K, N))
            ws = _ws(nb, dev)
            _native.check(lib.drt_linear_dgelu_bias_bf16(dy.data_ptr(), w_t.data_ptr(), gelu_pre.data_ptr(),
                                                         dx.data_ptr(), T, K, N, dx_colsum.data_ptr(), _ptr(ws), nb,
                                                         s), "dgrad (GELU backward + bias gradient epilogue)")
        elif gelu_pre is not None:
            if resid is not None:
                raise ValueError("linear_backward: gelu_pre and resid are exclusive")
            _native.check(lib.drt_linear_bf16_ex(dy.data_ptr(), w_t.data_ptr(), None, None, gelu_pre.data_ptr(),
                                                 dx.data_ptr(), None, T, K, N, 0, 0.0, 0, 0, _ptr(ws), nb, s),
                          "dgrad (GELU backward epilogue)")
        else:
            _native.check(lib.drt_linear_bf16_ws(dy.data_ptr(), w_t.data_ptr(), None, _ptr(resid), dx.data_ptr(), T, K,
                                                 N, 0, _ptr(ws), nb, s), "dgrad")
    dW = wgrad(dy, x)
    if not want_db:
        return dx, dW, None
    return dx, dW, (db if db is not None else colsum(dy))


WGRAD_TN = True   # A/B switch: False = transposed operand copies + NT GEMM (the round-1 path)


def wgrad(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """dW [N, K] fp32 = dy[T, N]^T x[T, K].  Token counts that are multiples of 32 go straight to
    the TN GEMM (drt_linear_wgrad_bf16, no transposed copies); others transpose both operands
    (zero-padded to 64 tokens) and run the NT GEMM."""
    lib = _native.load()
    dev = dy.device
    s = _native.stream_ptr(dev)
    T, N = dy.shape
    K = x.shape[1]
    dW = torch.empty((N, K), dtype=torch.float32, device=dev)
    if WGRAD_TN and T % 32 == 0:
        nb = int(lib.drt_linear_wgrad_workspace(T, N, K))
        ws = _ws(nb, dev)
        _native.check(lib.drt_linear_wgrad_bf16(dy.data_ptr(), x.data_ptr(), dW.data_ptr(), T, N, K, _ptr(ws), nb, s),
                      "drt_linear_wgrad_bf16")
        return dW
    pad = (-T) % 64
    dyT = transpose_bf16(dy, pad)        # [N, T64]
    xT = transpose_bf16(x, pad)          # [K, T64]
    T64 = T + pad
    nb = int(lib.drt_linear_workspace(N, K, T64))
    ws = _ws(nb, dev)
    _native.check(lib.drt_linear_bf16_ws(dyT.data_ptr(), xT.data_ptr(), None, None, dW.data_ptr(), N, K, T64, 2,
                                         _ptr(ws), nb, s), "wgrad")
    return dW


def layernorm_backward(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, eps: float,
                       dres: Optional[torch.Tensor] = None, drop=None, want_sum: bool = False):
    """(dx bf16 [M, H], dgamma fp32 [H], dbeta fp32 [H]) of out = LN(x) (x = the bf16 pre-LN sums).
    ``drop`` = (p, seed, site): also return dropout(dx) with that mask as a fourth value.
    ``want_sum``: also return (last) the column sums of the gradient handed down -- dropout(dx), or
    dx -- i.e. the bias gradient of the linear below."""
    lib = _native.load()
    M, H = x.shape
    dev = x.device
    dx = torch.empty((M, H), dtype=torch.bfloat16, device=dev)
    dg = torch.empty(H, dtype=torch.float32, device=dev)
    db = torch.empty(H, dtype=torch.float32, device=dev)
    nb = int(lib.drt_layernorm_bwd_workspace(M, H))
    ws = _ws(nb, dev)
    dxd = torch.empty_like(dx) if drop is not None else None
    p, seed, site = drop if drop is not None else (0.0, 0, 0)
    dsum = torch.empty(H, dtype=torch.float32, device=dev) if want_sum else None
    _native.check(lib.drt_layernorm_backward_bf16(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), float(eps), M, H,
                                                  _ptr(dres), dx.data_ptr(), _ptr(dxd), float(p), seed, site,
                                                  dg.data_ptr(), db.data_ptr(), _ptr(dsum), _ptr(ws), nb,
                                                  _native.stream_ptr(dev)), "drt_layernorm_backward_bf16")
    out = (dx, dg, db) + ((dxd,) if drop is not None else ()) + ((dsum,) if want_sum else ())
    return out


def gelu_backward(dy: torch.Tensor, pre: torch.Tensor) -> torch.Tensor:
    lib = _native.load()
    dx = torch.empty_like(dy)
    _native.check(lib.drt_gelu_bwd_bf16(dy.data_ptr(), pre.data_ptr(), dy.numel(), dx.data_ptr(),
                                        _native.stream_ptr(dy.device)), "drt_gelu_bwd_bf16")
    return dx

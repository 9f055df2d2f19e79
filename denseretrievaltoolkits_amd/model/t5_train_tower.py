"""Training forward + backward of a T5 encoder tower (HF ``T5EncoderModel``) on the HIP kernels.

The T5 counterpart of model/train_tower.py, opt-in through ``DRModel.hip_train_t5``: one
``torch.autograd.Function`` for the embedding, one per T5Block and one for the final norm, so each
block's parameter gradients reach autograd -- and DDP's bucketed all-reduce -- as soon as that
block's backward is done.  The forward runs the inference kernels of model/t5_encoder.py plus the
activations the backward needs, per block in bf16: the block input ``h``, its norm ``x0``, ``qkv``,
``ctx``, the attention LSE (fp32) and keep bits, ``h2`` (after attention), its norm ``x1``, the FFN
pre-activation(s) (gated-gelu: ``(a | b)`` of the one GEMM over [wi_0; wi_1]) and the activation as
``wo`` read it (after the inner dropout).  The backward chain per block, all on HIP kernels:

    dropout bwd -> wo linear bwd -> ReLU / gated gelu_new bwd (+ inner dropout) -> wi linear bwd
    -> RMSNorm bwd (+ d h2 residual) -> dropout bwd -> o linear bwd -> attention bwd with the
    relative-position bias (dQKV and dtable) -> QKV linear bwd -> RMSNorm bwd (+ residual)

then the embedding scatter-add, producing fp32 gradients for every HF parameter (QKV split back into
q / k / v, [wi_0; wi_1] into its halves).  The relative-position bias table [heads, 2L-1] is built
in torch with autograd attached (``weight[bucket].t()``) and enters every block node as a tensor
input; each block's backward returns its ``dtable`` and torch sums the blocks and folds the 2L-1
offsets into the buckets of ``relative_attention_bias.weight``.

Dropout as HF applies it in train mode (``dropout_rate`` at six sites: embedding output, attention
probabilities, attention output, FFN inner, FFN output, after the final norm), drawn from the
counter hash of csrc/drt_common.h as the BERT tower draws it (``t5_dropout_sites``); the seed comes
from torch's CPU generator.  Scope: what HipT5Encoder supports (d_kv 64, d_model a multiple of 256 up
to 1024, relu / gated-gelu) and L <= 512.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import _native
from .encoder_bwd import (_ptr, _ws, attention_backward, attention_forward, dropout, grads_out, linear,
                          linear_backward, transpose_bf16)
from .t5_encoder import LIN_RELU, T5Shape, _relative_buckets

MAX_TRAIN_SEQ = 512
SITE_EMBED, SITE_FINAL = 0, 1
REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def t5_tower_supported(model, L: Optional[int] = None) -> Optional[str]:
    """None if the HIP training tower can run this HF T5EncoderModel (at sequence length L), else
    the reason."""
    if type(model).__name__ != "T5EncoderModel":
        return f"{type(model).__name__} is not a T5EncoderModel"
    why = T5Shape.from_config(model.config).unsupported()
    if why is None and L is not None and L > MAX_TRAIN_SEQ:
        why = f"sequence length {L} > {MAX_TRAIN_SEQ}"
    return why


def t5_dropout_sites(block: int) -> Tuple[int, int, int, int]:
    """(attention probabilities, attention output, FFN inner, FFN output) site ids of a block;
    0 = embedding output, 1 = after the final norm."""
    return 4 * block + 2, 4 * block + 3, 4 * block + 4, 4 * block + 5


def relative_bias_table_grad(weight: torch.Tensor, L: int, num_buckets: int, max_distance: int) -> torch.Tensor:
    """``relative_bias_table`` with autograd attached: fp32 [heads, 2L-1], entry (h, k - q + L - 1) =
    weight[bucket(k - q), h]; a gradient on it folds back into ``weight`` through torch's indexing
    backward (buckets computed on the CPU, as ``relative_bias_table``)."""
    bucket = _relative_buckets(torch.arange(-(L - 1), L, dtype=torch.long), num_buckets, max_distance)
    return weight.float()[bucket.to(weight.device)].t().contiguous()


class _Weights:
    """bf16 copies (and transposes) of the tower's linears for one step; fp32 norm weights / table."""

    def __init__(self, model, dev):
        sd = dict(model.named_parameters())
        sh = T5Shape.from_config(model.config)
        gated = sh.act == "gated-gelu"

        def f32(n):
            return sd[n].detach().float().contiguous()

        def b16(*names):
            return torch.cat([sd[n].detach() for n in names], 0).to(torch.bfloat16).contiguous()

        tr = transpose_bf16   # [N, K] bf16 -> [K, N]

        self.layers = []
        for i in range(sh.layers):
            a = f"encoder.block.{i}.layer.0."
            f = f"encoder.block.{i}.layer.1."
            wi = [f + "DenseReluDense.wi_0.weight", f + "DenseReluDense.wi_1.weight"] if gated \
                else [f + "DenseReluDense.wi.weight"]
            wqkv, wo, wi_, wf = (b16(*(a + f"SelfAttention.{n}.weight" for n in "qkv")),
                                 b16(a + "SelfAttention.o.weight"), b16(*wi), b16(f + "DenseReluDense.wo.weight"))
            self.layers.append(dict(g0=f32(a + "layer_norm.weight"), wqkv=wqkv, wqkv_t=tr(wqkv), wo=wo, wo_t=tr(wo),
                                    g1=f32(f + "layer_norm.weight"), wi=wi_, wi_t=tr(wi_), wf=wf, wf_t=tr(wf),
                                    wi_names=wi))
        self.word = f32("shared.weight")
        self.final_g = f32("encoder.final_layer_norm.weight")


class _Step:
    """What every node of one tower pass shares: weights, shape, ids, mask, dropout (p, seed)."""

    def __init__(self, model, W: _Weights, ids, mask, drop):
        self.sh = T5Shape.from_config(model.config)
        self.W, self.ids, self.mask, self.drop = W, ids, mask, drop
        self.B, self.L = ids.shape
        self.dev = ids.device
        self.D, self.I, self.F = self.sh.d_model, self.sh.heads * self.sh.d_kv, self.sh.d_ff
        self.gated = self.sh.act == "gated-gelu"
        # the GEMM's dropout epilogue comes with a bias: T5's linears have none
        self.zero_bias = torch.zeros(self.D, dtype=torch.float32, device=self.dev) if drop[0] > 0 else None


def _rms(lib, x, g, eps, stream):
    out = torch.empty_like(x)
    _native.check(lib.drt_rmsnorm_bf16(x.data_ptr(), x.shape[0], x.shape[1], g.data_ptr(), eps, out.data_ptr(),
                                       stream), "drt_rmsnorm_bf16")
    return out


def rmsnorm_backward(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, eps: float,
                     dres: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx bf16 [M, H], dgamma fp32 [H]) of out = rmsnorm(x) * gamma; ``dres`` is added into dx."""
    lib = _native.load()
    M, H = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(H, dtype=torch.float32, device=x.device)
    nb = int(lib.drt_rmsnorm_bwd_workspace(M, H))
    ws = _ws(nb, x.device)
    _native.check(lib.drt_rmsnorm_bwd_bf16(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), float(eps), M, H,
                                           _ptr(dres), dx.data_ptr(), dg.data_ptr(), _ptr(ws), nb,
                                           _native.stream_ptr(x.device)), "drt_rmsnorm_bwd_bf16")
    return dx, dg


def embed_forward(st: _Step):
    lib = _native.load()
    s = _native.stream_ptr(st.dev)
    h = torch.empty((st.B * st.L, st.D), dtype=torch.bfloat16, device=st.dev)
    _native.check(lib.drt_t5_embed_bf16(st.ids.data_ptr(), st.B, st.L, st.W.word.data_ptr(), st.D, h.data_ptr(), s),
                  "drt_t5_embed_bf16")
    p, seed = st.drop
    return dropout(h, p, seed, SITE_EMBED) if p > 0 else h


def embed_backward(st: _Step, d) -> torch.Tensor:
    lib = _native.load()
    s = _native.stream_ptr(st.dev)
    p, seed = st.drop
    if p > 0:
        d = dropout(d, p, seed, SITE_EMBED)
    dword = torch.zeros_like(st.W.word)
    _native.check(lib.drt_t5_embedding_bwd(st.ids.data_ptr(), d.data_ptr(), st.B, st.L, st.D, int(dword.shape[0]),
                                           dword.data_ptr(), s), "drt_t5_embedding_bwd")
    return dword


def block_forward(st: _Step, i: int, h, table):
    """One T5Block (train-mode dropout as HF) -> (h_out, saved activations)."""
    lib = _native.load()
    dev, sh = st.dev, st.sh
    s = _native.stream_ptr(dev)
    ly = st.W.layers[i]
    B, L, T = st.B, st.L, st.B * st.L
    p, seed = st.drop
    s_att, s_out1, s_inner, s_out2 = t5_dropout_sites(i)

    def buf(n):
        return torch.empty((T, n), dtype=torch.bfloat16, device=dev)

    x0 = _rms(lib, h, ly["g0"], sh.eps, s)
    qkv = linear(x0, ly["wqkv"], buf(3 * st.I))
    ctx, lse, bits = attention_forward(qkv, st.mask, B, L, sh.heads, 1.0, relbias=table, drop=(p, seed, s_att))
    # h2 = dropout(ctx Wo^T) + h, the dropout in the GEMM epilogue
    h2 = linear(ctx, ly["wo"], buf(st.D), bias=st.zero_bias, resid=h, drop=(p, seed, s_out1) if p > 0 else None)
    x1 = _rms(lib, h2, ly["g1"], sh.eps, s)
    if st.gated:
        pre = linear(x1, ly["wi"], buf(2 * st.F))
        f = buf(st.F)
        _native.check(lib.drt_gated_gelu_new_bf16(pre.data_ptr(), T, st.F, f.data_ptr(), s), "drt_gated_gelu_new_bf16")
    else:
        pre = None
        f = linear(x1, ly["wi"], buf(st.F), flags=LIN_RELU)
    fd = dropout(f, p, seed, s_inner) if p > 0 else f   # what wo reads
    out = linear(fd, ly["wf"], buf(st.D), bias=st.zero_bias, resid=h2, drop=(p, seed, s_out2) if p > 0 else None)
    # the gated backward reads its pre-activations; ReLU's only the sign of f, and where the inner
    # dropout zeroed fd the gradient is dropped anyway: fd serves
    return out, (h, x0, qkv, ctx, lse, bits, h2, x1, pre, fd)


def block_backward(st: _Step, i: int, saved, table, d):
    """(d h_in, dtable, fp32 gradients of block i's parameters by HF name) for d h_out."""
    lib = _native.load()
    sh = st.sh
    s = _native.stream_ptr(st.dev)
    h, x0, qkv, ctx, lse, bits, h2, x1, pre, fd = saved
    ly = st.W.layers[i]
    T = st.B * st.L
    p, seed = st.drop
    s_att, s_out1, s_inner, s_out2 = t5_dropout_sites(i)
    # out = h2 + dropout(fd Wf^T)
    dy2 = dropout(d, p, seed, s_out2) if p > 0 else d
    dfd, dwf, _ = linear_backward(dy2, fd, ly["wf_t"], want_db=False)
    if st.gated:
        dpre = torch.empty_like(pre)
        _native.check(lib.drt_gated_gelu_new_bwd_bf16(dfd.data_ptr(), pre.data_ptr(), T, st.F, float(p), seed,
                                                      s_inner, dpre.data_ptr(), s), "drt_gated_gelu_new_bwd_bf16")
    else:
        dpre = torch.empty_like(fd)
        _native.check(lib.drt_relu_bwd_bf16(dfd.data_ptr(), fd.data_ptr(), fd.numel(), float(p), seed, s_inner,
                                            dpre.data_ptr(), s), "drt_relu_bwd_bf16")
    dx1, dwi, _ = linear_backward(dpre, x1, ly["wi_t"], want_db=False)
    dh2, dg1 = rmsnorm_backward(dx1, h2, ly["g1"], sh.eps, dres=d)
    # h2 = h + dropout(ctx Wo^T)
    dy1 = dropout(dh2, p, seed, s_out1) if p > 0 else dh2
    dctx, dwo, _ = linear_backward(dy1, ctx, ly["wo_t"], want_db=False)
    dqkv, dtable = attention_backward(qkv, ctx, dctx, lse, st.mask, bits, st.B, st.L, sh.heads, 1.0, relbias=table,
                                      drop=(p, seed, s_att))
    dx0, dwqkv, _ = linear_backward(dqkv, x0, ly["wqkv_t"], want_db=False)
    d_in, dg0 = rmsnorm_backward(dx0, h, ly["g0"], sh.eps, dres=dh2)
    a = f"encoder.block.{i}.layer.0."
    ff = f"encoder.block.{i}.layer.1."
    grads = {a + "layer_norm.weight": dg0, ff + "layer_norm.weight": dg1, a + "SelfAttention.o.weight": dwo,
             ff + "DenseReluDense.wo.weight": dwf}
    for j, n in enumerate("qkv"):
        grads[a + f"SelfAttention.{n}.weight"] = dwqkv[j * st.I:(j + 1) * st.I]
    for j, n in enumerate(ly["wi_names"]):
        grads[n] = dwi[j * st.F:(j + 1) * st.F]
    return d_in, dtable, grads


def final_forward(st: _Step, h):
    lib = _native.load()
    s = _native.stream_ptr(st.dev)
    p, seed = st.drop
    y = _rms(lib, h, st.W.final_g, st.sh.eps, s)
    return dropout(y, p, seed, SITE_FINAL) if p > 0 else y


def final_backward(st: _Step, h, d):
    p, seed = st.drop
    if p > 0:
        d = dropout(d, p, seed, SITE_FINAL)
    return rmsnorm_backward(d, h, st.W.final_g, st.sh.eps)


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, st, shared):
        ctx.st = st
        return embed_forward(st)

    @staticmethod
    def backward(ctx, d):
        return None, embed_backward(ctx.st, d.contiguous())


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, table, st, i, names, *params):
        out, saved = block_forward(st, i, h, table)
        ctx.st, ctx.i, ctx.saved_acts, ctx.names, ctx.table = st, i, saved, names, table.detach()
        return out

    @staticmethod
    def backward(ctx, d):
        d_in, dtable, grads = block_backward(ctx.st, ctx.i, ctx.saved_acts, ctx.table, d.contiguous())
        ctx.saved_acts = None
        return (d_in, dtable, None, None, None) + grads_out(ctx.names, grads)


class _FinalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, st, weight):
        ctx.st, ctx.h = st, h
        return final_forward(st, h)

    @staticmethod
    def backward(ctx, d):
        dh, dg = final_backward(ctx.st, ctx.h, d.contiguous())
        ctx.h = None
        return dh, None, dg


def _block_names(model) -> List[List[str]]:
    """Per block, the HF names of its linears and norms (block 0's relative_attention_bias is the
    bias table's input, not a block parameter)."""
    named = dict(model.named_parameters())
    out = []
    for i in range(model.config.num_layers):
        pre = f"encoder.block.{i}."
        out.append([n for n in named if n.startswith(pre) and n != REL_BIAS])
    return out


def train_hidden_t5(model, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                    seed: Optional[int] = None) -> torch.Tensor:
    """last_hidden_state fp32 [B, L, d_model] of ``model`` (T5EncoderModel) with the HIP tower backward
    attached.  Dropout follows ``model.training`` and ``config.dropout_rate`` (seed: torch CPU RNG)."""
    B, L = input_ids.shape
    why = t5_tower_supported(model, L)
    if why is not None:
        raise NotImplementedError(f"HIP T5 training tower: {why}")
    dev = next(model.parameters()).device
    ids = input_ids.to(dev, torch.int64).contiguous()
    mask = attention_mask.to(dev, torch.int64).contiguous() if attention_mask is not None else None
    cfg = model.config
    p = float(cfg.dropout_rate) if model.training else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
    st = _Step(model, _Weights(model, dev), ids, mask, (p, seed))
    named: Dict[str, torch.Tensor] = dict(model.named_parameters())
    table = relative_bias_table_grad(named[REL_BIAS], L, cfg.relative_attention_num_buckets,
                                     cfg.relative_attention_max_distance)
    h = _EmbedFn.apply(st, named["shared.weight"])
    for i, names in enumerate(_block_names(model)):
        h = _BlockFn.apply(h, table, st, i, names, *[named[n] for n in names])
    h = _FinalFn.apply(h, st, named["encoder.final_layer_norm.weight"])
    return h.view(B, L, cfg.d_model).float()

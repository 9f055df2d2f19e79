"""Training forward + backward of a BERT tower on the HIP kernels.

The reference differentiates HF ``BertModel`` under autograd in every training step
(DRT/trainer/trainer.py:113-133 -> DRModel.forward, DRT/model/biencoder.py:88-125).  Here one
``torch.autograd.Function`` per BertLayer (plus one for the embeddings) runs the tower, so each
layer's parameter gradients reach autograd -- and DDP's bucketed all-reduce -- as soon as that
layer's backward is done: the forward on the inference kernels plus the activations the backward needs (bf16: layer input, qkv, ctx, attention LSE, pre-LN sums,
post-LN1, FFN pre-/post-activation), and the backward entirely on HIP kernels:

    LN2 bwd -> FFN2 linear bwd -> GELU bwd -> FFN1 linear bwd (+ dx2 residual in the dgrad
    epilogue) -> LN1 bwd -> O-proj linear bwd -> attention bwd -> QKV linear bwd (+ dx1)
    ... -> embedding LN bwd -> word / position / type scatter-add

producing fp32 gradients for every HF parameter (QKV split back into query/key/value).
Dropout as HF applies it in train mode (embeddings output, attention probabilities, both
sublayer outputs before their residual add; hidden_dropout_prob / attention_probs_dropout_prob):
each keep is a counter-based hash of (per-call seed, site, element index) (csrc/drt_common.h
drop_hash24; the attention probabilities draw two keeps per 32-bit hash of (row key, key pair),
attn_row_key / attn_mix), so the backward regenerates the hidden-site masks instead of storing them
and reads the attention keep bits the forward wrote (1 bit per probability); the seed comes from torch's CPU generator (``torch.manual_seed`` makes a step reproducible).  The
masks are not HF's Philox stream: same distribution and semantics, different draws.
Scope: L <= 512 (BERT max_position_embeddings; L <= 160 -- the recipe, p_max_len 156 -- runs the whole-sequence
attention backward, longer sequences the streamed one), erf GELU, head_dim 64; anything else
raises.

Padding-free training (``train_hidden(..., plan=PackingPlan)``, opt-in through
``DRModel.hip_packed_train`` / ``RRModel.hip_packed_train``): the same nodes run on the packed rows of
the batch (model/packing.py) instead of the ``[B, L]`` rectangle -- the packed embedding, the varlen
attention pair (``drt_attention_varlen_train_forward_bf16`` / ``..._backward_bf16``) and, as a last node,
the unpack to ``[B, L, H]`` with zeros at the pads, whose backward is ``pack_rows``.  Every matrix has
``T32 = ceil(T / 32) * 32`` rows, so the weight gradients stay on the TN GEMM (which needs a multiple
of 32 rows).  INVARIANT: the ``T32 - T`` tail rows of every gradient that enters a wgrad or a column
sum are exactly zero, and the tail rows of every saved activation are finite.  It holds by
construction: the embedding output, ctx and dqkv are allocated with a zero tail (the attention kernels
never touch it), ``pack_rows`` zeroes the tail of the incoming gradient, and the LayerNorm, GELU,
dropout and dgrad of a zero gradient row are zero.  Hidden-site dropout uses the existing kernels and
GEMM epilogues unchanged, so element (t, j) of a packed matrix draws index ``t * H + j``: the same
distribution as the padded run, different draws; the attention keeps of every real (query, key) ARE
the padded run's (the hash takes the padded row).  A plan with ``max_len > 160`` (the streamed
backward has no varlen form) keeps the padded tower, logged once.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import _native
from .encoder import BertShape, _check_supported, bert_weights
from .encoder_bwd import (LIN_GELU, _ptr, attention_backward, attention_forward, attention_varlen_backward,
                          attention_varlen_forward, dropout, grads_out, layernorm_backward, linear, linear_backward,
                          pack_rows, transpose_bf16, unpack_rows)

MAX_TRAIN_SEQ = 512
# kAbMaxSeq of csrc/drt_common.h: the whole-sequence attention backward (the streamed one has no varlen
# form).  tests/test_packed_train_host_cpu.py pins it to what the two varlen training entries accept.
MAX_PACKED_TRAIN_LEN = 160

# Attention launches of the packed tower: False = one launch per batch (forward and backward), True =
# one per length class of the plan (PackingPlan.classes()).  A/B switch: one launch won in the attention
# backward alone (one layer at 512 x 128 with lengths 32-128: 182 us in one launch, 205 us in 4, 238 us
# padded; at 256 x 160: 178 / 186 / 215) and end to end (31.56 against 31.84 ms, 25.06 against 25.29 ms);
# DESIGN.md §5 "Padding-free training" (tools/packed_train_ab.py, profiles/packed_train01/).
packed_train_classes = False


def tower_supported(model) -> Optional[str]:
    """None if the HIP training tower can run this HF BertModel, else the reason."""
    cfg = model.config
    if type(model).__name__ != "BertModel":
        return f"{type(model).__name__} is not a BertModel"
    try:
        _check_supported(BertShape.from_config(cfg))
    except ValueError as e:
        return str(e)
    return None


class _Weights:
    """bf16 copies (and transposes) of the tower's linears for one step; fp32 LN / bias / tables."""

    def __init__(self, model, dev):
        sd = dict(model.named_parameters())
        self.names = list(sd.keys())
        self.sd = sd
        # the inference encoder's snapshot (model/encoder.py bert_weights) plus each linear's transpose
        # ([N, K] bf16 -> [K, N], the dgrad GEMM's operand)
        emb, self.layers = bert_weights(sd, dev, model.config.num_hidden_layers)
        self.word, self.pos, self.type, self.emb_g, self.emb_b = emb
        for ly in self.layers:
            for w in ("wqkv", "wo", "wi", "wf"):
                ly[w + "_t"] = transpose_bf16(ly[w])


def _layernorm(lib, x, g, b, eps, stream):
    out = torch.empty_like(x)
    _native.check(lib.drt_layernorm_bf16(x.data_ptr(), x.shape[0], x.shape[1], g.data_ptr(), b.data_ptr(), eps,
                                         out.data_ptr(), stream), "drt_layernorm_bf16")
    return out


def dropout_sites(layer: int):
    """(attention probabilities, attention output, FFN output) site ids of a layer; 0 = embeddings."""
    return 4 * layer + 1, 4 * layer + 2, 4 * layer + 3


class _Step:
    """What every node of one tower pass shares: weights, shape, masks' inputs, dropout."""

    def __init__(self, model, W: _Weights, ids, mask, drop, types=None, plan=None):
        cfg = model.config
        self.model, self.W, self.ids, self.mask, self.drop = model, W, ids, mask, drop
        self.types = types   # token_type_ids [B, L] int64 or None (all type 0)
        self.B, self.L = ids.shape
        self.plan = plan     # PackingPlan: the tower runs on ``rows`` packed rows, of which plan.T are tokens
        self.rows = (plan.T + 31) // 32 * 32 if plan is not None else self.B * self.L
        self.H, self.heads, self.eps = cfg.hidden_size, cfg.num_attention_heads, float(cfg.layer_norm_eps)
        self.scale = 1.0 / (self.H // self.heads) ** 0.5
        self.dev = ids.device


def embed_forward(st: _Step):
    """h0 = dropout(LN(word + pos + type)) bf16 [T, H] and the pre-LN sum the backward needs."""
    lib = _native.load()
    s = _native.stream_ptr(st.dev)
    W = st.W
    T = st.rows
    h = torch.empty((T, st.H), dtype=torch.bfloat16, device=st.dev)
    emb_pre = torch.empty_like(h)
    if st.plan is not None:
        pl = st.plan
        if T > pl.T:   # the tail rows: zeros
            h[pl.T:].zero_()
            emb_pre[pl.T:].zero_()
        _native.check(lib.drt_embed_ln_pre_packed(st.ids.data_ptr(), _ptr(st.types), pl.cu_seqlens.data_ptr(), st.B,
                                                  st.L, pl.T, W.word.data_ptr(), W.pos.data_ptr(), W.type.data_ptr(),
                                                  W.emb_g.data_ptr(), W.emb_b.data_ptr(), st.eps, st.H, h.data_ptr(),
                                                  emb_pre.data_ptr(), s), "drt_embed_ln_pre_packed")
    else:
        _native.check(lib.drt_embed_ln_pre(st.ids.data_ptr(), _ptr(st.types), st.B, st.L, W.word.data_ptr(),
                                           W.pos.data_ptr(),
                                           W.type.data_ptr(), W.emb_g.data_ptr(), W.emb_b.data_ptr(), st.eps, st.H,
                                           h.data_ptr(), emb_pre.data_ptr(), s), "drt_embed_ln_pre")
    ph, _, seed = st.drop
    if ph > 0:
        h = dropout(h, ph, seed, 0)
    return h, emb_pre


def embed_backward(st: _Step, emb_pre, d) -> Dict[str, torch.Tensor]:
    lib = _native.load()
    s = _native.stream_ptr(st.dev)
    W = st.W
    ph, _, seed = st.drop
    if ph > 0:
        d = dropout(d, ph, seed, 0)
    demb, dge, dbe = layernorm_backward(d, emb_pre, W.emb_g, st.eps)
    if st.plan is not None:
        # back to the zero-padded rectangle for the scatter-add: zero rows add exact zeros, once per step
        demb = unpack_rows(demb, st.plan)
    dword = torch.zeros_like(W.word)
    dpos = torch.zeros_like(W.pos)
    dtype = torch.zeros_like(W.type)
    pad = st.model.embeddings.word_embeddings.padding_idx
    _native.check(lib.drt_embedding_bwd(st.ids.data_ptr(), _ptr(st.types), int(W.type.shape[0]), demb.data_ptr(),
                                        st.B, st.L, st.H, -1 if pad is None else int(pad), dword.data_ptr(),
                                        dpos.data_ptr(), dtype.data_ptr(), s), "drt_embedding_bwd")
    e = "embeddings."
    return {e + "word_embeddings.weight": dword, e + "position_embeddings.weight": dpos,
            e + "token_type_embeddings.weight": dtype, e + "LayerNorm.weight": dge, e + "LayerNorm.bias": dbe}


def layer_forward(st: _Step, i: int, h):
    """One BertLayer (train-mode dropout as HF) -> (h_out, saved activations)."""
    lib = _native.load()
    dev = st.dev
    s = _native.stream_ptr(dev)
    ly = st.W.layers[i]
    B, L, H, heads = st.B, st.L, st.H, st.heads
    T = st.rows
    ph, pa, seed = st.drop
    s_att, s_out1, s_out2 = dropout_sites(i)
    qkv = linear(h, ly["wqkv"], torch.empty((T, 3 * H), dtype=torch.bfloat16, device=dev), bias=ly["bqkv"])
    if st.plan is not None:
        ctx, lse, bits = attention_varlen_forward(qkv, st.plan, heads, st.scale, drop=(pa, seed, s_att),
                                                  per_class=packed_train_classes)
    else:
        ctx, lse, bits = attention_forward(qkv, st.mask, B, L, heads, st.scale, drop=(pa, seed, s_att))
    # x1 = dropout(ctx Wo^T + bo) + h, dropout in the GEMM epilogue
    x1 = linear(ctx, ly["wo"], torch.empty_like(h), bias=ly["bo"], resid=h, drop=(ph, seed, s_out1) if ph > 0 else None)
    h1 = _layernorm(lib, x1, ly["g1"], ly["b1"], st.eps, s)
    # f = GELU(fpre), fpre = h1 Wi^T + bi: both from the one GEMM epilogue
    fpre = torch.empty((T, ly["wi"].shape[0]), dtype=torch.bfloat16, device=dev)
    f = linear(h1, ly["wi"], torch.empty_like(fpre), bias=ly["bi"], flags=LIN_GELU, pre_out=fpre)
    # x2 = dropout(f Wf^T + bf) + h1
    x2 = linear(f, ly["wf"], torch.empty_like(h), bias=ly["bf"], resid=h1, drop=(ph, seed, s_out2) if ph > 0 else None)
    h2 = _layernorm(lib, x2, ly["g2"], ly["b2"], st.eps, s)
    return h2, (h, qkv, ctx, lse, bits, x1, h1, fpre, f, x2)


def layer_backward(st: _Step, i: int, saved, d) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """d h_in and the fp32 gradients of layer i's parameters (HF names) for d h_out."""
    h, qkv, ctx, lse, bits, x1, h1, fpre, f, x2 = saved
    ly = st.W.layers[i]
    H, heads, eps = st.H, st.heads, st.eps
    ph, pa, seed = st.drop
    p = f"encoder.layer.{i}."
    s_att, s_out1, s_out2 = dropout_sites(i)
    # LN backward also emits the dropped gradient entering FFN2; FFN2's dgrad applies the GELU
    # backward in its epilogue (-> d fpre)
    # (the LayerNorm backwards also return the column sums of what they hand down: the dense
    # biases' gradients, without a pass over dy2 / dy1)
    if ph > 0:
        dx2, dg2, db2, dy2, sum2 = layernorm_backward(d, x2, ly["g2"], eps, drop=(ph, seed, s_out2), want_sum=True)
    else:
        dx2, dg2, db2, sum2 = layernorm_backward(d, x2, ly["g2"], eps, want_sum=True)
        dy2 = dx2
    dbi = torch.empty(fpre.shape[1], dtype=torch.float32, device=st.dev)   # from FFN2's dgrad epilogue
    dfpre, dwf, dbf = linear_backward(dy2, f, ly["wf_t"], gelu_pre=fpre, db=sum2, dx_colsum=dbi)
    dh1, dwi, dbi = linear_backward(dfpre, h1, ly["wi_t"], resid=dx2, db=dbi)
    if ph > 0:
        dx1, dg1, db1, dy1, sum1 = layernorm_backward(dh1, x1, ly["g1"], eps, drop=(ph, seed, s_out1), want_sum=True)
    else:
        dx1, dg1, db1, sum1 = layernorm_backward(dh1, x1, ly["g1"], eps, want_sum=True)
        dy1 = dx1
    dctx, dwo, dbo = linear_backward(dy1, ctx, ly["wo_t"], db=sum1)
    # the attention backward also leaves per-sequence column sums of dQKV: the q / k / v bias
    # gradients without a pass over dQKV
    if st.plan is not None:
        dqkv, dbqkv = attention_varlen_backward(qkv, ctx, dctx, lse, bits, st.plan, heads, st.scale,
                                                drop=(pa, seed, s_att), per_class=packed_train_classes)
    else:
        dqkv, dbqkv = attention_backward(qkv, ctx, dctx, lse, st.mask, bits, st.B, st.L, heads, st.scale,
                                         drop=(pa, seed, s_att), want_dbias=True)
    d_in, dwqkv, dbqkv = linear_backward(dqkv, h, ly["wqkv_t"], resid=dx1, db=dbqkv)
    grads = {}
    grads[p + "output.LayerNorm.weight"], grads[p + "output.LayerNorm.bias"] = dg2, db2
    grads[p + "output.dense.weight"], grads[p + "output.dense.bias"] = dwf, dbf
    grads[p + "intermediate.dense.weight"], grads[p + "intermediate.dense.bias"] = dwi, dbi
    grads[p + "attention.output.LayerNorm.weight"], grads[p + "attention.output.LayerNorm.bias"] = dg1, db1
    grads[p + "attention.output.dense.weight"], grads[p + "attention.output.dense.bias"] = dwo, dbo
    for j, n in enumerate(("query", "key", "value")):
        grads[p + f"attention.self.{n}.weight"] = dwqkv[j * H:(j + 1) * H]
        grads[p + f"attention.self.{n}.bias"] = dbqkv[j * H:(j + 1) * H]
    return d_in, grads


# One autograd node per BertLayer (and one for the embeddings): each node's parameter gradients
# are handed to autograd (AccumulateGrad, so DDP's bucket hooks) as soon as THAT layer's backward
# is done, and DDP's gradient all-reduce of layer i overlaps the backward of layers i-1 .. 0
# (trainer.py:47-63 wraps the model in DDP).  The activation between nodes is the bf16 hidden
# state; all nodes of one pass share a _Step (weights snapshot, ids, mask, dropout seed).


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, st, names, *params):
        h, emb_pre = embed_forward(st)
        ctx.st, ctx.emb_pre, ctx.names = st, emb_pre, names
        return h

    @staticmethod
    def backward(ctx, d):
        grads = embed_backward(ctx.st, ctx.emb_pre, d.contiguous())
        ctx.emb_pre = None
        return (None, None, None) + grads_out(ctx.names, grads)


class _LayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, st, i, names, *params):
        h2, saved = layer_forward(st, i, h)
        ctx.st, ctx.i, ctx.saved_acts, ctx.names = st, i, saved, names
        return h2

    @staticmethod
    def backward(ctx, d):
        d_in, grads = layer_backward(ctx.st, ctx.i, ctx.saved_acts, d.contiguous())
        ctx.saved_acts = None
        return (d_in, None, None, None) + grads_out(ctx.names, grads)


class _UnpackFn(torch.autograd.Function):
    """Last node of the packed tower: [T32, H] packed rows -> [B * L, H] with zeros at the pads; the
    backward packs the gradient's real rows and zeroes the tail."""

    @staticmethod
    def forward(ctx, h, st):
        ctx.st = st
        return unpack_rows(h, st.plan)

    @staticmethod
    def backward(ctx, d):
        return pack_rows(d.contiguous(), ctx.st.plan, ctx.st.rows), None


def _log_fallback(why: str):
    from .biencoder import _log_fallback as log
    log(why)


def _param_groups(model):
    """(embedding names/params, [per-layer names/params]) in the HF naming."""
    named = dict(model.named_parameters())
    emb = [n for n in named if n.startswith("embeddings.")]
    layers = []
    for i in range(model.config.num_hidden_layers):
        pre = f"encoder.layer.{i}."
        layers.append([n for n in named if n.startswith(pre)])
    return named, emb, layers


def train_hidden(model, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                 seed: Optional[int] = None, token_type_ids: Optional[torch.Tensor] = None, plan=None) -> torch.Tensor:
    """last_hidden_state fp32 [B, L, H] of ``model`` with the HIP tower backward attached (one autograd
    node per layer).  Dropout follows ``model.training`` and the config's probabilities (seed: torch
    CPU RNG).  ``plan`` (model/packing.py PackingPlan of this batch's mask): the tower runs on the
    packed rows and the pad positions of the result are zeros; a plan the packed tower cannot take
    (its longest sequence over 160 tokens, or a plan of another batch shape) keeps the padded tower,
    logged once."""
    why = tower_supported(model)
    if why is not None:
        raise NotImplementedError(f"HIP training tower: {why}")
    if plan is not None:
        if plan.max_len > MAX_PACKED_TRAIN_LEN:
            _log_fallback(f"hip_packed_train: padded tower, longest sequence {plan.max_len} > {MAX_PACKED_TRAIN_LEN}")
            plan = None
        elif (plan.B, plan.L) != tuple(input_ids.shape):
            _log_fallback("hip_packed_train: padded tower, the plan is of another batch shape")
            plan = None
    dev = next(model.parameters()).device
    ids = input_ids.to(dev, torch.int64).contiguous()
    mask = attention_mask.to(dev, torch.int64).contiguous() if attention_mask is not None else None
    types = token_type_ids.to(dev, torch.int64).contiguous() if token_type_ids is not None else None
    if types is not None and (types.shape != ids.shape or model.config.type_vocab_size > 4):
        raise ValueError("HIP training tower: token_type_ids must match input_ids, type_vocab_size <= 4")
    B, L = ids.shape
    cfg = model.config
    lmax = min(MAX_TRAIN_SEQ, int(cfg.max_position_embeddings))
    if L > lmax:
        raise ValueError(f"HIP training tower: sequence length {L} > {lmax}")
    ph = float(cfg.hidden_dropout_prob) if model.training else 0.0
    pa = float(cfg.attention_probs_dropout_prob) if model.training else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (ph > 0 or pa > 0) else 0
    if plan is not None and plan.cu_seqlens.device != dev:
        plan.cu_seqlens = plan.cu_seqlens.to(dev)
    st = _Step(model, _Weights(model, dev), ids, mask, (ph, pa, seed), types, plan)
    named, emb, layers = _param_groups(model)
    h = _EmbedFn.apply(ids, st, emb, *[named[n] for n in emb])
    for i, names in enumerate(layers):
        h = _LayerFn.apply(h, st, i, names, *[named[n] for n in names])
    if plan is not None:
        h = _UnpackFn.apply(h, st)
    return h.view(B, L, cfg.hidden_size).float()

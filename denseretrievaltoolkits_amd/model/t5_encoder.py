"""T5 encoder forward on the HIP kernels (bf16 storage, fp32 accumulation).

Replaces the HF ``T5EncoderModel.forward`` that ``DRModel.encode`` calls for ``encoder_only``
towers (transformers modeling_t5.py, eval mode) for inference:

    h    = shared.weight[ids]                       (bf16 residual stream; no position table)
    per block:
      x    = rmsnorm(h, ln0)                        (fp32 sum of squares, no mean, no bias)
      qkv  = linear(x, [Wq|Wk|Wv])                  (no bias; inner = heads * 64 may differ from d_model)
      ctx  = attention(qkv, key mask, bias table)   (q k^T + bias[head][bucket(k - q)], NOT scaled)
      h    = linear(ctx, Wo) + h                    (fp32 sum, stored bf16)
      x    = rmsnorm(h, ln1)
      relu:        f = relu(linear(x, Wi))          (epilogue flag)
      gated-gelu:  f = gelu_new(x Wi0^T) * (x Wi1^T)  (one GEMM over [Wi0; Wi1], then the gate)
      h    = linear(f, Wo_ff) + h
    h = rmsnorm(h, final_layer_norm)

The relative-position bias of block 0 serves every block; it reaches the attention kernel as a
table over k - q (``relative_bias_table``), built once per sequence length.  Weights are
snapshotted from the HF module (bf16 linears, fp32 embedding / norm weights / bias table).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .. import _native
from .encoder import HipBertEncoder, linear_ws, run_on_two_streams

MAX_SEQ = 512
LIN_RELU = 8     # drt_linear_bf16* flag bit 3


@dataclass
class T5Shape:
    d_model: int
    layers: int
    heads: int
    d_kv: int
    d_ff: int
    eps: float
    act: str            # feed_forward_proj: "relu" or "gated-gelu"
    buckets: int
    max_distance: int

    @classmethod
    def from_config(cls, cfg) -> "T5Shape":
        return cls(cfg.d_model, cfg.num_layers, cfg.num_heads, cfg.d_kv, cfg.d_ff, float(cfg.layer_norm_epsilon),
                   str(cfg.feed_forward_proj), cfg.relative_attention_num_buckets,
                   cfg.relative_attention_max_distance)

    def unsupported(self) -> Optional[str]:
        if self.d_kv != 64:
            return f"d_kv {self.d_kv} unsupported (the attention kernel's head_dim is 64)"
        if self.d_model % 256 or self.d_model > 1024:
            return f"d_model {self.d_model} unsupported (multiple of 256, <= 1024)"
        if self.d_ff % 64:
            return f"d_ff {self.d_ff} unsupported (multiple of 64)"
        if self.act not in ("relu", "gated-gelu"):
            return f"feed_forward_proj {self.act!r} unsupported (relu or gated-gelu)"
        return None


def t5_supported(model) -> Optional[str]:
    """None when HipT5Encoder can run this module, else the reason it cannot."""
    if type(model).__name__ != "T5EncoderModel":
        return f"{type(model).__name__} is not a T5EncoderModel"
    return T5Shape.from_config(model.config).unsupported()


def _relative_buckets(rel: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """HF T5Attention._relative_position_bucket, bidirectional, of rel = key - query (int64): half the
    buckets per sign, exact up to num_buckets / 4, log-spaced up to max_distance, then clamped."""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    rel = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact)
                         * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(rel < max_exact, rel, large)


def relative_bias_table(weight: torch.Tensor, L: int, num_buckets: int, max_distance: int) -> torch.Tensor:
    """fp32 [heads, 2L-1] on the weight's device: entry (h, k - q + L - 1) is HF's
    T5Attention.compute_bias(L, L)[0, h, q, k], from relative_attention_bias.weight [num_buckets, heads].
    The 2L-1 bucket numbers are computed on the CPU, as HF's fp32 reference run computes them."""
    bucket = _relative_buckets(torch.arange(-(L - 1), L, dtype=torch.long), num_buckets, max_distance)
    return weight.detach().float()[bucket.to(weight.device)].t().contiguous()


class HipT5Encoder:
    """Inference forward of a T5EncoderModel tower on gfx950 kernels."""

    def __init__(self, shape: T5Shape, state: Dict[str, torch.Tensor], device: torch.device):
        why = shape.unsupported()
        if why is not None:
            raise ValueError(why)
        self.split_streams = True       # two halves on two streams, as HipBertEncoder
        self.split_min_tokens = 8192
        self._streams = None
        self._ws_plan = {}
        self._ws = None
        self._bias_tables = {}
        self.shape = shape
        self.device = device
        self.lib = _native.load()
        self._load(state)

    # -- weights --------------------------------------------------------
    def _load(self, sd: Dict[str, torch.Tensor]):
        dev = self.device

        def f32(name):
            return sd[name].detach().to(dev, torch.float32).contiguous()

        def b16(*names):
            w = torch.cat([sd[n].detach().float() for n in names], 0)
            return w.to(dev).to(torch.bfloat16).contiguous()

        self.word = f32("shared.weight")
        self.rel_weight = f32("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")
        self.final_g = f32("encoder.final_layer_norm.weight")
        gated = self.shape.act == "gated-gelu"
        self.layers = []
        for i in range(self.shape.layers):
            a = f"encoder.block.{i}.layer.0."
            f = f"encoder.block.{i}.layer.1."
            wi = [f + "DenseReluDense.wi_0.weight", f + "DenseReluDense.wi_1.weight"] if gated \
                else [f + "DenseReluDense.wi.weight"]
            self.layers.append(dict(
                g0=f32(a + "layer_norm.weight"),
                wqkv=b16(*(a + f"SelfAttention.{n}.weight" for n in "qkv")),
                wo=b16(a + "SelfAttention.o.weight"),
                g1=f32(f + "layer_norm.weight"),
                wi=b16(*wi),
                wf=b16(f + "DenseReluDense.wo.weight"),
            ))

    @classmethod
    def from_hf(cls, model, device) -> "HipT5Encoder":
        why = t5_supported(model)
        if why is not None:
            raise ValueError(why)
        return cls(T5Shape.from_config(model.config), dict(model.state_dict()), torch.device(device))

    def _bias_table(self, L: int) -> torch.Tensor:
        t = self._bias_tables.get(L)
        if t is None:
            t = self._bias_tables[L] = relative_bias_table(self.rel_weight, L, self.shape.buckets,
                                                           self.shape.max_distance)
        return t

    # -- forward --------------------------------------------------------
    def _lin(self, x, w, out, resid=None, flags=0):
        return linear_ws(self.lib, x, w, None, resid, out, flags, self._ws, self.stream)

    def _rms(self, x, g, out):
        _native.check(self.lib.drt_rmsnorm_bf16(x.data_ptr(), x.shape[0], x.shape[1], g.data_ptr(), self.shape.eps,
                                                out.data_ptr(), self.stream), "drt_rmsnorm_bf16")
        return out

    def _ws_bytes(self, T: int) -> int:
        """Split-K scratch for this token count (small batches only; 0 at encode sizes)."""
        nb = self._ws_plan.get(T)
        if nb is None:
            sh = self.shape
            D, I, F = sh.d_model, sh.heads * sh.d_kv, sh.d_ff
            F1 = 2 * F if sh.act == "gated-gelu" else F
            nb = max(int(self.lib.drt_linear_workspace(T, n, k)) for n, k in ((3 * I, D), (D, I), (F1, D), (D, F)))
            self._ws_plan[T] = nb
        return nb

    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                token_type_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """last_hidden_state [B, L, d_model] bf16."""
        if token_type_ids is not None:
            raise ValueError("T5 has no token types: token_type_ids must be None")
        dev = self.device
        ids = input_ids.to(dev, torch.int64).contiguous()
        B, L = ids.shape
        if L > MAX_SEQ:
            raise ValueError(f"sequence length {L} exceeds the attention kernel's {MAX_SEQ}")
        mask = attention_mask.to(dev, torch.int64).contiguous() if attention_mask is not None else None
        if (self.split_streams and B >= 2 and B * L >= self.split_min_tokens
                and not torch.cuda.is_current_stream_capturing()):
            # two halves on two streams, as HipBertEncoder (same kernels per half -> same bits)
            def part(a, b):
                return lambda out: self._run(ids[a:b], mask[a:b] if mask is not None else None, out=out)

            half = B // 2
            out = torch.empty((B * L, self.shape.d_model), dtype=torch.bfloat16, device=dev)
            self._bias_table(L)             # built on the launch stream, before the halves fork
            return run_on_two_streams(self, out, [(part(0, half), slice(0, half * L)),
                                                  (part(half, B), slice(half * L, B * L))]).view(B, L, -1)
        return self._run(ids, mask)

    def _run(self, ids, mask, out=None):
        sh = self.shape
        dev = self.device
        lib = self.lib
        B, L = ids.shape
        D, I, F, T = sh.d_model, sh.heads * sh.d_kv, sh.d_ff, B * L
        gated = sh.act == "gated-gelu"
        self.stream = _native.stream_ptr(dev)
        table = self._bias_table(L)

        def buf(n):
            return torch.empty((T, n), dtype=torch.bfloat16, device=dev)

        h, h2, x = buf(D), buf(D), buf(D)
        qkv, ctx, ffn = buf(3 * I), buf(I), buf(F)
        ffn2 = buf(2 * F) if gated else None
        nb = self._ws_bytes(T)
        self._ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev) if nb else None
        _native.check(lib.drt_t5_embed_bf16(ids.data_ptr(), B, L, self.word.data_ptr(), D, h.data_ptr(), self.stream),
                      "drt_t5_embed_bf16")
        mp = mask.data_ptr() if mask is not None else None
        for ly in self.layers:
            self._rms(h, ly["g0"], x)
            self._lin(x, ly["wqkv"], qkv)
            _native.check(lib.drt_attention_forward_bf16(qkv.data_ptr(), mp, table.data_ptr(), ctx.data_ptr(), None, None,
                                                         B, L, sh.heads, sh.d_kv, 1.0, 0.0, 0, 0, self.stream),
                          "drt_attention_forward_bf16")
            self._lin(ctx, ly["wo"], h2, resid=h)
            self._rms(h2, ly["g1"], x)
            if gated:
                self._lin(x, ly["wi"], ffn2)
                _native.check(lib.drt_gated_gelu_new_bf16(ffn2.data_ptr(), T, F, ffn.data_ptr(), self.stream),
                              "drt_gated_gelu_new_bf16")
            else:
                self._lin(x, ly["wi"], ffn, flags=LIN_RELU)
            self._lin(ffn, ly["wf"], h, resid=h2)
        res = out if out is not None else x
        return self._rms(h, self.final_g, res).view(B, L, D)

    __call__ = forward

    pool = HipBertEncoder.pool          # drt_pool_bf16 with the reference's pooling semantics

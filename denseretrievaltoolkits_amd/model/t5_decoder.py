"""One decoder step of a T5ForConditionalGeneration on the HIP kernels: monoT5 pair scoring.

Replaces what ``RRModel.encode`` asks of the HF module for T5 rerankers (reference
DRT/model/reranker.py:115-119): ``decoder_input_ids = 0`` and ``logits[:, 0, [neg, pos]]``.  The
encoder is ``HipT5Encoder``; its output E [B, L, D] (after the final RMSNorm) feeds one decoder token
per sequence, for which the step collapses (transformers modeling_t5.py, eval mode):

    h = shared.weight[0]                            (bf16 residual stream [B, D])
    per decoder block:
      x  = rmsnorm(h, ln0);  h += x (Wo_self Wv_self)^T       (one key: the softmax is 1, so q, k and the
                                                               decoder's position bias never matter; the
                                                               [D, D] product is formed once at snapshot
                                                               time in fp32 and rounded once)
      x  = rmsnorm(h, ln1);  q = x Wq^T                       [B, I], I = heads * 64
      qt[b, h, :]  = sum_j q[b, 64h+j] Wk[64h+j, :]           (drt_t5_head_expand_bf16)
      pooled[b, h] = softmax_l(qt[b, h] . E[b, l] + key mask) E[b]     (drt_t5_cross_pool_bf16: E read
                                                               once, no K / V projection of it)
      c[b, 64h+j]  = Wv[64h+j, :] . pooled[b, h, :]           (drt_t5_head_reduce_bf16)
      h += c Wo^T
      x  = rmsnorm(h, ln2);  h += FFN(x)                      (the encoder's FFN: relu or gated-gelu)
    y = rmsnorm(h, decoder.final_layer_norm)
    logit_t = c_out * y . lm_head.weight[t],  c_out = d_model^-0.5 where the HF module scales its
    decoder output (config.scale_decoder_outputs, or tie_word_embeddings on older transformers).

T5 scales no score and the cross-attention has a zero position bias.  Weights are snapshotted as
the encoder loader does (bf16 linears, fp32 norm weights); c_out is folded into the requested
lm_head rows in fp32 before they are rounded to bf16.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .. import _native
from .encoder import linear_ws
from .t5_encoder import LIN_RELU, HipT5Encoder, T5Shape

MAX_HEADS = 16
LIN_F32 = 2      # drt_linear_bf16* flag bit 1: fp32 output


def t5_seq2seq_supported(model) -> Optional[str]:
    """None when HipT5PairScorer can run this module, else the reason it cannot."""
    if type(model).__name__ != "T5ForConditionalGeneration":
        return f"{type(model).__name__} is not a T5ForConditionalGeneration"
    shape = T5Shape.from_config(model.config)
    why = shape.unsupported()
    if why is not None:
        return why
    if shape.heads > MAX_HEADS:
        return f"num_heads {shape.heads} unsupported (the cross-attention kernel holds at most {MAX_HEADS} heads)"
    return None


def _output_scale(cfg) -> float:
    scaled = cfg.scale_decoder_outputs if hasattr(cfg, "scale_decoder_outputs") else cfg.tie_word_embeddings
    return float(cfg.d_model) ** -0.5 if scaled else 1.0


class HipT5PairScorer:
    """Inference forward of a T5ForConditionalGeneration over one decoder token on gfx950 kernels."""

    def __init__(self, shape: T5Shape, dec_layers: int, out_scale: float, state: Dict[str, torch.Tensor],
                 device: torch.device):
        if shape.heads > MAX_HEADS:
            raise ValueError(f"num_heads {shape.heads} unsupported (at most {MAX_HEADS})")
        self.encoder = HipT5Encoder(shape, state, device)
        self.shape = shape
        self.dec_layers = dec_layers
        self.out_scale = out_scale
        self.device = device
        self.lib = self.encoder.lib
        self._token_rows = {}
        self._ws_plan = {}
        self._ws = None
        self._load(state)

    # -- weights --------------------------------------------------------
    def _load(self, sd: Dict[str, torch.Tensor]):
        dev = self.device

        def f32(name):
            return sd[name].detach().to(dev, torch.float32).contiguous()

        def b16(*names):
            w = torch.cat([sd[n].detach().float() for n in names], 0)
            return w.to(dev).to(torch.bfloat16).contiguous()

        def self_product(prefix):
            # Wo_self Wv_self [D, D]: the fp32 product of the fp32 weights, rounded once
            wo = sd[prefix + "SelfAttention.o.weight"].detach().to(dev, torch.float32)
            wv = sd[prefix + "SelfAttention.v.weight"].detach().to(dev, torch.float32)
            return (wo @ wv).to(torch.bfloat16).contiguous()

        self.start = f32("shared.weight")[:1].contiguous()       # the row of decoder_start_token_id = 0
        self.final_g = f32("decoder.final_layer_norm.weight")
        self.lm_head = sd["lm_head.weight"].detach() if "lm_head.weight" in sd else sd["shared.weight"].detach()
        gated = self.shape.act == "gated-gelu"
        self.layers = []
        for i in range(self.dec_layers):
            s = f"decoder.block.{i}.layer.0."
            c = f"decoder.block.{i}.layer.1."
            f = f"decoder.block.{i}.layer.2."
            wi = [f + "DenseReluDense.wi_0.weight", f + "DenseReluDense.wi_1.weight"] if gated \
                else [f + "DenseReluDense.wi.weight"]
            self.layers.append(dict(
                g0=f32(s + "layer_norm.weight"),
                w_self=self_product(s),
                g1=f32(c + "layer_norm.weight"),
                wq=b16(c + "EncDecAttention.q.weight"),
                wk=b16(c + "EncDecAttention.k.weight"),
                wv=b16(c + "EncDecAttention.v.weight"),
                wo=b16(c + "EncDecAttention.o.weight"),
                g2=f32(f + "layer_norm.weight"),
                wi=b16(*wi),
                wf=b16(f + "DenseReluDense.wo.weight"),
            ))

    @classmethod
    def from_hf(cls, model, device) -> "HipT5PairScorer":
        why = t5_seq2seq_supported(model)
        if why is not None:
            raise ValueError(why)
        cfg = model.config
        return cls(T5Shape.from_config(cfg), int(cfg.num_decoder_layers), _output_scale(cfg), dict(model.state_dict()),
                   torch.device(device))

    def _rows(self, token_ids: Sequence[int]) -> torch.Tensor:
        """bf16 [len(token_ids), D]: c_out * lm_head.weight[token_ids], scaled in fp32, rounded once."""
        key = tuple(int(t) for t in token_ids)
        rows = self._token_rows.get(key)
        if rows is None:
            w = self.lm_head[list(key)].to(self.device, torch.float32) * self.out_scale
            rows = self._token_rows[key] = w.to(torch.bfloat16).contiguous()
        return rows

    # -- forward --------------------------------------------------------
    def _lin(self, x, w, out, resid=None, flags=0):
        return linear_ws(self.lib, x, w, None, resid, out, flags, self._ws, self.stream)

    def _rms(self, x, g, out):
        _native.check(self.lib.drt_rmsnorm_bf16(x.data_ptr(), x.shape[0], x.shape[1], g.data_ptr(), self.shape.eps,
                                                out.data_ptr(), self.stream), "drt_rmsnorm_bf16")
        return out

    def _ws_bytes(self, B: int, n_tokens: int) -> int:
        key = (B, n_tokens)
        nb = self._ws_plan.get(key)
        if nb is None:
            sh = self.shape
            D, I, F = sh.d_model, sh.heads * sh.d_kv, sh.d_ff
            F1 = 2 * F if sh.act == "gated-gelu" else F
            shapes = [(D, D), (I, D), (D, I), (F1, D), (D, F)] + ([(n_tokens, D)] if n_tokens else [])
            nb = max(int(self.lib.drt_linear_workspace(B, n, k)) for n, k in shapes)
            self._ws_plan[key] = nb
        return nb

    def _decode(self, enc: torch.Tensor, mask: Optional[torch.Tensor], n_tokens: int = 0) -> torch.Tensor:
        """The final normalised decoder state [B, D] bf16 for enc [B, L, D] bf16."""
        sh = self.shape
        dev = self.device
        lib = self.lib
        B, L, D = enc.shape
        I, F, H = sh.heads * sh.d_kv, sh.d_ff, sh.heads
        gated = sh.act == "gated-gelu"
        self.stream = _native.stream_ptr(dev)

        def buf(*shape):
            return torch.empty(shape, dtype=torch.bfloat16, device=dev)

        h, h2, x = buf(B, D), buf(B, D), buf(B, D)
        q, ctx = buf(B, I), buf(B, I)
        qt, pooled = buf(B, H * D), buf(B, H * D)
        ffn = buf(B, F)
        ffn2 = buf(B, 2 * F) if gated else None
        nb = self._ws_bytes(B, n_tokens)
        self._ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev) if nb else None
        ids = torch.zeros((B, 1), dtype=torch.int64, device=dev)
        _native.check(lib.drt_t5_embed_bf16(ids.data_ptr(), B, 1, self.start.data_ptr(), D, h.data_ptr(), self.stream),
                      "drt_t5_embed_bf16")
        mp = mask.data_ptr() if mask is not None else None
        for ly in self.layers:
            self._rms(h, ly["g0"], x)
            self._lin(x, ly["w_self"], h2, resid=h)
            self._rms(h2, ly["g1"], x)
            self._lin(x, ly["wq"], q)
            _native.check(lib.drt_t5_head_expand_bf16(q.data_ptr(), ly["wk"].data_ptr(), qt.data_ptr(), B, H, D,
                                                      self.stream), "drt_t5_head_expand_bf16")
            _native.check(lib.drt_t5_cross_pool_bf16(qt.data_ptr(), enc.data_ptr(), mp, pooled.data_ptr(), B, L, H, D,
                                                     self.stream), "drt_t5_cross_pool_bf16")
            _native.check(lib.drt_t5_head_reduce_bf16(pooled.data_ptr(), ly["wv"].data_ptr(), ctx.data_ptr(), B, H, D,
                                                      self.stream), "drt_t5_head_reduce_bf16")
            self._lin(ctx, ly["wo"], h, resid=h2)
            self._rms(h, ly["g2"], x)
            if gated:
                self._lin(x, ly["wi"], ffn2)
                _native.check(lib.drt_gated_gelu_new_bf16(ffn2.data_ptr(), B, F, ffn.data_ptr(), self.stream),
                              "drt_gated_gelu_new_bf16")
            else:
                self._lin(x, ly["wi"], ffn, flags=LIN_RELU)
            self._lin(ffn, ly["wf"], h2, resid=h)
            h, h2 = h2, h
        return self._rms(h, self.final_g, x)

    def _encode(self, input_ids, attention_mask):
        dev = self.device
        mask = attention_mask.to(dev, torch.int64).contiguous() if attention_mask is not None else None
        enc = self.encoder(input_ids, mask).contiguous()
        return enc, mask

    def decode_hidden(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HF decoder_hidden_states[-1][:, 0] (after the decoder's final norm): [B, D] bf16."""
        enc, mask = self._encode(input_ids, attention_mask)
        return self._decode(enc, mask)

    def logits(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
               token_ids: Sequence[int]) -> torch.Tensor:
        """HF logits[:, 0, token_ids] for decoder_input_ids = 0: [B, len(token_ids)] fp32."""
        rows = self._rows(token_ids)
        enc, mask = self._encode(input_ids, attention_mask)
        y = self._decode(enc, mask, n_tokens=rows.shape[0])
        out = torch.empty((y.shape[0], rows.shape[0]), dtype=torch.float32, device=self.device)
        return self._lin(y, rows, out, flags=LIN_F32)

"""Drop-in for DRT/model/reranker.py (RRModel, RROutput): cross-encoder reranking.

``RRModel.encode`` (reranker.py:111-130): pair forward ([CLS] q [SEP] d [SEP],
L = q_max_len + p_max_len = 160) -> pooling -> LinearHead(768 -> 1) score.  When
no gradient can be asked for (grad mode off or a frozen tower) the whole pair
tower runs on the HIP inference kernels (the same bf16 MFMA GEMMs + fused
attention as the bi-encoder) and the 768 -> 1 head on the HIP GEMM; with grad on
(training, or eval mode with grad) BERT pair towers up to L = 512 run on the HIP
training tower (model/train_tower.py, forward + backward on HIP kernels, HF
train-mode dropout), other towers on the HF module under autograd.  ``hip_packed = True``
(attribute, or ``model_args.hip_packed``) makes the no-grad BERT pair tower padding-free: only
the pairs' real tokens are computed (model/packing.py); same scores up to bf16 rounding.

T5 rerankers (monoT5, :115-119: ``T5ForConditionalGeneration`` with ``decoder_input_ids = 0``,
scores = ``logits[:, 0, [neg_token_id, pos_token_id]]``) follow the same rule: with no gradient to
ask for, the encoder runs on ``HipT5Encoder`` and the single decoder step on the absorbed
cross-attention kernels (model/t5_decoder.py, ``HipT5PairScorer``), returning [B, 2] fp32 in the
reference's column order; with grad on, or on the CPU, the HF module computes exactly what the
reference computes.  A configuration the kernels do not cover raises ``NotImplementedError`` on the
no-grad GPU path.
"""
from __future__ import annotations

import json
import logging
import os
from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn as nn
from torch import Tensor
from transformers import AutoConfig, AutoModel, BatchEncoding, PreTrainedModel
from transformers.modeling_outputs import ModelOutput

from ..trainer.losses import CrossEntropyLoss, rr_loss_functions
from .encoder import HipBertEncoder, linear_head
from .linear import LinearHead
from .t5_decoder import HipT5PairScorer, t5_seq2seq_supported
from .train_tower import MAX_TRAIN_SEQ, tower_supported, train_hidden

logger = logging.getLogger(__name__)


@dataclass
class RROutput(ModelOutput):
    pos_pair_scores: Tensor = None
    neg_pair_scores: Tensor = None
    loss: Tensor = None


def relevance(scores: Tensor) -> Tensor:
    """One relevance column from RRModel.encode's scores: a T5 reranker's [B, 2] (neg, pos) logits
    become monoT5's log_softmax(scores, -1)[:, 1] as [B, 1]; one-column scores pass through."""
    if scores.dim() == 2 and scores.shape[1] == 2:
        return torch.log_softmax(scores.float(), -1)[:, 1:2]
    return scores


class RRModel(nn.Module):
    def __init__(self, lm: PreTrainedModel, head: nn.Module, feature: str = "last_hidden_state",
                 pooling: str = "first", pos_token: str = None, neg_token: str = None, tokenizer=None,
                 model_args=None, data_args=None, train_args=None):
        super().__init__()
        self.lm = lm
        self.head = head
        self.feature = feature
        self.pooling = pooling
        self.pos_token = pos_token
        self.neg_token = neg_token
        self.tokenizer = tokenizer
        self.pos_token_id = tokenizer.encode(pos_token, add_special_tokens=False)[0] if pos_token else None
        self.neg_token_id = tokenizer.encode(neg_token, add_special_tokens=False)[0] if neg_token else None
        self.model_args = model_args
        self.data_args = data_args
        self.train_args = train_args
        self._hip = None
        # opt-in: padding-free inference of a BERT pair tower (model/packing.py); T5 rerankers stay padded
        self.hip_packed = bool(getattr(model_args, "hip_packed", False))
        # opt-in: padding-free training of a BERT pair tower (model/train_tower.py); separate from hip_packed
        self.hip_packed_train = bool(getattr(model_args, "hip_packed_train", False))
        if train_args is not None:
            self.loss_fn_str = train_args.loss_fn
            self.margin = train_args.margin
            self.loss_fn = rr_loss_functions[self.loss_fn_str](self.margin)
        if "T5" in type(self.lm).__name__ and not getattr(model_args, "encoder_only", False):
            self.loss_fn_str = "ce"
            self.loss_fn = CrossEntropyLoss()

    def _get_config_dict(self):
        return {"plm_backbone": {"type": type(self.lm).__name__, "feature": self.feature},
                "pooling": self.pooling, "pos_token": self.pos_token, "neg_token": self.neg_token}

    def forward(self, pos_pairs: Dict[str, Tensor] = None, neg_pairs: Dict[str, Tensor] = None):
        pos = self.encode(pos_pairs)
        if neg_pairs is None:
            return pos
        neg = self.encode(neg_pairs)
        if pos.shape != neg.shape:
            return RROutput(pos_pair_scores=pos, neg_pair_scores=neg)
        return RROutput(loss=self.loss_fn(pos, neg), pos_pair_scores=pos, neg_pair_scores=neg)

    def _hip_state(self):
        dev = next(self.lm.parameters()).device
        ver = tuple(p._version for p in self.lm.parameters()) + (self.head.linear.weight._version, str(dev))
        if self._hip is None or self._hip[0] != ver:
            if type(self.lm).__name__ != "BertModel":
                raise NotImplementedError(f"HIP reranker supports BERT-family towers only (got {type(self.lm).__name__})")
            enc = HipBertEncoder.from_hf(self.lm, dev)
            w = self.head.linear.weight.detach().to(torch.bfloat16).contiguous()
            self._hip = (ver, enc, w)
        return self._hip[1], self._hip[2]

    def _hip_t5_state(self):
        dev = next(self.lm.parameters()).device
        ver = tuple(p._version for p in self.lm.parameters()) + ("t5", str(dev))
        if self._hip is None or self._hip[0] != ver:
            why = t5_seq2seq_supported(self.lm)
            if why is not None:
                raise NotImplementedError(f"HIP T5 reranker: {why}")
            self._hip = (ver, HipT5PairScorer.from_hf(self.lm, dev))
        return self._hip[1]

    def _encode_t5(self, items):
        """reranker.py:115-119: one decoder step from token 0, logits of (neg_token, pos_token)."""
        dev = next(self.lm.parameters()).device
        tokens = (self.neg_token_id, self.pos_token_id)
        frozen = not any(p.requires_grad for p in self.lm.parameters())
        if dev.type == "cuda" and (not torch.is_grad_enabled() or frozen):
            return self._hip_t5_state().logits(items["input_ids"], items.get("attention_mask"), tokens)
        from .biencoder import _log_fallback
        _log_fallback("T5 reranker: " + ("tower on the CPU" if dev.type != "cuda" else
                                         "autograd on (the decoder step has no HIP backward)"))
        ids = items["input_ids"]
        start = ids.new_zeros((ids.shape[0], 1), dtype=torch.long)
        logits = self.lm(**items, decoder_input_ids=start, return_dict=True).logits
        return logits[:, 0, list(tokens)]

    def encode(self, items):
        if items is None:
            return None, None
        items = BatchEncoding(items)
        if "T5" in type(self.lm).__name__ and not getattr(self.model_args, "encoder_only", False):
            if self.hip_packed:
                from .biencoder import _log_fallback
                _log_fallback("hip_packed: padded path, a T5 reranker has no packed form")
            if self.hip_packed_train and torch.is_grad_enabled():
                from .biencoder import _log_fallback
                _log_fallback("hip_packed_train: no packed tower, a T5 reranker has no packed form")
            return self._encode_t5(items)
        if self.pooling not in ("first", "mean"):
            raise ValueError("Unknown pooling type: {}".format(self.pooling))
        dev = next(self.lm.parameters()).device
        # inference kernels only when no gradient can be asked for (grad mode off or a frozen
        # tower); eval mode with grad on returns differentiable scores as the reference does
        frozen = not any(p.requires_grad for p in self.lm.parameters())
        if dev.type == "cuda" and (not torch.is_grad_enabled() or frozen):
            enc, w = self._hip_state()
            mask = items.get("attention_mask")
            plan = None
            if self.hip_packed:   # padding-free: only the pairs' real tokens are computed
                from .biencoder import packed_plan
                plan = packed_plan(enc, items)
            if plan is not None:
                packed = enc.forward_packed(items["input_ids"], plan, items.get("token_type_ids"))
                _, rb = enc.pool_packed(packed, plan, items["input_ids"].shape[1], self.pooling, want_bf16=True)
                return linear_head(rb, w)
            hidden = enc(items["input_ids"], mask, items.get("token_type_ids"))
            _, rb = enc.pool(hidden, mask, self.pooling, want_bf16=True)
            return linear_head(rb, w)  # [B, 1] fp32
        if (dev.type == "cuda" and self.feature == "last_hidden_state"
                and tower_supported(self.lm) is None and items["input_ids"].shape[1] <= MAX_TRAIN_SEQ):
            # pair forward + backward on the HIP training tower (model/train_tower.py)
            plan = None
            if self.hip_packed_train:
                from .biencoder import packed_train_plan
                plan = packed_train_plan(items, dev)
            hidden = train_hidden(self.lm, items["input_ids"], items.get("attention_mask"),
                                  token_type_ids=items.get("token_type_ids"), plan=plan)
        else:
            from .biencoder import _log_fallback
            why = "tower on the CPU" if dev.type != "cuda" else tower_supported(self.lm) or "feature / length"
            if self.hip_packed_train:
                _log_fallback("hip_packed_train: no packed tower, " + why)
            _log_fallback("reranker: " + why)
            out = self.lm(**items, return_dict=True)
            hidden = getattr(out, self.feature)
        if self.pooling == "first":
            reps = hidden[:, 0, :]
        else:
            m = items.attention_mask.unsqueeze(-1).expand(hidden.size()).float()
            reps = torch.sum(hidden * m, 1) / torch.clamp(m.sum(1), min=1e-9)
        return self.head(reps)

    @classmethod
    def build(cls, model_args, data_args=None, train_args=None, tokenizer=None, **hf_kwargs):
        from transformers import T5EncoderModel, T5ForConditionalGeneration
        config = None
        hf_config = AutoConfig.from_pretrained(model_args.model_name_or_path, **hf_kwargs)
        if getattr(model_args, "encoder_only", False):
            model_class = T5EncoderModel
        elif "T5" in hf_config.architectures[0]:
            model_class = T5ForConditionalGeneration
        else:
            model_class = AutoModel
        cfg = os.path.join(model_args.model_name_or_path, "openmatch_config.json")
        if os.path.exists(cfg):
            with open(cfg) as f:
                config = json.load(f)
        if os.path.isdir(model_args.model_name_or_path) and config is not None:
            lm = model_class.from_pretrained(model_args.model_name_or_path, **hf_kwargs)
            head = LinearHead.load(ckpt_dir=model_args.model_name_or_path)
        else:
            lm = model_class.from_pretrained(model_args.model_name_or_path, **hf_kwargs)
            head = LinearHead(model_args.projection_in_dim, 1)
        return cls(lm=lm, head=head,
                   feature=model_args.feature if config is None else config["plm_backbone"]["feature"],
                   pooling=model_args.pooling if config is None else config["pooling"],
                   pos_token=model_args.pos_token if config is None else config["pos_token"],
                   neg_token=model_args.neg_token if config is None else config["neg_token"],
                   tokenizer=tokenizer, model_args=model_args, data_args=data_args, train_args=train_args)

    def save(self, output_dir: str):
        self.lm.save_pretrained(output_dir)
        self.head.save(output_dir)
        with open(os.path.join(output_dir, "openmatch_config.json"), "w") as f:
            json.dump(self._get_config_dict(), f, indent=4)

"""Drop-in for DRT/model/biencoder.py (DRModel, DRModelForInference, DROutput).

Same constructor, ``build``/``save``/``load``/``encode``/``forward`` contract
and checkpoint format (HF ``save_pretrained`` per tower + ``openmatch_config.json``,
biencoder.py:159-241).  What changes is where the arithmetic runs:

* encode without autograd (grad mode off or a frozen tower — Trainer.evaluate /
  _encoding_corpus, DRModelForInference) runs the whole tower on the HIP inference
  kernels (model/encoder.HipBertEncoder): bf16 MFMA GEMMs, fused attention, fp32
  LayerNorm statistics, pooling / head / L2-normalise kernels.  ``hidden`` is
  returned in bf16, ``reps`` in fp32.  ``encoder_only`` T5 towers (T5EncoderModel)
  take the same path through model/t5_encoder.HipT5Encoder.  With ``hip_packed = True``
  (attribute, or ``model_args.hip_packed``; default off) a BERT tower computes only the real
  tokens of a padded batch (model/packing.py, HipBertEncoder.forward_packed): ``reps`` as
  before, ``hidden`` [B, L, H] with ZEROS at the pad positions.  A mask that is not a batch of
  non-empty prefixes, a batch with too little padding and T5 towers keep the padded path.
* encode with autograd (training, or eval mode with grad on, where the reference
  returns differentiable reps) runs BERT towers up to L = 512 on the HIP training
  tower (model/train_tower.py: forward with saved bf16 activations + backward on
  HIP kernels, HF train-mode dropout regenerated from a counter hash; dropout is
  off in eval mode).  With ``hip_packed_train = True`` (attribute, or
  ``model_args.hip_packed_train``; default off, separate from ``hip_packed``) that tower
  runs on the packed real tokens of the batch (sequences up to 160 tokens, a padding share
  of at least ``packing.hip_packed_train_min_saving``; otherwise padded, logged once).
  ``encoder_only`` T5 towers stay on the HF module under
  autograd by default; with ``hip_train_t5 = True`` (attribute, or
  ``model_args.hip_train_t5``) a supported T5EncoderModel on the GPU runs the HIP
  T5 training tower (model/t5_train_tower.py: RMSNorm / ReLU / gated-GELU /
  relative-bias attention backwards, fp32 gradients for every HF parameter).
  Other towers, and the T5 reranker's decoder, stay on the HF module under autograd.
* the training score matrix + cross entropy (forward :107-119) runs on the
  fused fp32 kernels with autograd (torch.ops.drt.score_ce_fwd, score_ce.py); with
  ``forward(..., teacher_scores=)`` the distillation loss of torch.ops.drt.score_kd_fwd.
"""
from __future__ import annotations

import copy
import json
import logging
import os
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor
from transformers import AutoModel, BatchEncoding, PreTrainedModel
from transformers.modeling_outputs import ModelOutput

from .encoder import HipBertEncoder, l2_normalize_, linear_head
from . import packing
from .packing import plan_packing
from .t5_encoder import HipT5Encoder, t5_supported
from .train_tower import MAX_TRAIN_SEQ, tower_supported, train_hidden
from .t5_train_tower import t5_tower_supported, train_hidden_t5
from .linear import LinearHead

logger = logging.getLogger(__name__)


@dataclass
class DROutput(ModelOutput):
    q_reps: Tensor = None
    p_reps: Tensor = None
    loss: Tensor = None
    scores: Tensor = None


_FALLBACK_LOGGED = set()


def _log_fallback(why: str):
    """Once per reason: an encode that cannot take the HIP towers runs the HF module under torch
    (the reference's own arithmetic) -- say so instead of silently."""
    if why not in _FALLBACK_LOGGED:
        _FALLBACK_LOGGED.add(why)
        logger.warning("DRModel.encode: HF module under torch, not the HIP tower (%s)", why)


def packed_plan(enc, items):
    """The packing plan of a batch for an encode with ``hip_packed`` set, or None (padded path, the
    reason logged once): the tower is not a HipBertEncoder (T5 stays padded), or the mask is not a
    batch of non-empty prefixes with padding to drop (model/packing.py)."""
    if not isinstance(enc, HipBertEncoder):
        _log_fallback(f"hip_packed: padded path, {type(enc).__name__} has no packed form")
        return None
    ids = items["input_ids"]
    plan = plan_packing(items.get("attention_mask"), ids.shape[1], device=enc.device)
    if plan is None or plan.B != ids.shape[0]:
        _log_fallback("hip_packed: padded path, the mask is not a batch of non-empty prefixes with "
                      "enough padding to drop")
        return None
    return plan


def packed_train_plan(items, dev):
    """The packing plan of a batch for a training pass with ``hip_packed_train`` set, or None (padded
    tower, the reason logged once): the mask is not a batch of non-empty prefixes, or its padding
    share is below ``packing.hip_packed_train_min_saving``."""
    ids = items["input_ids"]
    plan = plan_packing(items.get("attention_mask"), ids.shape[1], device=dev,
                        min_saving=packing.hip_packed_train_min_saving)
    if plan is None or plan.B != ids.shape[0]:
        _log_fallback("hip_packed_train: padded tower, the mask is not a batch of non-empty prefixes with "
                      "enough padding to drop")
        return None
    return plan


def _torch_mean_pooling(h, mask):
    m = mask.unsqueeze(-1).expand(h.size()).float()
    return torch.sum(h * m, 1) / torch.clamp(m.sum(1), min=1e-9)


def _torch_max_pooling(h, mask):
    m = mask.unsqueeze(-1).expand(h.size()).float()
    return torch.max(h * m, 1)[0]


class DRModel(nn.Module):
    def __init__(self, lm_q: PreTrainedModel, lm_p: PreTrainedModel, tied: bool = True,
                 feature: str = "last_hidden_state", pooling: str = "first", head_q: nn.Module = None,
                 head_p: nn.Module = None, normalize: bool = False, model_args=None, data_args=None,
                 train_args=None):
        super().__init__()
        self.tied = tied
        self.lm_q = lm_q
        self.lm_p = lm_p
        self.head_q = head_q
        self.head_p = head_p
        self.loss_fn = nn.CrossEntropyLoss(reduction="mean")
        self.feature = feature
        self.pooling = pooling
        self.hip_train = True   # HIP training tower for BERT towers with L <= 512 (set False: HF autograd)
        # opt-in: T5EncoderModel towers with autograd on the HIP T5 training tower (default: HF module)
        self.hip_train_t5 = bool(getattr(model_args, "hip_train_t5", False))
        # opt-in: padding-free inference of BERT towers (only the real tokens of a padded batch are
        # computed; model/packing.py, HipBertEncoder.forward_packed)
        self.hip_packed = bool(getattr(model_args, "hip_packed", False))
        # opt-in: padding-free TRAINING of BERT towers (the autograd pass of train_hidden on the packed
        # rows; model/train_tower.py).  Separate from hip_packed, which covers the no-grad encode only.
        self.hip_packed_train = bool(getattr(model_args, "hip_packed_train", False))
        self.normalize = normalize
        self.model_args = model_args
        self.train_args = train_args
        self.data_args = data_args
        self._hip_cache: Dict[int, tuple] = {}
        if train_args is not None and getattr(train_args, "negatives_x_device", False):
            if not dist.is_initialized():
                raise ValueError("Distributed training has not been initialized for representation all gather.")
            self.process_rank = dist.get_rank()
            self.world_size = dist.get_world_size()

    def _get_config_dict(self):
        return {
            "tied": self.tied,
            "plm_backbone": {"type": type(self.lm_q).__name__, "feature": self.feature},
            "pooling": self.pooling,
            "linear_head": bool(self.head_q),
            "normalize": self.normalize,
        }

    # ------------------------------------------------------------------
    def forward(self, query: Dict[str, Tensor] = None, passage: Dict[str, Tensor] = None,
                teacher_scores: Optional[Tensor] = None):
        q_hidden, q_reps = self.encode_query(query)
        p_hidden, p_reps = self.encode_passage(passage)
        if query is None or passage is None:
            return DROutput(q_reps=q_reps, p_reps=p_reps)
        x_dev = bool(self.train_args is not None and getattr(self.train_args, "negatives_x_device", False))
        if x_dev:
            q_reps = self.dist_gather_tensor(q_reps)
            p_reps = self.dist_gather_tensor(p_reps)
            if teacher_scores is not None:
                teacher_scores = self.dist_gather_tensor(teacher_scores.detach())
        n_passages = self.data_args.train_n_passages
        scale = float(self.world_size) if (self.training and x_dev) else 1.0
        from ..score_ce import score_ce, score_kd
        if teacher_scores is None:
            def score(q, p, t):
                return score_ce(q, p, n_passages, scale)
        else:
            # distillation towards a cross-encoder's scores [B, n_passages] (trainer/distill.py)
            kd = dict(temperature=float(getattr(self.train_args, "distill_temperature", 1.0)),
                      w_ce=float(getattr(self.train_args, "distill_ce_weight", 0.0)),
                      w_kd=float(getattr(self.train_args, "distill_kd_weight", 1.0)), scale=scale)

            def score(q, p, t):
                return score_kd(q, p, t.to(q.device), n_passages, **kd)
        if q_reps.is_cuda:
            loss, scores = score(q_reps, p_reps, teacher_scores)
        elif torch.cuda.is_available():
            # a tower on the CPU (the reference scores on any device, biencoder.py:107-116): the reps go to
            # the GPU for the fused HIP op and the loss / scores come back; autograd carries the gradients
            # across both copies to the CPU tower
            dev = torch.device("cuda", torch.cuda.current_device())
            loss, scores = score(q_reps.to(dev), p_reps.to(dev), teacher_scores)
            loss, scores = loss.to(q_reps.device), scores.to(q_reps.device)
        else:
            raise ValueError("DRModel.forward: the MI355X build computes the score matrix on the GPU only "
                             "(no GPU visible)")
        return DROutput(loss=loss, scores=scores, q_reps=q_reps, p_reps=p_reps)

    # ------------------------------------------------------------------
    def _hip_encoder(self, model):
        """HipBertEncoder / HipT5Encoder snapshot of the tower, rebuilt when a parameter changes."""
        dev = next(model.parameters()).device
        key = id(model)
        ver = tuple(p._version for p in model.parameters()) + (str(dev),)
        hit = self._hip_cache.get(key)
        if hit is None or hit[0] != ver:
            name = type(model).__name__
            if name == "BertModel":
                enc = HipBertEncoder.from_hf(model, dev)
            elif name == "T5EncoderModel":
                why = t5_supported(model)
                if why is not None:
                    raise NotImplementedError(f"HIP T5 encoder: {why}")
                enc = HipT5Encoder.from_hf(model, dev)
            else:
                raise NotImplementedError(f"HIP encoder supports BERT-family towers only (got {name})")
            self._hip_cache[key] = (ver, enc)
            return enc
        return hit[1]

    def _head_weight(self, head) -> torch.Tensor:
        w = head.linear.weight
        key = id(head)
        ver = (w._version, str(w.device))
        hit = self._hip_cache.get(key)
        if hit is None or hit[0] != ver:
            wb = w.detach().to(torch.bfloat16).contiguous()
            self._hip_cache[key] = (ver, wb)
            return wb
        return hit[1]

    def _use_hip(self, model) -> bool:
        """Inference kernels (no autograd) when no gradient can be asked for: grad mode off, or
        a frozen tower.  Eval mode with grad on (the reference returns differentiable reps
        there) takes the training tower, which drops dropout when the module is in eval."""
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            return False
        return not torch.is_grad_enabled() or not any(p.requires_grad for p in model.parameters())

    def encode(self, items, model, head):
        if items is None:
            return None, None
        items = BatchEncoding(items)
        if "T5" in type(model).__name__ and not getattr(self.model_args, "encoder_only", False):
            raise NotImplementedError("T5 towers are outside the MI355X hot path (BERT-family encoders only)")
        if self.pooling not in ("first", "mean", "max"):
            raise ValueError("Unknown pooling type: {}".format(self.pooling))
        # a feature other than last_hidden_state (arguments.py:34-37) is off the HIP path in both modes:
        # it takes the HF module below, with the reason logged, whether or not autograd is on
        if self._use_hip(model) and self.feature == "last_hidden_state":
            enc = self._hip_encoder(model)
            plan = packed_plan(enc, items) if self.hip_packed else None
            if plan is not None:
                # padding-free: only the real tokens are computed; `hidden` comes back in the padded
                # [B, L, H] layout with ZEROS at the pad positions (the padded path leaves the
                # encoder's values of the pad tokens there, which the reference never reads)
                L = items["input_ids"].shape[1]
                packed = enc.forward_packed(items["input_ids"], plan, items.get("token_type_ids"))
                reps, rb = enc.pool_packed(packed, plan, L, self.pooling, want_bf16=head is not None)
                hidden = enc.unpack(packed, plan, L)
            else:
                hidden = enc(items["input_ids"], items.get("attention_mask"), items.get("token_type_ids"))
                reps, rb = enc.pool(hidden, items.get("attention_mask"), self.pooling, want_bf16=head is not None)
            if head is not None:
                reps = linear_head(rb, self._head_weight(head))
            if self.normalize:
                reps, _ = l2_normalize_(reps)
            return hidden, reps
        # forward with autograd: BERT towers up to MAX_TRAIN_SEQ tokens run the HIP training tower
        # (saved bf16 activations + backward on HIP kernels, HF dropout semantics in train mode,
        # model/train_tower.py), T5EncoderModel towers the T5 one when hip_train_t5 is set
        # (model/t5_train_tower.py); anything else keeps the HF module under autograd.
        why = None
        is_t5 = type(model).__name__ == "T5EncoderModel"
        if self.feature != "last_hidden_state":
            why = f"feature {self.feature!r}"
        elif is_t5 and not self.hip_train_t5:
            why = "T5 tower with hip_train_t5 = False"
        elif is_t5 and not next(model.parameters()).is_cuda:
            why = "tower on the CPU"
        elif is_t5:
            why = t5_tower_supported(model, items["input_ids"].shape[1])
        elif not self.hip_train:
            why = "hip_train = False"
        elif not next(model.parameters()).is_cuda:
            why = "tower on the CPU"
        elif items["input_ids"].shape[1] > MAX_TRAIN_SEQ:
            why = f"sequence length {items['input_ids'].shape[1]} > {MAX_TRAIN_SEQ}"
        else:
            why = tower_supported(model)
        if self.hip_packed_train and (why is not None or is_t5):
            _log_fallback("hip_packed_train: no packed tower, " + (why or "a T5 tower has no packed form"))
        if why is None and is_t5:
            hidden = train_hidden_t5(model, items["input_ids"], items.get("attention_mask"))
        elif why is None:
            plan = packed_train_plan(items, next(model.parameters()).device) if self.hip_packed_train else None
            hidden = train_hidden(model, items["input_ids"], items.get("attention_mask"),
                                  token_type_ids=items.get("token_type_ids"), plan=plan)
        else:
            _log_fallback(why)
            out = model(**items, return_dict=True)
            hidden = getattr(out, self.feature)
        if self.pooling == "first":
            reps = hidden[:, 0, :]
        elif self.pooling == "mean":
            reps = _torch_mean_pooling(hidden, items.attention_mask)
        else:
            reps = _torch_max_pooling(hidden, items.attention_mask)
        if head is not None:
            reps = head(reps)
        if self.normalize:
            reps = F.normalize(reps, dim=1)
        return hidden, reps

    def encode_passage(self, psg):
        return self.encode(psg, self.lm_p, self.head_p)

    def encode_query(self, qry):
        return self.encode(qry, self.lm_q, self.head_q)

    # ------------------------------------------------------------------
    @classmethod
    def build(cls, model_args, data_args=None, train_args=None, **hf_kwargs):
        from transformers import T5EncoderModel
        config = None
        model_class = T5EncoderModel if getattr(model_args, "encoder_only", False) else AutoModel
        head_q = head_p = None
        cfg_path = os.path.join(model_args.model_name_or_path, "openmatch_config.json")
        if os.path.exists(cfg_path):
            with open(cfg_path) as f:
                config = json.load(f)
        if os.path.isdir(model_args.model_name_or_path) and config is not None:
            tied = config["tied"]
            if tied:
                lm_q = lm_p = model_class.from_pretrained(model_args.model_name_or_path, **hf_kwargs)
                if config["linear_head"]:
                    head_q = head_p = LinearHead.load(model_args.model_name_or_path)
            else:
                root = model_args.model_name_or_path
                lm_q = model_class.from_pretrained(os.path.join(root, "query_model"), **hf_kwargs)
                lm_p = model_class.from_pretrained(os.path.join(root, "passage_model"), **hf_kwargs)
                if config["linear_head"]:
                    head_q = LinearHead.load(os.path.join(root, "query_head"))
                    head_p = LinearHead.load(os.path.join(root, "passage_head"))
        else:
            tied = not model_args.untie_encoder
            lm_q = model_class.from_pretrained(model_args.model_name_or_path, **hf_kwargs)
            lm_p = copy.deepcopy(lm_q) if not tied else lm_q
            if model_args.add_linear_head:
                head_q = LinearHead(model_args.projection_in_dim, model_args.projection_out_dim)
                head_p = copy.deepcopy(head_q) if not tied else head_q
        return cls(
            lm_q=lm_q, lm_p=lm_p, tied=tied,
            feature=model_args.feature if config is None else config["plm_backbone"]["feature"],
            pooling=model_args.pooling if config is None else config["pooling"],
            head_q=head_q, head_p=head_p,
            normalize=model_args.normalize if config is None else config["normalize"],
            model_args=model_args, data_args=data_args, train_args=train_args,
        )

    def save(self, output_dir: str):
        if not self.tied:
            os.makedirs(os.path.join(output_dir, "query_model"), exist_ok=True)
            os.makedirs(os.path.join(output_dir, "passage_model"), exist_ok=True)
            self.lm_q.save_pretrained(os.path.join(output_dir, "query_model"))
            self.lm_p.save_pretrained(os.path.join(output_dir, "passage_model"))
            if self.head_q is not None:
                os.makedirs(os.path.join(output_dir, "query_head"), exist_ok=True)
                os.makedirs(os.path.join(output_dir, "passage_head"), exist_ok=True)
                self.head_q.save(os.path.join(output_dir, "query_head"))
                self.head_p.save(os.path.join(output_dir, "passage_head"))
        else:
            self.lm_q.save_pretrained(output_dir)
            if self.head_q is not None:
                self.head_q.save(output_dir)
        with open(os.path.join(output_dir, "openmatch_config.json"), "w") as f:
            json.dump(self._get_config_dict(), f, indent=4)

    def dist_gather_tensor(self, t: Optional[torch.Tensor]):
        if t is None:
            return None
        # same semantics as the reference (biencoder.py:243-254): the other ranks' slices are
        # detached copies, this rank's slice is `t` itself so its gradient flows back
        from .. import comm
        t = t.contiguous()
        all_tensors = comm.all_gather_list(t)
        all_tensors[self.process_rank] = t
        return torch.cat(all_tensors, dim=0)

    def get_model_ckpt(self):
        return self.lm_q.state_dict()

    def load(self, _state_dict):
        self.lm_q.load_state_dict(_state_dict)
        self.lm_p.load_state_dict(_state_dict)


class DRModelForInference(DRModel):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    @torch.no_grad()
    def encode_passage(self, psg):
        return super().encode_passage(psg)

    @torch.no_grad()
    def encode_query(self, qry):
        return super().encode_query(qry)

    def forward(self, query: Dict[str, Tensor] = None, passage: Dict[str, Tensor] = None):
        q_hidden, q_reps = self.encode_query(query)
        p_hidden, p_reps = self.encode_passage(passage)
        return DROutput(q_reps=q_reps, p_reps=p_reps)

"""Cross-encoder distillation for the bi-encoder (served as ``DRT.trainer.distill``).

Mined hard negatives contain false negatives; the remedy is to let a cross-encoder (``RRModel``) score
each query's own passages and train the bi-encoder towards that distribution.  The pieces:

* ``pack_pairs``      the bi-encoder's collated batch -> the cross-encoder's pair inputs, on the device
                      (the format of RRCollator.create_one_example + pad, DRT/dataset/data_collator.py:230-266)
* ``teacher_scores``  ``RRModel.encode`` of those pairs without autograd: the HIP inference tower
* ``DistillTrainer``  ``Trainer`` whose step hands the scores to ``DRModel.forward(teacher_scores=)``, i.e. to
                      the fused score + CE + KL loss (score_ce.score_kd, torch.ops.drt.score_kd_fwd)
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from .trainer import Trainer


def _lengths(items: Dict[str, Tensor]) -> Tensor:
    ids = items["input_ids"]
    mask = items.get("attention_mask")
    if mask is None:
        return torch.full((ids.shape[0],), ids.shape[1], dtype=torch.long, device=ids.device)
    return mask.to(torch.long).sum(1)   # right-padded


def pack_pairs(query: Dict[str, Tensor], passage: Dict[str, Tensor], n_passages: int, pad_token_id: int):
    """Pair inputs [B * n, Lq + Lp] for query [B, Lq] and passage [B * n, Lp] batches: row i * n + j is
    ``q_ids[i, :lq_i]`` followed by ``p_ids[i * n + j, 1:lp]`` ([CLS] q [SEP] p [SEP]), padded with
    ``pad_token_id``.  Returns ``{"input_ids", "attention_mask"}`` (no token types, as RRCollator)."""
    q_ids, p_ids = query["input_ids"], passage["input_ids"]
    n = int(n_passages)
    if n < 1 or p_ids.shape[0] != q_ids.shape[0] * n:
        raise ValueError(f"{p_ids.shape[0]} passages for {q_ids.shape[0]} queries x {n} passages per query")
    Lq, Lp = q_ids.shape[1], p_ids.shape[1]
    lq = _lengths(query).repeat_interleave(n).unsqueeze(1)            # [R, 1]
    lp = _lengths(passage).unsqueeze(1)
    pos = torch.arange(Lq + Lp, device=q_ids.device).unsqueeze(0)     # [1, L]
    from_q = pos < lq
    from_p = ~from_q & (pos < lq + (lp - 1).clamp(min=0))
    qg = q_ids.repeat_interleave(n, dim=0).gather(1, pos.clamp(max=Lq - 1).expand(lq.shape[0], -1))
    pg = p_ids.gather(1, (pos - lq + 1).clamp(min=0, max=Lp - 1))
    ids = torch.where(from_q, qg, torch.where(from_p, pg, torch.full_like(pg, int(pad_token_id))))
    return {"input_ids": ids, "attention_mask": (from_q | from_p).to(torch.long)}


def teacher_scores(rr_model, query: Dict[str, Tensor], passage: Dict[str, Tensor], n_passages: int,
                   pad_token_id: int, chunk: int = 256) -> Tensor:
    """[B, n] fp32 cross-encoder scores of every query's own passages (no autograd: RRModel.encode
    takes the HIP inference tower), ``chunk`` pairs per tower pass.  A T5 teacher's two columns
    (neg, pos logits) are reduced to monoT5's relevance log_softmax(scores, -1)[:, 1]."""
    from ..model.reranker import relevance
    pairs = pack_pairs(query, passage, n_passages, pad_token_id)
    rows = pairs["input_ids"].shape[0]
    out = []
    with torch.no_grad():
        for a in range(0, rows, int(chunk)):
            scores = rr_model.encode({k: v[a: a + chunk] for k, v in pairs.items()})
            out.append(relevance(scores).float().reshape(-1))
    return torch.cat(out).view(rows // int(n_passages), int(n_passages))


class DistillTrainer(Trainer):
    """``Trainer`` with a frozen cross-encoder ``teacher`` (an RRModel).  The teacher lives on this rank's
    device, is never wrapped in DDP and never reaches the optimizer.  A loader that supplies
    ``batch[2]["teacher_scores"]`` ([B, n], e.g. precomputed) is taken at its word; otherwise the teacher
    scores the batch on the fly.  Temperature and weights come from the training arguments
    (distill_temperature / distill_ce_weight / distill_kd_weight, read by DRModel.forward)."""

    def __init__(self, training_args, model, teacher, pad_token_id: Optional[int] = None, teacher_chunk: int = 256,
                 **loaders):
        super().__init__(training_args, model, **loaders)
        self.teacher = teacher.to(self.device).eval().requires_grad_(False)
        if pad_token_id is None:
            pad_token_id = getattr(getattr(teacher, "tokenizer", None), "pad_token_id", None)
        self.pad_token_id = 0 if pad_token_id is None else int(pad_token_id)
        self.teacher_chunk = int(teacher_chunk)

    def train_step(self, inputs):
        extra = inputs[2] if len(inputs) > 2 and isinstance(inputs[2], dict) else {}
        scores = extra.get("teacher_scores")
        if scores is None:
            scores = teacher_scores(self.teacher, inputs[0], inputs[1], self.module.data_args.train_n_passages,
                                    self.pad_token_id, self.teacher_chunk)
        return self.model(query=inputs[0], passage=inputs[1], teacher_scores=scores).loss

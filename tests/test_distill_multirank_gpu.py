"""GPU, two ranks: the distillation loss under negatives_x_device as real processes over gloo (the ranks share
the one GPU of the test box, as tests/test_multirank_gpu.py).

Each rank holds half of one batch and its half of the teacher scores.  Representations and teacher scores are
all-gathered, every rank computes the global loss scaled by the world size (DDP averages the gradients), so
loss = world x the single-process score_kd loss and a rank's gradients = world x its rows of the single-process
gradients -- for DistributedDistillContrastiveLoss on given representations and for DRModel.forward on a tower.
Tolerances as tests/test_score_kd_gpu.py: loss rtol 1e-5, gradients rtol 1e-4 / atol 1e-6.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KD = dict(temperature=2.0, w_ce=0.5, w_kd=1.5)


def _w_distill(rank, world, dev):
    import torch
    from types import SimpleNamespace
    from transformers import BertModel
    from oracle import bert_weights as bw
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.score_ce import score_kd
    from denseretrievaltoolkits_amd.trainer.losses import DistributedDistillContrastiveLoss

    # ---- the loss on given representations: one batch of 6 queries x 3 passages, split in two
    B, n, d = 6, 3, 96
    gen = torch.Generator().manual_seed(17)          # the same full batch on every rank
    q = torch.randn(B, d, generator=gen).to(dev)
    p = torch.randn(B * n, d, generator=gen).to(dev)
    t = (torch.randn(B, n, generator=gen) * 3.0).to(dev)
    t[1, 2] = -math.inf                              # rank 0 drops a passage,
    t[4] = -math.inf                                 # rank 1 a whole query
    qs, ps = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
    single, _ = score_kd(qs, ps, t, n, **KD)
    single.backward()
    b = B // world
    rows, prow = slice(rank * b, (rank + 1) * b), slice(rank * b * n, (rank + 1) * b * n)
    ql, pl = q[rows].clone().requires_grad_(True), p[prow].clone().requires_grad_(True)
    loss = DistributedDistillContrastiveLoss(**KD)(ql, pl, t[rows])
    loss.backward()
    np.testing.assert_allclose(loss.item(), world * single.item(), rtol=1e-5)
    np.testing.assert_allclose(ql.grad.cpu().numpy(), world * qs.grad[rows].cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(pl.grad.cpu().numpy(), world * ps.grad[prow].cpu().numpy(), rtol=1e-4, atol=1e-6)

    # ---- DRModel.forward(teacher_scores=) with negatives_x_device on the HIP training tower (dropout off)
    torch.manual_seed(0)
    lm = BertModel(bw.bert_config(layers=1), add_pooling_layer=False)
    bw.init_model_(lm, 5)
    lm = lm.to(dev).train()
    model = DRModel(lm_q=lm, lm_p=lm, pooling="first", data_args=SimpleNamespace(train_n_passages=n),
                    train_args=SimpleNamespace(negatives_x_device=True, distill_temperature=KD["temperature"],
                                               distill_ce_weight=KD["w_ce"], distill_kd_weight=KD["w_kd"])).train()
    qi, qm = bw.token_batch(b, 16, seed=100 + rank)
    pi, pm = bw.token_batch(b * n, 32, seed=200 + rank)
    o = model(query={"input_ids": torch.from_numpy(qi).to(dev), "attention_mask": torch.from_numpy(qm).to(dev)},
              passage={"input_ids": torch.from_numpy(pi).to(dev), "attention_mask": torch.from_numpy(pm).to(dev)},
              teacher_scores=t[rows])
    assert o.q_reps.shape == (B, 768) and o.p_reps.shape == (B * n, 768) and o.scores.shape == (B, B * n)
    o.q_reps.retain_grad()
    o.p_reps.retain_grad()
    o.loss.backward()
    qa, pa = o.q_reps.detach().clone().requires_grad_(True), o.p_reps.detach().clone().requires_grad_(True)
    ref, _ = score_kd(qa, pa, t, n, **KD)            # single process: the gathered batch, all teacher rows
    ref.backward()
    np.testing.assert_allclose(o.loss.item(), world * ref.item(), rtol=1e-5)
    np.testing.assert_allclose(o.q_reps.grad.cpu().numpy(), world * qa.grad.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(o.p_reps.grad.cpu().numpy(), world * pa.grad.cpu().numpy(), rtol=1e-4, atol=1e-6)
    g = lm.embeddings.word_embeddings.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    return {"loss": o.loss.item(), "loss_reps": loss.item()}


def test_distill_negatives_x_device_world2():
    from test_multirank_gpu import _spawn
    res = _spawn(_w_distill, 2)
    assert set(res) == {0, 1}
    for key in ("loss", "loss_reps"):   # the x-device loss is the same global quantity on every rank
        assert abs(res[0][key] - res[1][key]) <= 1e-5 * abs(res[0][key])

"""T5 rerankers on the HIP path (model/t5_decoder.py HipT5PairScorer, RRModel.encode's T5 branch,
trainer/distill.py teacher_scores) against the HF T5ForConditionalGeneration in fp32, same process.

Models: tests/t5_decoder_refs.py (small seeded modules, cross-attention queries times 4 so that the
cross-attention is far from uniform; the helper asserts that on the HF reference itself).

Tolerances.  Final decoder state: per-row cosine >= 0.999, the project's tolerance for a bf16 tower
against HF fp32.  Logits: 2 x the largest |HF bf16 - HF fp32| over the full-vocabulary row of the
same module and batch, computed here on the CPU (the full-vocabulary maximum over 4 x 1024 values is
a stable scale of bf16 error in this model, about four standard deviations; this path rounds at
other points than HF's bf16 run and the factor covers that; a missing output scale, a wrong token
row or swapped columns are off by the order of the logits themselves).

Measured on an MI355X (printed by the tests): see the docstring of test_scorer_matches_hf.
"""
import copy
import functools
import logging
from types import SimpleNamespace

import pytest

import t5_decoder_refs as dr
import t5_refs as tr

pytestmark = pytest.mark.gpu

COS_MIN = 0.999
TOKENS = (3, 7)          # (neg, pos)
# the three configurations, and the first with its own lm_head weight and no output scale
VARIANTS = [(0, False), (1, False), (2, False), (0, True)]
VARIANT_IDS = ["d256-relu", "d512-gated-gelu", "d768-relu", "d256-untied-unscaled"]


class _Tok:
    """Stub tokenizer: RRModel only asks it for the ids of the two relevance tokens."""
    pad_token_id = 0

    def __init__(self, table):
        self.table = table

    def encode(self, text, add_special_tokens=False):
        return [self.table[text]]


def _hf_tolerance(model, ids, mask, logits):
    """2 x max |HF bf16 - HF fp32| over the full vocabulary row."""
    lb, _, _, _ = dr.hf_step(copy.deepcopy(model).bfloat16(), ids, mask)
    return 2.0 * float((lb.float() - logits).abs().max())


@functools.lru_cache(maxsize=None)
def _setup(case_idx, plain_head):
    """The CPU fp32 module, its batch and HF's own results; shared by the tests, never modified."""
    d_model, enc_layers, dec_layers, heads, d_ff, act, B, L = dr.S2S_CASES[case_idx]
    cfg = dr.s2s_config(d_model, enc_layers, dec_layers, heads, d_ff, act, scale_outputs=not plain_head)
    model = dr.s2s_model(cfg, untie=plain_head)
    ids, mask = tr.t5_batch(B, L, seed=11)
    logits, hidden, enc, att = dr.hf_step(model, ids, mask, attentions=True)
    frac = dr.cross_entropy_fraction(att, L)
    # the inputs discriminate: no decoder layer's cross-attention is near uniform or near one-hot
    assert len(frac) == dec_layers and all(0.2 <= f <= 0.8 for f in frac), frac
    tol = _hf_tolerance(model, ids, mask, logits)
    return SimpleNamespace(model=model, cfg=cfg, ids=ids, mask=mask, logits=logits, hidden=hidden, enc=enc, tol=tol,
                           B=B, L=L)


def _rr(s, dev, pos=TOKENS[1], neg=TOKENS[0], model=None):
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    lm = copy.deepcopy(s.model if model is None else model).to(dev)
    return RRModel(lm, LinearHead(s.cfg.d_model, 1), pos_token="true", neg_token="false",
                   tokenizer=_Tok({"true": pos, "false": neg})).eval()


def _items(s, dev):
    return {"input_ids": s.ids.to(dev), "attention_mask": s.mask.to(dev)}


@pytest.mark.parametrize("case_idx,plain_head", VARIANTS, ids=VARIANT_IDS)
def test_scorer_matches_hf(dev, case_idx, plain_head):
    """decode_hidden: per-row cosine >= 0.999 against HF decoder_hidden_states[-1][:, 0]; logits of two
    token ids within 2 x max |HF bf16 - HF fp32|; and, on the CPU reference alone, the fp64 formula
    with uniform cross-attention probabilities is outside that tolerance (the inputs can tell).

    Measured on an MI355X (worst |logit error| / tolerance, min cosine): d256-relu 0.0265 / 0.0853,
    0.999958; d512-gated-gelu 0.0386 / 0.1441, 0.999809; d768-relu 0.0168 / 0.1155, 0.999898;
    d256-untied-unscaled 0.2771 / 1.3224 (logits of rms 15.7), 0.999958.  The tolerance itself (2 x the
    HF bf16 - fp32 maximum, computed on the CPU) read 0.085-0.144 on logits of rms 1."""
    import torch
    from denseretrievaltoolkits_amd.model.t5_decoder import HipT5PairScorer
    s = _setup(case_idx, plain_head)
    _, uniform = dr.decoder_step_ref(s.model, s.enc, s.mask, uniform=True)
    want = s.logits[:, list(TOKENS)]
    gap = float((uniform[:, list(TOKENS)] - want.double()).abs().max())
    assert gap > s.tol, f"uniform cross-attention within the tolerance ({gap} <= {s.tol})"

    scorer = HipT5PairScorer.from_hf(s.model, dev)
    with torch.no_grad():
        y = scorer.decode_hidden(s.ids.to(dev), s.mask.to(dev))
        got = scorer.logits(s.ids.to(dev), s.mask.to(dev), TOKENS)
    torch.cuda.synchronize()
    assert y.shape == s.hidden.shape and got.shape == (s.B, 2) and got.dtype == torch.float32
    cos = torch.nn.functional.cosine_similarity(y.float().cpu(), s.hidden, dim=1)
    err = float((got.cpu() - want).abs().max())
    print(f"{VARIANT_IDS[VARIANTS.index((case_idx, plain_head))]}: min cos {float(cos.min()):.6f}, worst logit error "
          f"{err:.4f}, tolerance {s.tol:.4f}, logits rms {float(s.logits.pow(2).mean().sqrt()):.3f}, "
          f"uniform-attention gap {gap:.3f}")
    assert torch.isfinite(got).all()
    assert cos.min() >= COS_MIN
    assert err <= s.tol
    # the rows are cached per token tuple, and another tuple gets its own rows
    with torch.no_grad():
        again = scorer.logits(s.ids.to(dev), s.mask.to(dev), TOKENS)
        swapped = scorer.logits(s.ids.to(dev), s.mask.to(dev), TOKENS[::-1])
    assert torch.equal(again, got) and torch.equal(swapped, got[:, [1, 0]])


def test_rrmodel_encode_t5_no_grad(dev):
    """Under no_grad on the GPU RRModel.encode returns [B, 2] fp32 = (neg, pos) logits on the HIP scorer
    (the call raised NotImplementedError before), within the logit tolerance of the HF module;
    swapping the two tokens swaps the columns."""
    import torch
    from denseretrievaltoolkits_amd.model.t5_decoder import HipT5PairScorer
    s = _setup(0, False)
    rr = _rr(s, dev)
    assert rr.loss_fn_str == "ce"
    with torch.no_grad():
        got = rr.encode(_items(s, dev))
        got2 = rr.encode(_items(s, dev))
        flipped = _rr(s, dev, pos=TOKENS[0], neg=TOKENS[1]).encode(_items(s, dev))
    assert isinstance(rr._hip[1], HipT5PairScorer)
    assert got.shape == (s.B, 2) and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
    assert torch.equal(got, got2)
    assert torch.equal(flipped, got[:, [1, 0]])
    want = s.logits[:, [TOKENS[0], TOKENS[1]]]
    err = float((got.cpu() - want).abs().max())
    print(f"RRModel t5 encode: worst logit error {err:.4f}, tolerance {s.tol:.4f}")
    assert err <= s.tol
    assert float((want[:, 0] - want[:, 1]).abs().min()) > 0      # the column check means something


def test_rrmodel_resnapshots_t5_weights(dev):
    """An in-place update of a decoder weight bumps its _version: the next encode uses the new weights."""
    import torch
    s = _setup(0, False)
    rr = _rr(s, dev)
    with torch.no_grad():
        a = rr.encode(_items(s, dev))
        g = torch.Generator().manual_seed(0)
        w = rr.lm.decoder.block[1].layer[2].DenseReluDense.wo.weight
        w.add_((0.1 * torch.randn(w.shape, generator=g)).to(dev))
        b = rr.encode(_items(s, dev))
    assert not torch.equal(a, b)
    want, _, _, _ = dr.hf_step(copy.deepcopy(rr.lm).cpu(), s.ids, s.mask)
    assert float((b.cpu() - want[:, list(TOKENS)]).abs().max()) <= s.tol


def test_rrmodel_t5_grad_on_keeps_hf_module(dev, caplog):
    """With autograd on the HF module computes the scores as the reference does: they carry a graph,
    the fallback is logged, and the values are HF's."""
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    s = _setup(0, False)
    rr = _rr(s, dev)
    biencoder._FALLBACK_LOGGED.clear()
    with caplog.at_level(logging.WARNING, logger=biencoder.logger.name):
        got = rr.encode(_items(s, dev))
    assert got.requires_grad and got.grad_fn is not None and got.shape == (s.B, 2)
    assert any("HF module under torch" in r.getMessage() and "T5 reranker" in r.getMessage() for r in caplog.records)
    assert rr._hip is None
    torch.testing.assert_close(got.detach().float().cpu(), s.logits[:, list(TOKENS)], atol=1e-3, rtol=1e-3)


def test_rrmodel_unsupported_t5_config_raises(dev):
    import torch
    s = _setup(0, False)
    lm = dr.s2s_model(dr.s2s_config(256, 1, 1, 4, 512, "relu", d_kv=32))
    rr = _rr(s, dev, model=lm)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="d_kv 32"):
        rr.encode(_items(s, dev))


def test_rrmodel_t5_forward_ce_loss(dev):
    """forward(pos_pairs, neg_pairs) with equal shapes: a finite cross-entropy loss over the (neg, pos)
    columns (label 1 for the positive pairs, 0 for the negative ones)."""
    import torch
    import torch.nn.functional as F
    s = _setup(0, False)
    rr = _rr(s, dev)
    ids2, mask2 = tr.t5_batch(s.B, s.L, seed=12)
    with torch.no_grad():
        out = rr(pos_pairs=_items(s, dev), neg_pairs={"input_ids": ids2.to(dev), "attention_mask": mask2.to(dev)})
    assert out.pos_pair_scores.shape == out.neg_pair_scores.shape == (s.B, 2)
    assert out.loss.dim() == 0 and torch.isfinite(out.loss)
    want = (F.cross_entropy(out.pos_pair_scores.cpu(), torch.ones(s.B, dtype=torch.long))
            + F.cross_entropy(out.neg_pair_scores.cpu(), torch.zeros(s.B, dtype=torch.long)))
    torch.testing.assert_close(out.loss.cpu(), want, atol=1e-5, rtol=1e-5)


def test_teacher_scores_t5_teacher(dev):
    """teacher_scores with a T5 teacher: [B, n] = log_softmax of the HF (neg, pos) logits at index 1,
    within the logit tolerance of the pair batch; chunking keeps the layout."""
    import torch
    from denseretrievaltoolkits_amd.trainer.distill import pack_pairs, teacher_scores
    s = _setup(0, False)
    rr = _rr(s, dev).requires_grad_(False)
    B, n = 3, 2
    qi, qm = tr.t5_batch(B, 12, seed=21)
    pi, pm = tr.t5_batch(B * n, 30, seed=22)
    query = {"input_ids": qi.to(dev), "attention_mask": qm.to(dev)}
    passage = {"input_ids": pi.to(dev), "attention_mask": pm.to(dev)}
    got = teacher_scores(rr, query, passage, n, 0)
    assert got.shape == (B, n) and got.dtype == torch.float32
    pairs = {k: v.cpu() for k, v in pack_pairs(query, passage, n, 0).items()}
    logits, _, _, _ = dr.hf_step(s.model, pairs["input_ids"], pairs["attention_mask"])
    tol = _hf_tolerance(s.model, pairs["input_ids"], pairs["attention_mask"], logits)
    want = torch.log_softmax(logits[:, list(TOKENS)], -1)[:, 1].view(B, n)
    err = float((got.cpu() - want).abs().max())
    print(f"teacher_scores t5: worst error {err:.4f}, tolerance {tol:.4f}")
    assert err <= tol
    chunks = teacher_scores(rr, query, passage, n, 0, chunk=4)
    assert float((chunks.cpu() - want).abs().max()) <= tol


def test_teacher_scores_bert_teacher_unchanged(dev):
    """A one-column (BERT) teacher's scores are RRModel.encode's own, bit for bit."""
    import torch
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    from denseretrievaltoolkits_amd.trainer.distill import pack_pairs, teacher_scores
    from test_score_kd_gpu import _batch, _tower
    B, n = 4, 3
    torch.manual_seed(3)
    rr = RRModel(lm=_tower(1, 2, dev), head=LinearHead(768, 1).to(dev), pooling="first").eval().requires_grad_(False)
    query, passage = _batch(dev, B, n, 16, 32)
    with torch.no_grad():
        enc = rr.encode(pack_pairs(query, passage, n, 0))
    assert enc.shape == (B * n, 1)
    assert torch.equal(teacher_scores(rr, query, passage, n, 0), enc.float().reshape(-1).view(B, n))

"""GPU parity of the HIP T5 encoder forward (model/t5_encoder.HipT5Encoder) against HF
T5EncoderModel in fp32, in the same process, and DRModel's dispatch of ``encoder_only`` towers.

The build computes in bf16 with fp32 accumulation, so parity is the project's tolerance: per-token
cosine of last_hidden_state >= 0.999 on unmasked tokens (COS_MIN of tests/test_encoder_gpu.py).
HF's own bf16 run of these models reaches >= 0.9997 against fp32 on a CPU, while dropping the
relative bias gives 0.79-0.87 and scaling Q by 1/8 gives 0.87-0.94.  Measured on an MI355X: minimum
cosine 0.999981 / 0.999965 / 0.999970 / 0.999949 over the four configurations of t5_refs.T5_CASES,
>= 0.999977 on DRModel's pooled reps.
"""
import logging
from types import SimpleNamespace

import pytest

import t5_refs as tr

pytestmark = pytest.mark.gpu

COS_MIN = 0.999


def _cos(a, b):
    import torch
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


@pytest.mark.parametrize("d_model,layers,heads,d_ff,act,B,L", tr.T5_CASES)
def test_hidden_states_vs_hf_fp32(dev, d_model, layers, heads, d_ff, act, B, L):
    import torch
    from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder
    m = tr.t5_model(tr.t5_config(d_model, layers, heads, d_ff, act))
    ids, mask = tr.t5_batch(B, L, seed=B + L)
    with torch.no_grad():
        ref = m(input_ids=ids, attention_mask=mask).last_hidden_state
    enc = HipT5Encoder.from_hf(m, dev)
    out = enc(ids.to(dev), mask.to(dev))
    assert out.shape == (B, L, d_model) and out.dtype == torch.bfloat16
    out = out.float().cpu()
    valid = mask.bool()
    cos = _cos(out[valid], ref[valid])
    print(f"t5 d_model={d_model} layers={layers} heads={heads} {act} B={B} L={L}: min cos {float(cos.min()):.6f}, "
          f"max abs err {float((out[valid] - ref[valid]).abs().max()):.4f}")
    assert torch.isfinite(out).all()
    assert cos.min() >= COS_MIN


def test_two_stream_halves_bit_identical(dev):
    """The two-stream driver gives the bits of one pass."""
    import torch
    from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder
    m = tr.t5_model(tr.t5_config(256, 2, 2, 512, "gated-gelu"))
    ids, mask = tr.t5_batch(5, 40, seed=3)
    enc = HipT5Encoder.from_hf(m, dev)
    enc.split_streams = False
    one = enc(ids.to(dev), mask.to(dev))
    enc.split_streams, enc.split_min_tokens = True, 1
    two = enc(ids.to(dev), mask.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))


def test_encoder_rejects_long_sequences_and_token_types(dev):
    import torch
    from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder
    enc = HipT5Encoder.from_hf(tr.t5_model(tr.t5_config(256, 1, 4, 512, "relu")), dev)
    with pytest.raises(ValueError, match="513"):
        enc(torch.ones(1, 513, dtype=torch.int64))
    with pytest.raises(ValueError, match="token_type_ids"):
        enc(torch.ones(1, 8, dtype=torch.int64), None, torch.zeros(1, 8, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------
# DRModel level
# ---------------------------------------------------------------------------------------------
def _drmodel(dev, tied, pooling, normalize, head):
    import copy
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    lm_q = tr.t5_model(tr.t5_config(256, 2, 4, 512, "relu"), seed=5).to(dev)
    lm_p = lm_q if tied else tr.t5_model(tr.t5_config(256, 2, 4, 512, "relu"), seed=7).to(dev)
    head_q = head_p = None
    if head:
        torch.manual_seed(11)
        head_q = LinearHead(256, 64).to(dev)
        head_p = head_q if tied else copy.deepcopy(head_q)
    return DRModel(lm_q, lm_p, tied=tied, pooling=pooling, head_q=head_q, head_p=head_p, normalize=normalize,
                   model_args=SimpleNamespace(encoder_only=True)).eval()


def _want_reps(lm, head, ids, mask, pooling, normalize):
    """The reference's formula on the HF module's fp32 hidden states (CPU)."""
    import copy
    import torch
    lm = copy.deepcopy(lm).cpu().float()
    with torch.no_grad():
        h = lm(input_ids=ids, attention_mask=mask).last_hidden_state
        if pooling == "first":
            reps = h[:, 0]
        else:
            mk = mask.unsqueeze(-1).float()
            reps = (h * mk).sum(1) / mk.sum(1).clamp(min=1e-9)
        if head is not None:
            reps = reps @ head.linear.weight.detach().cpu().float().T
        if normalize:
            reps = torch.nn.functional.normalize(reps, dim=1)
    return reps


@pytest.mark.parametrize("tied,pooling,normalize,head", [(True, "mean", False, False), (True, "mean", True, False),
                                                         (False, "first", True, False), (False, "mean", False, True),
                                                         (True, "first", False, False)])
def test_drmodel_encodes_t5_towers_grad_off(dev, tied, pooling, normalize, head):
    """DRModel.forward under no_grad runs encoder_only T5 towers on the HIP path (the call raised
    NotImplementedError before): q_reps / p_reps cosine >= 0.999 per row against the HF fp32 formula."""
    import torch
    model = _drmodel(dev, tied, pooling, normalize, head)
    qi, qm = tr.t5_batch(3, 24, seed=1)
    pi, pm = tr.t5_batch(4, 70, seed=2)
    with torch.no_grad():   # one side per call: with both, forward goes on to the training loss
        q_reps = model(query={"input_ids": qi.to(dev), "attention_mask": qm.to(dev)}).q_reps
        p_reps = model(passage={"input_ids": pi.to(dev), "attention_mask": pm.to(dev)}).p_reps
    from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder
    assert sum(isinstance(e, HipT5Encoder) for _, e in model._hip_cache.values()) == (1 if tied else 2)
    for name, got, lm, hd, ids, mask in (("q", q_reps, model.lm_q, model.head_q, qi, qm),
                                         ("p", p_reps, model.lm_p, model.head_p, pi, pm)):
        want = _want_reps(lm, hd, ids, mask, pooling, normalize)
        got = got.float().cpu()
        assert got.shape == want.shape and torch.isfinite(got).all()
        cos = _cos(got, want)
        print(f"DRModel t5 tied={tied} {pooling} normalize={normalize} head={head} {name}_reps: min cos "
              f"{float(cos.min()):.6f}")
        assert cos.min() >= COS_MIN
        if normalize:
            torch.testing.assert_close(got.norm(dim=1), torch.ones(got.shape[0]), atol=1e-5, rtol=0)


def test_drmodel_resnapshots_t5_weights(dev):
    """An in-place update of shared.weight bumps its _version: the next encode uses the new weights."""
    import torch
    model = _drmodel(dev, True, "mean", False, False)
    ids, mask = tr.t5_batch(3, 24, seed=1)
    batch = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}
    with torch.no_grad():
        _, a = model.encode_passage(batch)
        _, a2 = model.encode_passage(batch)
        assert torch.equal(a, a2)
        g = torch.Generator().manual_seed(0)
        w = model.lm_p.shared.weight
        w.add_(0.5 * torch.randn(w.shape, generator=g).to(dev))
        _, b = model.encode_passage(batch)
    assert not torch.equal(a, b)
    want = _want_reps(model.lm_p, None, ids, mask, "mean", False)
    assert _cos(b.float().cpu(), want).min() >= COS_MIN


def test_drmodel_unsupported_t5_config_raises(dev):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    lm = tr.t5_model(tr.t5_config(256, 1, 4, 512, "relu", d_kv=32)).to(dev)
    model = DRModel(lm, lm, pooling="mean", model_args=SimpleNamespace(encoder_only=True)).eval()
    ids, mask = tr.t5_batch(2, 16, seed=1)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="d_kv 32"):
        model.encode_passage({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)})


def test_drmodel_t5_grad_on_keeps_hf_module(dev, caplog):
    """With autograd on, a T5 tower stays on the HF module and the fallback is logged (T5 training is
    out of scope): reps carry a graph and equal the HF formula on the module's own device."""
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    model = _drmodel(dev, True, "mean", False, False)
    ids, mask = tr.t5_batch(2, 16, seed=1)
    biencoder._FALLBACK_LOGGED.clear()
    with caplog.at_level(logging.WARNING, logger=biencoder.logger.name):
        hidden, reps = model.encode_passage({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)})
    assert reps.requires_grad and hidden.dtype == torch.float32
    assert any("HF module under torch" in r.getMessage() for r in caplog.records)
    assert not model._hip_cache
    want = _want_reps(model.lm_p, None, ids, mask, "mean", False)
    torch.testing.assert_close(reps.detach().float().cpu(), want, atol=1e-3, rtol=1e-3)

"""Padding-free T5 inference end to end: DRModel and RRModel with ``hip_packed_t5`` set, against HF fp32 with the
tolerances of tests/test_t5_encoder_gpu.py and tests/test_t5_reranker_gpu.py, and against the padded HIP path:
the packed error is at most 1.1 x the padded error, the factor tests/test_packed_encoder_gpu.py uses for BERT."""
import copy
from types import SimpleNamespace

import pytest
import torch

import t5_decoder_refs as dr
import t5_refs as tr

pytestmark = pytest.mark.gpu

COS_MIN = 0.999
ENTRY = "drt_attention_varlen_relbias_forward_bf16"
TOKENS = (3, 7)          # (neg, pos)


class _Spy:
    """Counts the calls of one native entry (the ctypes handle is shared by every encoder)."""

    def __init__(self, monkeypatch, name=ENTRY):
        from denseretrievaltoolkits_amd import _native
        lib = _native.load()
        self.calls = 0
        real = getattr(lib, name)

        def counted(*args):
            self.calls += 1
            return real(*args)

        monkeypatch.setattr(lib, name, counted)


def _pooled(h, mask, pooling):
    mk = mask.unsqueeze(-1).float()
    if pooling == "first":
        return h[:, 0]
    return (h * mk).sum(1) / mk.sum(1) if pooling == "mean" else (h * mk).max(1)[0]


@pytest.mark.parametrize("act", ["relu", "gated-gelu"])
def test_drmodel_hip_packed_t5_vs_hf_fp32(dev, monkeypatch, act):
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    cpu = tr.t5_model(tr.t5_config(256, 2, 4, 512, act))
    ids, mask = tr.t5_batch(6, 72, seed=4)
    with torch.no_grad():
        hid = cpu(input_ids=ids, attention_mask=mask).last_hidden_state
    lm = copy.deepcopy(cpu).to(dev)
    items = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}
    real = mask.bool()
    spy = _Spy(monkeypatch)
    for pooling in ("first", "mean", "max"):
        err = {}
        for flag in (False, True):
            model = DRModel(lm, lm, pooling=pooling,
                            model_args=SimpleNamespace(encoder_only=True, hip_packed_t5=flag)).eval()
            assert model.hip_packed_t5 is flag and model.hip_packed is False
            before = spy.calls
            with torch.no_grad():
                hidden, reps = model.encode(items, lm, None)
            assert spy.calls - before == (2 if flag else 0), "one varlen launch per layer, none with the flag off"
            hidden, reps = hidden.float().cpu(), reps.cpu()
            want = _pooled(hid, mask, pooling)
            assert hidden.shape == hid.shape and reps.shape == want.shape and torch.isfinite(reps).all()
            cos_r = torch.nn.functional.cosine_similarity(reps.double(), want.double(), dim=1)
            cos_h = torch.nn.functional.cosine_similarity(hidden[real].double(), hid[real].double(), dim=1)
            err[flag] = (float((reps - want).abs().max()), float((hidden[real] - hid[real]).abs().max()))
            print(f"DRModel t5 {act} {pooling} hip_packed_t5={flag}: min cos reps {float(cos_r.min()):.6f} hidden "
                  f"{float(cos_h.min()):.6f}, max abs err reps {err[flag][0]:.4f} hidden {err[flag][1]:.4f}")
            assert cos_r.min() >= COS_MIN and cos_h.min() >= COS_MIN
            if flag:
                assert (hidden[~real] == 0).all(), "pad rows of hidden are not zero"
        assert err[True][0] <= 1.1 * err[False][0] and err[True][1] <= 1.1 * err[False][1], (pooling, err)


def test_rrmodel_hip_packed_t5_scores(dev, monkeypatch):
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    cfg = dr.s2s_config(256, 2, 2, 4, 512, "relu")
    cpu = dr.s2s_model(cfg)
    ids, mask = tr.t5_batch(6, 160, seed=13)
    logits, _, _, _ = dr.hf_step(cpu, ids, mask)
    bf16, _, _, _ = dr.hf_step(copy.deepcopy(cpu).bfloat16(), ids, mask)
    tol = 2.0 * float((bf16.float() - logits).abs().max())
    want = logits[:, list(TOKENS)]
    tok = SimpleNamespace(pad_token_id=0, encode=lambda text, add_special_tokens=False: [{"false": 3, "true": 7}[text]])
    rr = RRModel(copy.deepcopy(cpu).to(dev), LinearHead(256, 1), "last_hidden_state", "first", "true", "false", tok).eval()
    items = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        padded = rr.encode(items)
        assert spy.calls == 0 and rr.hip_packed_t5 is False
        rr.hip_packed_t5 = True
        packed = rr.encode(items)
    assert spy.calls == 2 and packed.shape == (6, 2) and packed.dtype == torch.float32
    e_padded = float((padded.cpu() - want).abs().max())
    e_packed = float((packed.cpu() - want).abs().max())
    print(f"RRModel t5 scores: padded error {e_padded:.4f}, packed error {e_packed:.4f}, tolerance {tol:.4f}")
    assert e_packed <= tol
    assert e_packed <= 1.1 * e_padded

"""The padding-free training tower above 160 tokens end to end: DRModel / RRModel with
``hip_packed_train`` and ``hip_packed_train_long`` set against the same model with both off (the
comparison and tolerances of tests/test_packed_train_tower_gpu.py), the new backward entry called once
per layer, and the tail-row invariant of the gradients handed to a wgrad."""
import pytest

import test_packed_train_tower_gpu as pt
import test_train_tower_gpu as tt
from oracle import bert_weights as bw

pytestmark = pytest.mark.gpu

LONG_BWD = "drt_attention_varlen_long_backward_bf16"
BATCHES = {"3x192": (3, 192, (170, 40, 40)), "2x320": (2, 320, (300, 161))}


def _batch(name, dev):
    import torch
    B, L, lens = BATCHES[name]
    ids, mask = bw.token_batch(B, L, seed=L + B)
    mask[:] = 0
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    return torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("model", ["DRModel", "RRModel"])
def test_flags_on_against_flags_off(dev, monkeypatch, model, batch):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    layers = 2
    ids_t, mask_t = _batch(batch, dev)
    B = ids_t.shape[0]
    R = torch.randn(B, 768, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    spy_long, spy_short = pt._Spy(monkeypatch, LONG_BWD), pt._Spy(monkeypatch, pt.VARLEN_BWD)
    out = {}
    for flag in (False, True):
        lm = tt._bert(layers, 17, dev).train()
        torch.manual_seed(1)
        m = DRModel(lm, lm) if model == "DRModel" else RRModel(lm, LinearHead(768, 1).to(dev))
        m.hip_packed_train = m.hip_packed_train_long = flag
        before = spy_long.calls, spy_short.calls
        if model == "DRModel":
            hidden, reps = m.encode(pt._items(ids_t, mask_t), lm, None)
            loss = (reps * R).sum()
            if flag:
                assert (hidden[~mask_t.bool()] == 0).all()
        else:
            loss = (m.encode(pt._items(ids_t, mask_t)) * R[:, :1]).sum()
        loss.backward()
        # the long entry once per layer; the short sequences of the same batch through the short entry
        has_short = min(BATCHES[batch][2]) <= 160
        assert spy_long.calls - before[0] == (layers if flag else 0)
        assert spy_short.calls - before[1] == (layers if flag and has_short else 0)
        out[flag] = (loss.detach(), pt._grads(m))
    pt._close_to_flag_off(out[True][0], out[False][0], out[True][1], out[False][1])


def test_tail_rows_handed_to_wgrad_are_exact_zeros(dev, monkeypatch):
    import torch
    from denseretrievaltoolkits_amd.model import encoder_bwd, train_tower
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    layers = 2
    ids_t, mask_t = _batch("3x192", dev)
    plan = plan_packing(mask_t, 192, force=True)
    T, T32 = plan.T, (plan.T + 31) // 32 * 32
    assert T == 250 and T32 == 256
    seen = []
    real = encoder_bwd.wgrad
    monkeypatch.setattr(encoder_bwd, "wgrad", lambda dy, x: (seen.append((dy, x)), real(dy, x))[1])
    for p in (0.0, 0.1):
        m = tt._bert(layers, 31, dev).train()
        m.config.hidden_dropout_prob = m.config.attention_probs_dropout_prob = p
        seen.clear()
        train_tower.train_hidden(m, ids_t, mask_t, seed=77, plan=plan, packed_long=True).square().sum().backward()
        assert len(seen) == 4 * layers
        for dy, x in seen:
            assert dy.shape[0] == T32 and x.shape[0] == T32
            assert ((dy[T:].view(torch.int16) & 0x7FFF) == 0).all(), "a tail row of a gradient is not zero"
            assert torch.isfinite(x[T:].float()).all() and torch.isfinite(dy.float()).all()

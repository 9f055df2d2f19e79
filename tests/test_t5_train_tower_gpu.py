"""GPU: the HIP T5 training tower (model/t5_train_tower.py) against HF T5EncoderModel under torch
fp32 autograd on the same weights and inputs: the hidden state and every parameter gradient
(shared.weight, every norm weight and relative_attention_bias.weight included), train-mode dropout
against a functional fp32 reference that applies the kernels' masks, and DRModel's opt-in routing.

Bounds (those of tests/test_train_tower_gpu.py): hidden cos > 0.9999; per tensor cos > 0.995 and
relative error < 0.1.  A tensor that misses them is bounded by 1.5x the error of the HF module under
torch bf16 autocast against HF fp32 on the same inputs (the tower's bf16 rounding points differ from
autocast's); both figures are printed.
"""
import copy
import logging
from types import SimpleNamespace

import pytest

import t5_refs as tr
import t5_train_refs as ttr

pytestmark = pytest.mark.gpu

CONFIGS = [(256, 2, 4, 512, "relu"), (512, 1, 6, 1024, "gated-gelu"), (1024, 1, 16, 2048, "gated-gelu")]
SHAPES = [(4, 32), (3, 50), (2, 156), (2, 200)]


def _err(a, b):
    import torch
    a, b = a.flatten().double(), b.flatten().double()
    return float((a - b).norm() / b.norm()), float(torch.nn.functional.cosine_similarity(a, b, dim=0))


def _compare_grads(tag, m_hip, m_ref, autocast_grads):
    """Every parameter gradient of m_hip against m_ref's; ``autocast_grads()`` -> {name: grad} of the HF
    module under bf16 autocast, asked for only when a tensor misses the plain bounds."""
    worst, bad, ac = [], [], None
    for (n, p_ref), (n2, p_hip) in zip(m_ref.named_parameters(), m_hip.named_parameters()):
        assert n == n2
        assert p_ref.grad is not None and p_hip.grad is not None, n
        assert float(p_ref.grad.norm()) > 0, n
        rel, cos = _err(p_hip.grad, p_ref.grad)
        worst.append((rel, cos, n))
        if cos > 0.995 and rel < 0.1:
            continue
        if ac is None:
            ac = autocast_grads()
        rel_ac, cos_ac = _err(ac[n], p_ref.grad)
        print(f"{tag} {n}: HIP tower rel {rel:.4f} cos {cos:.6f} | HF bf16 autocast rel {rel_ac:.4f} cos {cos_ac:.6f}")
        if not (rel <= 1.5 * rel_ac and 1.0 - cos <= 1.5 * (1.0 - cos_ac)):
            bad.append((n, rel, cos, rel_ac, cos_ac))
    worst.sort(reverse=True)
    print(f"{tag} worst relative gradient errors:", [(round(r, 4), round(c, 6), n) for r, c, n in worst[:4]])
    assert not bad, bad


@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("d_model,layers,heads,d_ff,act", CONFIGS)
def test_tower_grads_vs_hf_autograd(dev, d_model, layers, heads, d_ff, act, B, L):
    import torch
    from denseretrievaltoolkits_amd.model.t5_train_tower import train_hidden_t5
    m_ref = tr.t5_model(tr.t5_config(d_model, layers, heads, d_ff, act), seed=3).to(dev).train()
    m_hip = copy.deepcopy(m_ref)
    ids, mask = tr.t5_batch(B, L, seed=B + L)
    ids, mask = ids.to(dev), mask.to(dev)
    R = torch.randn(B, L, d_model, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    ref = m_ref(input_ids=ids, attention_mask=mask).last_hidden_state
    (ref * R).sum().backward()
    hid = train_hidden_t5(m_hip, ids, mask)
    assert hid.dtype == torch.float32 and hid.shape == ref.shape and hid.requires_grad
    (hid * R).sum().backward()
    _, cos_h = _err(hid.detach(), ref.detach())
    tag = f"t5 {d_model}/{layers}/{heads}/{d_ff}/{act} B={B} L={L}"
    print(f"{tag}: hidden cos {cos_h:.6f}")
    assert cos_h > 0.9999, cos_h

    def autocast_grads():
        m_ac = copy.deepcopy(m_ref)
        m_ac.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = m_ac(input_ids=ids, attention_mask=mask).last_hidden_state
        (h.float() * R).sum().backward()
        return {n: p.grad for n, p in m_ac.named_parameters()}

    _compare_grads(tag, m_hip, m_ref, autocast_grads)


@pytest.mark.parametrize("B,L", [(3, 50), (2, 156), (2, 200)])
@pytest.mark.parametrize("d_model,layers,heads,d_ff,act", CONFIGS[:2])
def test_tower_with_dropout_vs_masked_fp32_reference(dev, d_model, layers, heads, d_ff, act, B, L):
    """Train mode with dropout_rate 0.1 against the functional fp32 T5 encoder under autograd that
    applies the SAME hash masks at HF's six sites: hidden state and every parameter gradient; the
    same seed twice gives identical hidden states."""
    import torch
    from denseretrievaltoolkits_amd.model.t5_train_tower import train_hidden_t5
    m_ref = tr.t5_model(tr.t5_config(d_model, layers, heads, d_ff, act), seed=4).to(dev).train()
    m_ref.config.dropout_rate = 0.1
    m_hip = copy.deepcopy(m_ref)
    ids, mask = tr.t5_batch(B, L, seed=2 * B + L)
    ids, mask = ids.to(dev), mask.to(dev)
    seed = 24680
    R = torch.randn(B, L, d_model, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
    ref = ttr.t5_forward_with_masks(m_ref, ids, mask, 0.1, seed)
    (ref * R).sum().backward()
    hid = train_hidden_t5(m_hip, ids, mask, seed=seed)
    (hid * R).sum().backward()
    with torch.no_grad():
        again = train_hidden_t5(m_hip, ids, mask, seed=seed)
        other = train_hidden_t5(m_hip, ids, mask, seed=seed + 1)
    assert torch.equal(hid.detach(), again) and not torch.equal(hid.detach(), other)
    assert float((hid.detach() == 0).float().mean()) > 0.05          # the final dropout zeroes ~10 %
    _, cos_h = _err(hid.detach(), ref.detach())
    tag = f"t5 dropout {d_model}/{layers}/{heads}/{d_ff}/{act} B={B} L={L}"
    print(f"{tag}: hidden cos {cos_h:.6f}")
    assert cos_h > 0.9999, cos_h

    def autocast_grads():
        m_ac = copy.deepcopy(m_ref)
        m_ac.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = ttr.t5_forward_with_masks(m_ac, ids, mask, 0.1, seed)
        (h.float() * R).sum().backward()
        return {n: p.grad for n, p in m_ac.named_parameters()}

    _compare_grads(tag, m_hip, m_ref, autocast_grads)


def test_tower_rejects_unsupported(dev):
    import torch
    from denseretrievaltoolkits_amd.model.t5_train_tower import train_hidden_t5
    m = tr.t5_model(tr.t5_config(256, 1, 4, 512, "relu")).to(dev)
    with pytest.raises(NotImplementedError, match="513"):
        train_hidden_t5(m, torch.ones((1, 513), dtype=torch.int64, device=dev), None)
    m = tr.t5_model(tr.t5_config(256, 1, 4, 512, "relu", d_kv=32)).to(dev)
    with pytest.raises(NotImplementedError, match="d_kv 32"):
        train_hidden_t5(m, torch.ones((1, 8), dtype=torch.int64, device=dev), None)


# ---------------------------------------------------------------------------------------------
# DRModel level
# ---------------------------------------------------------------------------------------------
def _drmodel(dev, tied, flag, cfg=None):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    # gated-gelu: a ReLU tower's bf16 forward flips the sign of ~0.2 % of the FFN pre-activations next to
    # fp32 (|pre| below the bf16 rounding of its inputs), which alone moves wi.weight's gradient by
    # ~5 % (cos 0.998, the figure of test_tower_grads_vs_hf_autograd's relu cases) and would hide a
    # wiring error behind the 0.999 bound; this test is about the wiring (pooling, head, tied towers, the
    # bias table summed over two blocks), the relu arithmetic is bounded above
    cfg = cfg or tr.t5_config(512, 2, 6, 1024, "gated-gelu")
    lm_q = tr.t5_model(cfg, seed=5).to(dev)
    lm_p = lm_q if tied else tr.t5_model(cfg, seed=7).to(dev)
    torch.manual_seed(11)
    head_q = LinearHead(cfg.d_model, 64).to(dev)
    head_p = head_q if tied else copy.deepcopy(head_q)
    args = SimpleNamespace(encoder_only=True, hip_train_t5=True) if flag else SimpleNamespace(encoder_only=True)
    return DRModel(lm_q, lm_p, tied=tied, pooling="mean", head_q=head_q, head_p=head_p, normalize=True,
                   model_args=args, data_args=SimpleNamespace(train_n_passages=2),
                   train_args=SimpleNamespace(negatives_x_device=False)).eval()


@pytest.mark.parametrize("tied", [True, False])
def test_drmodel_trains_t5_towers_on_the_hip_path(dev, caplog, tied):
    """hip_train_t5 = True, mean pooling + normalize + head: reps carry a graph, no fallback is logged,
    loss.backward() fills every tower parameter's .grad, and under the SAME upstream gradient on the
    reps every gradient agrees with the HF path's at cosine >= 0.999."""
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    qi, qm = tr.t5_batch(2, 24, seed=1)
    pi, pm = tr.t5_batch(4, 70, seed=2)
    q_in = {"input_ids": qi.to(dev), "attention_mask": qm.to(dev)}
    p_in = {"input_ids": pi.to(dev), "attention_mask": pm.to(dev)}
    gen = torch.Generator(device=dev).manual_seed(3)
    grads, reps, g_q, g_p = {}, {}, None, None
    for hip in (True, False):
        m = _drmodel(dev, tied, hip)
        biencoder._FALLBACK_LOGGED.clear()
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger=biencoder.logger.name):
            out = m(query=q_in, passage=p_in)
        logged = any("HF module under torch" in r.getMessage() for r in caplog.records)
        assert logged == (not hip)
        assert out.q_reps.requires_grad and out.p_reps.requires_grad and out.loss.requires_grad
        if hip:
            assert not m._hip_cache
            out.loss.backward()      # the training loss reaches every tower parameter
            for lm in {id(m.lm_q): m.lm_q, id(m.lm_p): m.lm_p}.values():
                for n, p in lm.named_parameters():
                    assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n
            m.zero_grad(set_to_none=True)
            out = m(query=q_in, passage=p_in)
            g_q = torch.randn(out.q_reps.shape, device=dev, generator=gen)
            g_p = torch.randn(out.p_reps.shape, device=dev, generator=gen)
        ((out.q_reps * g_q).sum() + (out.p_reps * g_p).sum()).backward()
        reps[hip] = (out.q_reps.detach().double(), out.p_reps.detach().double())
        grads[hip] = {f"{side}.{n}": p.grad.detach().clone()
                      for side, lm in (("q", m.lm_q), ("p", m.lm_p)) for n, p in lm.named_parameters()}
    for a, b in zip(reps[True], reps[False]):
        cos = torch.nn.functional.cosine_similarity(a, b, dim=1)
        assert float(cos.min()) >= 0.9999, float(cos.min())
    assert set(grads[True]) == set(grads[False])
    cosines = sorted((_err(grads[True][n], g)[1], n) for n, g in grads[False].items())
    print("lowest gradient cosines:", cosines[:4])
    assert cosines[0][0] >= 0.999, cosines[:4]


def test_drmodel_default_flag_keeps_hf_module(dev, caplog):
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    m = _drmodel(dev, True, False)
    ids, mask = tr.t5_batch(2, 16, seed=1)
    biencoder._FALLBACK_LOGGED.clear()
    with caplog.at_level(logging.WARNING, logger=biencoder.logger.name):
        _, reps = m.encode_passage({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)})
    assert reps.requires_grad and m.hip_train_t5 is False
    assert any("HF module under torch" in r.getMessage() for r in caplog.records)
    assert not m._hip_cache


def test_drmodel_unsupported_config_logs_reason_and_runs_hf(dev, caplog):
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    m = _drmodel(dev, True, True, cfg=tr.t5_config(256, 1, 4, 512, "relu", d_kv=32))
    ids, mask = tr.t5_batch(2, 16, seed=1)
    biencoder._FALLBACK_LOGGED.clear()
    with caplog.at_level(logging.WARNING, logger=biencoder.logger.name):
        hidden, reps = m.encode_passage({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)})
    assert reps.requires_grad and hidden.dtype == torch.float32
    assert any("d_kv 32" in r.getMessage() for r in caplog.records)
    with torch.no_grad():
        want = m.lm_p(input_ids=ids.to(dev), attention_mask=mask.to(dev)).last_hidden_state
    torch.testing.assert_close(hidden.detach(), want, atol=1e-5, rtol=1e-5)

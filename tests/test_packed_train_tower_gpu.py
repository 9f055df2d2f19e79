"""The padding-free training tower (model/train_tower.py with a PackingPlan) end to end: hidden
states and every parameter gradient against HF BertModel under torch fp32 autograd, with the
criteria of tests/test_train_tower_gpu.py; with dropout against a functional fp32 BERT that applies
the same hash masks at the PACKED positions; DRModel / RRModel with ``hip_packed_train`` set against
the same model with the flag off; the cases that must keep the padded tower; the tail-row invariant.
Every packed case asserts that the varlen attention backward ran for every layer."""
import logging

import numpy as np
import pytest

import test_train_tower_gpu as tt
from oracle import bert_weights as bw

pytestmark = pytest.mark.gpu

VARLEN_BWD = "drt_attention_varlen_backward_bf16"
VARLEN_FWD = "drt_attention_varlen_train_forward_bf16"


class _Spy:
    """Counts the calls of one native entry (the ctypes handle is shared)."""

    def __init__(self, monkeypatch, name=VARLEN_BWD):
        from denseretrievaltoolkits_amd import _native
        lib = _native.load()
        self.calls = 0
        real = getattr(lib, name)

        def counted(*args):
            self.calls += 1
            return real(*args)

        monkeypatch.setattr(lib, name, counted)


def _batch(B, L, dev, not_multiple_of_32=False):
    """(ids, mask) of bw.token_batch on the device and its forced plan; with not_multiple_of_32 the
    first seed (counting up) whose token count is no multiple of 32."""
    import torch
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    seed = L + B
    while True:
        ids, mask = bw.token_batch(B, L, seed=seed)
        if not not_multiple_of_32 or int(mask.sum()) % 32:
            break
        seed += 1
    ids_t, mask_t = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    plan = plan_packing(mask_t, L, force=True)
    assert plan is not None and plan.T == int(mask.sum())
    return ids_t, mask_t, plan


def _compare_grads(m_ref, m_hip):
    """The criteria of test_train_tower_gpu._grads_vs_hf: cos > 0.995 and rel < 0.1 per parameter, the
    key.bias rule."""
    import torch
    worst, bad = [], []
    for (n, p_ref), (n2, p_hip) in zip(m_ref.named_parameters(), m_hip.named_parameters()):
        assert n == n2
        if p_ref.grad is None:
            assert p_hip.grad is None or float(p_hip.grad.abs().max()) == 0.0, n
            continue
        assert p_hip.grad is not None, n
        a, b = p_hip.grad.flatten().double(), p_ref.grad.flatten().double()
        nb = float(b.norm())
        if nb == 0.0:
            continue
        rel = float((a - b).norm()) / nb
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        if n.endswith("attention.self.key.bias"):
            vb = dict(m_ref.named_parameters())[n.replace("key.bias", "value.bias")].grad.double().norm()
            if float(a.norm()) > 0.05 * float(vb):
                bad.append((n, float(a.norm()), float(vb)))
            continue
        worst.append((rel, cos, n))
        if not (cos > 0.995 and rel < 0.1):
            bad.append((n, cos, rel))
    worst.sort(reverse=True)
    print("worst relative gradient errors:", worst[:4])
    assert not bad, bad


def _check_hidden(hid, ref, mask_t):
    import torch
    real = mask_t.bool()
    cos_h = torch.nn.functional.cosine_similarity(hid[real].flatten(), ref.detach()[real].flatten(), dim=0).item()
    assert cos_h > 0.9999, cos_h
    assert (hid[~real] == 0).all(), "pad positions of the packed tower's hidden state are not exactly zero"


SHAPES = [(2, 4, 64, False), (1, 8, 128, False), (2, 6, 32, False), (1, 4, 156, False), (1, 6, 64, True)]


@pytest.mark.parametrize("layers,B,L,types", SHAPES, ids=[f"{ly}-{B}-{L}" + ("-types" if t else "") for ly, B, L, t in SHAPES])
def test_packed_tower_grads_vs_hf_autograd(dev, monkeypatch, layers, B, L, types):
    """Dropout 0; the loss (hidden R mask).sum() is the same function of the parameters on both sides.
    (1, 8, 128) is searched for a token count that is no multiple of 32."""
    import torch
    from denseretrievaltoolkits_amd.model.train_tower import train_hidden
    m_ref = tt._bert(layers, 11, dev).train()
    m_hip = tt._bert(layers, 11, dev).train()
    ids_t, mask_t, plan = _batch(B, L, dev, not_multiple_of_32=(B, L) == (8, 128))
    if (B, L) == (8, 128):
        assert plan.T % 32 != 0
    tok = None
    if types:
        rng = np.random.default_rng(L)
        cut = rng.integers(1, L, size=(B, 1))
        tok = torch.from_numpy((np.arange(L)[None, :] >= cut).astype(np.int64)).to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    R = torch.randn(B, L, 768, generator=g, device=dev) * mask_t[:, :, None].float()
    ref = m_ref(input_ids=ids_t, attention_mask=mask_t, token_type_ids=tok).last_hidden_state
    (ref * R).sum().backward()
    fwd, bwd = _Spy(monkeypatch, VARLEN_FWD), _Spy(monkeypatch, VARLEN_BWD)
    hid = train_hidden(m_hip, ids_t, mask_t, token_type_ids=tok, plan=plan)
    (hid * R).sum().backward()
    assert fwd.calls == layers and bwd.calls == layers, (fwd.calls, bwd.calls)
    print(f"packed tower layers={layers} B={B} L={L} T={plan.T}/{B * L}")
    _check_hidden(hid, ref, mask_t)
    _compare_grads(m_ref, m_hip)


def _ref_forward_with_packed_masks(m, ids, mask, ph, pa, seed, cu):
    """test_train_tower_gpu._ref_forward_with_masks with the hidden-site index of element (b, l, j) taken
    from its packed position, (cu[b] + l) H + j (pad positions: index 0, never read by the loss or by a
    real token); the attention keeps use the padded length L, as the kernels do."""
    import torch
    import torch.nn.functional as F
    from denseretrievaltoolkits_amd.model.train_tower import dropout_sites
    cfg = m.config
    B, L = ids.shape
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    dh = H // nh
    eps = cfg.layer_norm_eps
    dev = ids.device
    row = cu[:B].to(torch.int64)[:, None] + torch.arange(L, device=dev)[None, :]
    flat = row[:, :, None] * H + torch.arange(H, device=dev)[None, None, :]
    flat = torch.where(mask.bool()[:, :, None], flat, torch.zeros_like(flat))

    def drop(x, site, p):
        return torch.where(tt._keep_torch(seed, site, flat, p), x / (1 - p), torch.zeros_like(x)) if p > 0 else x

    def drop_probs(x, site, p):
        keep = tt._attn_keep_torch(seed, site, B, nh, L, p, dev)
        return torch.where(keep, x / (1 - p), torch.zeros_like(x)) if p > 0 else x

    e = m.embeddings
    x = e.word_embeddings(ids) + e.token_type_embeddings(torch.zeros_like(ids)) + \
        e.position_embeddings(torch.arange(L, device=dev))[None]
    x = drop(F.layer_norm(x, (H,), e.LayerNorm.weight, e.LayerNorm.bias, eps), 0, ph)
    bias = (1 - mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    for i, layer in enumerate(m.encoder.layer):
        s_att, s1, s2 = dropout_sites(i)
        sa = layer.attention.self
        q = sa.query(x).view(B, L, nh, dh).transpose(1, 2)
        k = sa.key(x).view(B, L, nh, dh).transpose(1, 2)
        v = sa.value(x).view(B, L, nh, dh).transpose(1, 2)
        probs = torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5 + bias, -1)
        ctx = (drop_probs(probs, s_att, pa) @ v).transpose(1, 2).reshape(B, L, H)
        ao = layer.attention.output
        x1 = F.layer_norm(drop(ao.dense(ctx), s1, ph) + x, (H,), ao.LayerNorm.weight, ao.LayerNorm.bias, eps)
        f = F.gelu(layer.intermediate.dense(x1))
        o = layer.output
        x = F.layer_norm(drop(o.dense(f), s2, ph) + x1, (H,), o.LayerNorm.weight, o.LayerNorm.bias, eps)
    return x


@pytest.mark.parametrize("classes", [False, True], ids=["one-launch", "per-class"])
@pytest.mark.parametrize("layers,B,L", [(2, 4, 64), (1, 6, 128), (1, 3, 156)])
def test_packed_tower_with_dropout_vs_masked_fp32_reference(dev, monkeypatch, layers, B, L, classes):
    """Train-mode packed tower with dropout 0.1 / 0.1 against a functional fp32 BERT under autograd that
    applies the same hash masks (hidden sites at the packed element index, attention keeps of the padded
    batch), in both launch policies."""
    import torch
    from denseretrievaltoolkits_amd.model import train_tower
    m_ref = tt._bert(layers, 13, dev).train()
    m_hip = tt._bert(layers, 13, dev).train()
    for m in (m_ref, m_hip):
        m.config.hidden_dropout_prob = 0.1
        m.config.attention_probs_dropout_prob = 0.1
    ids_t, mask_t, plan = _batch(B, L, dev)
    seed = 24680
    R = torch.randn(B, L, 768, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
    R = R * mask_t[:, :, None].float()
    ref = _ref_forward_with_packed_masks(m_ref, ids_t, mask_t, 0.1, 0.1, seed, plan.cu_seqlens)
    (ref * R).sum().backward()
    monkeypatch.setattr(train_tower, "packed_train_classes", classes)
    bwd = _Spy(monkeypatch)
    hid = train_tower.train_hidden(m_hip, ids_t, mask_t, seed=seed, plan=plan)
    (hid * R).sum().backward()
    assert bwd.calls == layers * (len(plan.classes()) if classes else 1)
    _check_hidden(hid, ref, mask_t)
    _compare_grads(m_ref, m_hip)


def _items(ids_t, mask_t):
    return {"input_ids": ids_t, "attention_mask": mask_t}


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _close_to_flag_off(loss_on, loss_off, g_on, g_off):
    import torch
    assert abs(float(loss_on) - float(loss_off)) <= 1e-2 * abs(float(loss_off)) + 1e-3, (float(loss_on), float(loss_off))
    assert g_on.keys() == g_off.keys()
    bad = []
    vb = {n: g for n, g in g_off.items() if n.endswith("value.bias")}
    for n in g_off:
        a, b = g_on[n].flatten().double(), g_off[n].flatten().double()
        if float(b.norm()) == 0.0:
            continue
        if n.endswith("attention.self.key.bias"):
            if float(a.norm()) > 0.05 * float(vb[n.replace("key.bias", "value.bias")].double().norm()):
                bad.append((n, float(a.norm())))
            continue
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        rel = float((a - b).norm() / b.norm())
        if not (cos > 0.995 and rel < 0.1):
            bad.append((n, cos, rel))
    assert not bad, bad


@pytest.mark.parametrize("pooling", ["first", "mean", "max"])
def test_drmodel_with_hip_packed_train(dev, monkeypatch, pooling):
    """DRModel.encode under autograd with the flag: the varlen backward runs once per layer, and the loss
    and every gradient are within the tower criteria of the same model with the flag off."""
    import torch
    from denseretrievaltoolkits_amd.model import packing
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    layers, B, L = 2, 6, 64
    ids_t, mask_t, plan = _batch(B, L, dev)
    assert 1.0 - plan.T / (B * L) > packing.hip_packed_train_min_saving    # packs without force
    R = torch.randn(B, 768, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    out = {}
    spy = _Spy(monkeypatch)
    for flag in (False, True):
        lm = tt._bert(layers, 17, dev).train()
        dr = DRModel(lm, lm, pooling=pooling)
        dr.hip_packed_train = flag
        before = spy.calls
        hidden, reps = dr.encode(_items(ids_t, mask_t), lm, None)
        loss = (reps * R).sum()
        loss.backward()
        assert spy.calls - before == (layers if flag else 0)
        out[flag] = (loss.detach(), _grads(lm), hidden.detach())
    _close_to_flag_off(out[True][0], out[False][0], out[True][1], out[False][1])
    assert (out[True][2][~mask_t.bool()] == 0).all()


def test_rrmodel_with_hip_packed_train(dev, monkeypatch):
    import torch
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model import packing
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    layers, B, L = 2, 5, 96
    ids_t, mask_t, plan = _batch(B, L, dev)
    assert 1.0 - plan.T / (B * L) > packing.hip_packed_train_min_saving
    tok = (torch.arange(L, device=dev)[None, :] >= (mask_t.sum(1, keepdim=True) // 2)).to(torch.int64)
    items = dict(_items(ids_t, mask_t), token_type_ids=tok)
    r = torch.randn(B, 1, generator=torch.Generator(device=dev).manual_seed(4), device=dev)
    out = {}
    spy = _Spy(monkeypatch)
    for flag in (False, True):
        lm = tt._bert(layers, 19, dev).train()
        torch.manual_seed(1)
        rr = RRModel(lm, LinearHead(768, 1).to(dev))
        rr.hip_packed_train = flag
        before = spy.calls
        loss = (rr.encode(items) * r).sum()
        loss.backward()
        assert spy.calls - before == (layers if flag else 0)
        out[flag] = (loss.detach(), _grads(rr))
    _close_to_flag_off(out[True][0], out[False][0], out[True][1], out[False][1])


@pytest.mark.parametrize("kind", ["hole", "long"])
def test_flag_keeps_the_padded_tower_and_logs_why(dev, monkeypatch, caplog, kind):
    """A mask with a hole, and a batch whose longest sequence is over 160 tokens: the padded tower runs
    (no varlen call, the bits of the flag-off result) and the reason is logged."""
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    B, L = (4, 64) if kind == "hole" else (3, 192)
    ids, mask = bw.token_batch(B, L, seed=8)
    if kind == "hole":
        mask[1, 2] = 0
    else:
        mask[0, :] = 0
        mask[0, :170] = 1
        mask[1:, 40:] = 0
    ids_t, mask_t = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    spy_f, spy_b = _Spy(monkeypatch, VARLEN_FWD), _Spy(monkeypatch, VARLEN_BWD)
    res = {}
    for flag in (False, True):
        lm = tt._bert(1, 23, dev).train()
        dr = DRModel(lm, lm)
        dr.hip_packed_train = flag
        biencoder._FALLBACK_LOGGED.clear()
        with caplog.at_level(logging.WARNING):
            hidden, reps = dr.encode(_items(ids_t, mask_t), lm, None)
        reps.sum().backward()
        res[flag] = (hidden.detach(), _grads(lm))
    assert spy_f.calls == 0 and spy_b.calls == 0
    assert torch.equal(res[True][0], res[False][0])
    for n, g in res[False][1].items():             # the same kernels; fp32 atomics may reorder a sum
        torch.testing.assert_close(res[True][1][n], g, rtol=1e-4, atol=1e-6, msg=n)
    text = " ".join(r.getMessage() for r in caplog.records)
    assert "hip_packed_train" in text
    assert ("prefixes" in text) if kind == "hole" else ("> 160" in text)


def test_hip_packed_alone_does_not_change_training(dev, monkeypatch):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    ids_t, mask_t, _ = _batch(4, 64, dev)
    spy_f, spy_b = _Spy(monkeypatch, VARLEN_FWD), _Spy(monkeypatch, VARLEN_BWD)
    res = {}
    for flag in (False, True):
        lm = tt._bert(1, 29, dev).train()
        dr = DRModel(lm, lm)
        dr.hip_packed = flag
        assert dr.hip_packed_train is False
        hidden, reps = dr.encode(_items(ids_t, mask_t), lm, None)
        reps.sum().backward()
        res[flag] = (hidden.detach(), _grads(lm))
    assert spy_f.calls == 0 and spy_b.calls == 0
    assert torch.equal(res[True][0], res[False][0])
    for n, g in res[False][1].items():             # the same kernels; fp32 atomics may reorder a sum
        torch.testing.assert_close(res[True][1][n], g, rtol=1e-4, atol=1e-6, msg=n)


def test_tail_rows_handed_to_wgrad_are_exact_zeros(dev, monkeypatch):
    """The invariant of model/train_tower.py: with T32 = ceil(T / 32) 32 rows, the T32 - T tail rows of
    every gradient that enters a wgrad are exactly zero and the tail rows of its activation operand are
    finite, with and without dropout."""
    import torch
    from denseretrievaltoolkits_amd.model import encoder_bwd, train_tower
    layers, B, L = 2, 8, 128
    ids_t, mask_t, plan = _batch(B, L, dev, not_multiple_of_32=True)
    T, T32 = plan.T, (plan.T + 31) // 32 * 32
    assert T % 32 != 0
    seen = []
    real = encoder_bwd.wgrad

    def spying(dy, x):
        seen.append((dy, x))
        return real(dy, x)

    monkeypatch.setattr(encoder_bwd, "wgrad", spying)
    for p in (0.0, 0.1):
        m = tt._bert(layers, 31, dev).train()
        m.config.hidden_dropout_prob = p
        m.config.attention_probs_dropout_prob = p
        seen.clear()
        hid = train_tower.train_hidden(m, ids_t, mask_t, seed=77, plan=plan)
        hid.square().sum().backward()
        assert len(seen) == 4 * layers
        for dy, x in seen:
            assert dy.shape[0] == T32 and x.shape[0] == T32
            assert ((dy[T:].view(torch.int16) & 0x7FFF) == 0).all(), "a tail row of a gradient is not zero"
            assert torch.isfinite(x[T:].float()).all() and torch.isfinite(dy.float()).all()

"""The padding-free inference path end to end: HipBertEncoder.forward_packed against HF BertModel
in fp32 (COS_MIN of tests/test_encoder_gpu.py), DRModel / RRModel with ``hip_packed`` set, and the
cases that must keep the padded path.  Every packed case asserts that the packed path really ran:
a plan exists and the varlen attention entry was called for every layer."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import t5_refs as tr
from oracle import bert_weights as bw

pytestmark = pytest.mark.gpu

COS_MIN = 0.999
VARLEN = "drt_attention_varlen_forward_bf16"


def _bert(layers, seed=0):
    from transformers import BertModel
    m = BertModel(bw.bert_config(layers=layers), add_pooling_layer=False).eval()
    return bw.init_model_(m, seed)


class _Spy:
    """Counts the calls of one native entry (the ctypes handle is shared by every encoder)."""

    def __init__(self, monkeypatch, name=VARLEN):
        from denseretrievaltoolkits_amd import _native
        lib = _native.load()
        self.calls = 0
        real = getattr(lib, name)

        def counted(*args):
            self.calls += 1
            return real(*args)

        monkeypatch.setattr(lib, name, counted)


def _cos_rows(a, b):
    a = a.reshape(-1, a.shape[-1]).astype(np.float64)
    b = b.reshape(-1, b.shape[-1]).astype(np.float64)
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) + 1e-30)


@pytest.mark.parametrize("presum", ["bf16", "fp32"])
@pytest.mark.parametrize("layers,B,L", [(2, 8, 128), (12, 4, 128), (2, 5, 32), (2, 3, 160), (1, 2, 512)])
def test_forward_packed_vs_hf_fp32(dev, monkeypatch, layers, B, L, presum):
    import torch
    from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    m = _bert(layers)
    ids, mask = bw.token_batch(B, L, seed=L + B)
    with torch.no_grad():
        ref = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state.numpy()
    enc = HipBertEncoder.from_hf(m, dev, presum=presum)
    ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    plan = plan_packing(mask_d, L)
    assert plan is not None and plan.T == int(mask.sum()) and plan.T < B * L
    spy = _Spy(monkeypatch)
    enc.packed_classes = False
    out = enc.forward_packed(ids_d, plan)
    assert spy.calls == layers                               # one launch per layer
    assert out.shape == (plan.T, enc.shape.hidden) and out.dtype == torch.bfloat16
    enc.packed_classes = True                                # one launch per layer and length class
    by_class = enc.forward_packed(ids_d, plan)
    assert spy.calls == layers + layers * len(plan.classes())
    padded = enc(ids_d, mask_d)
    assert spy.calls == layers + layers * len(plan.classes())   # the padded path does not use it
    valid = mask.astype(bool)
    padded = padded.float().cpu().numpy()[valid]
    for tag, got in (("one launch", out), ("length classes", by_class)):
        got = got.float().cpu().numpy()
        assert np.isfinite(got).all()
        cos = _cos_rows(got, ref[valid])
        print(f"packed ({tag}) layers={layers} B={B} L={L} presum={presum} T={plan.T}/{B * L}: "
              f"min cos {cos.min():.6f}, max abs err {np.abs(got - ref[valid]).max():.4f}, "
              f"max abs diff from the padded HIP path {np.abs(got - padded).max():.4f}")
        assert cos.min() >= COS_MIN


def test_forward_packed_two_stream_halves(dev, monkeypatch):
    """The two-stream form (two packed sub-batches split on a sequence boundary) holds the same
    bound, and unpack / pool_packed of its output agree with the one-pass form's layout."""
    import torch
    from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    m = _bert(2, seed=6)
    B, L = 41, 64
    ids, mask = bw.token_batch(B, L, seed=62)
    with torch.no_grad():
        ref = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state.numpy()
    enc = HipBertEncoder.from_hf(m, dev)
    ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    plan = plan_packing(mask_d, L)
    assert plan is not None
    spy = _Spy(monkeypatch)
    enc.packed_split_streams, enc.split_min_tokens = True, 64
    two = enc.forward_packed(ids_d, plan)
    torch.cuda.synchronize()
    launches = sum(len(sub.classes()) if enc.packed_classes else 1 for _, sub in plan.halves())
    assert spy.calls == 2 * launches and launches >= 2
    valid = mask.astype(bool)
    cos = _cos_rows(two.float().cpu().numpy(), ref[valid])
    assert cos.min() >= COS_MIN
    back = enc.unpack(two, plan, L)
    assert torch.equal(back[mask_d.bool()], two) and (back[~mask_d.bool()] == 0).all()


# ---------------------------------------------------------------------------------------------
# DRModel / RRModel
# ---------------------------------------------------------------------------------------------
_DR = {}


def _dr_fixture(dev):
    """One 2-layer tower, its query / passage batches and the HF fp32 hidden states, shared."""
    import torch
    if not _DR:
        lm = _bert(2, seed=3)
        batches = {}
        for name, (B, L, seed) in {"q": (6, 32, 5), "p": (5, 128, 9)}.items():
            ids, mask = bw.token_batch(B, L, seed=seed)
            ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
            with torch.no_grad():
                hid = lm(input_ids=ids, attention_mask=mask).last_hidden_state
            batches[name] = (ids, mask, hid)
        torch.manual_seed(11)
        from denseretrievaltoolkits_amd.model.linear import LinearHead
        _DR.update(lm=copy.deepcopy(lm).to(dev), batches=batches, head=LinearHead(768, 128).to(dev))
    return _DR


def _want_reps(hid, mask, pooling, normalize, head):
    import torch
    mk = mask.unsqueeze(-1).float()
    if pooling == "first":
        reps = hid[:, 0]
    elif pooling == "mean":
        reps = (hid * mk).sum(1) / mk.sum(1).clamp(min=1e-9)
    else:
        reps = (hid * mk).max(1)[0]
    if head is not None:
        reps = reps @ head.linear.weight.detach().cpu().float().T
    if normalize:
        reps = torch.nn.functional.normalize(reps, dim=1)
    return reps


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("pooling", ["first", "mean", "max"])
def test_drmodel_hip_packed_reps_vs_hf_fp32(dev, monkeypatch, pooling, normalize, head):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    fx = _dr_fixture(dev)
    hd = fx["head"] if head else None
    model = DRModel(fx["lm"], fx["lm"], pooling=pooling, normalize=normalize, head_q=hd, head_p=hd,
                    model_args=SimpleNamespace(hip_packed=True)).eval()
    assert model.hip_packed is True
    spy = _Spy(monkeypatch)
    for name in ("q", "p"):
        ids, mask, hid = fx["batches"][name]
        before = spy.calls
        with torch.no_grad():
            hidden, reps = model.encode({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}, fx["lm"], hd)
        assert spy.calls - before >= 2, "the packed path did not run"
        want = _want_reps(hid, mask, pooling, normalize, hd)
        cos = torch.nn.functional.cosine_similarity(reps.double().cpu(), want.double(), dim=1)
        print(f"DRModel hip_packed {name} {pooling} normalize={normalize} head={head}: min cos {float(cos.min()):.6f}")
        assert cos.min() >= COS_MIN
        # hidden: [B, L, H] with the real tokens in place and zeros at the pads
        assert hidden.shape == hid.shape and hidden.dtype == torch.bfloat16
        hidden = hidden.float().cpu()
        assert (hidden[~mask.bool()] == 0).all()
        tok = torch.nn.functional.cosine_similarity(hidden[mask.bool()].double(), hid[mask.bool()].double(), dim=1)
        assert tok.min() >= COS_MIN


def test_rrmodel_hip_packed_scores(dev, monkeypatch):
    """The packed scores' error against the HF fp32 tower is at most the padded HIP path's error on
    the same pairs plus 10 %; both errors are measured here."""
    import torch
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    lm = _bert(2, seed=8)
    torch.manual_seed(3)
    head = LinearHead(768, 1)
    B, L = 8, 160
    ids, mask = bw.token_batch(B, L, seed=31, min_len=40)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    tt = (torch.arange(L)[None, :] >= (mask.sum(1, keepdim=True) // 3)).to(torch.int64) * mask
    with torch.no_grad():
        hid = lm(input_ids=ids, attention_mask=mask, token_type_ids=tt).last_hidden_state
        want = head(hid[:, 0])
    model = RRModel(copy.deepcopy(lm).to(dev), copy.deepcopy(head).to(dev), pooling="first").eval()
    items = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": tt.to(dev)}
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        padded = model.encode(items)
        assert spy.calls == 0
        model.hip_packed = True
        packed = model.encode(items)
    assert spy.calls >= 2, "the packed path did not run"
    assert packed.shape == (B, 1) and packed.dtype == torch.float32
    e_padded = float((padded.cpu() - want).abs().max())
    e_packed = float((packed.cpu() - want).abs().max())
    print(f"RRModel scores: padded error {e_padded:.3e}, packed error {e_packed:.3e} (|score| <= {float(want.abs().max()):.3f})")
    assert e_packed <= 1.1 * e_padded


@pytest.mark.parametrize("case", ["holes", "full", "t5"])
def test_hip_packed_fallbacks_keep_the_padded_path(dev, monkeypatch, case):
    """With the flag set, a mask with holes, a batch without padding and a T5 tower take today's
    path: the varlen entry is never called and the result has the bits of the flag-off result."""
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    if case == "t5":
        lm = tr.t5_model(tr.t5_config(256, 2, 4, 512, "relu"), seed=5).to(dev)
        ids, mask = tr.t5_batch(4, 40, seed=2)
        args = dict(encoder_only=True)
    else:
        lm = _dr_fixture(dev)["lm"]
        ids, mask = bw.token_batch(4, 48, seed=17, fixed=(case == "full"))
        ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
        if case == "holes":
            mask[1, 2] = 0
        args = {}
    items = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}
    spy = _Spy(monkeypatch)
    outs = []
    for flag in (False, True):
        model = DRModel(lm, lm, pooling="mean", normalize=True, model_args=SimpleNamespace(hip_packed=flag, **args)).eval()
        assert model.hip_packed is flag
        with torch.no_grad():
            outs.append(model.encode(items, lm, None))
    assert spy.calls == 0
    (h0, r0), (h1, r1) = outs
    assert torch.equal(h0.view(torch.int16), h1.view(torch.int16)) and torch.equal(r0, r1)


def test_flag_off_never_packs(dev, monkeypatch):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    fx = _dr_fixture(dev)
    model = DRModel(fx["lm"], fx["lm"], pooling="first").eval()
    assert model.hip_packed is False
    spy = _Spy(monkeypatch)
    ids, mask, _ = fx["batches"]["p"]
    with torch.no_grad():
        model.encode({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}, fx["lm"], None)
    assert spy.calls == 0

"""MiniLM-class towers (hidden 384, 12 heads, head_dim 32) on the HIP inference path: the head_dim-32
attention (padded and varlen) and the H = 384 row kernels against the fp64 references of
tests/encoder_refs.py, and the tower end to end against HF fp32.

Masks, data kinds and the bound |ctx - ref| <= 2.5 u A + 1e-7 are those of
tests/test_encoder_fwd_fp64_gpu.py (nothing in its derivation depends on head_dim).  Its generator
makes 64-wide heads; called with heads / 2 it fills the same [rows, 3 H] layout, each 64-wide head read
as two 32-wide ones (the ramps then climb 11.4 and 4.9 log2 units per key tile: at every tile, and at
every other).  Outputs start as NaN, so an unwritten element fails the bound."""
import math
from types import SimpleNamespace

import pytest

import encoder_refs as er
import test_encoder_fwd_fp64_gpu as fw
import test_packed_encoder_gpu as pk
from oracle import bert_weights as bw

pytestmark = pytest.mark.gpu

B_ATT = 3
SHAPES = [(L, 12) for L in (1, 31, 32, 33, 64, 100, 128, 129, 160, 161, 257, 512)] + [(33, 2), (161, 2)]
LENS = (1, 31, 32, 33, 96, 160, 161, 300, 512)


def _scale():
    import torch
    return torch.tensor(1.0 / math.sqrt(32.0), dtype=torch.float32).item()   # the fp32 value, for both sides


def _nan(dev, rows, H):
    import torch
    return torch.full((rows, H), float("nan"), dtype=torch.bfloat16, device=dev)


@pytest.mark.parametrize("data", fw.DATA_KINDS)
@pytest.mark.parametrize("L,heads", SHAPES)
def test_attention_hd32_vs_fp64(dev, L, heads, data):
    from denseretrievaltoolkits_amd import _native
    lib, s, bad = _native.load(), _native.stream_ptr(dev), []
    for mk in fw.MASK_KINDS:
        g = fw._gen("hd32", L, heads, data, mk)
        mask = fw._mask(mk, B_ATT, L, g)
        qkv = fw._qkv(data, B_ATT, L, heads // 2, mask, g)
        ref, A, _ = er.attention_ref(qkv, mask, B_ATT, L, heads, _scale())
        qd, md, ctx = qkv.to(dev), None if mask is None else mask.to(dev), _nan(dev, B_ATT * L, heads * 32)
        _native.check(lib.drt_attention_hd32_forward_bf16(qd.data_ptr(), None if md is None else md.data_ptr(),
                                                          ctx.data_ptr(), B_ATT, L, heads, _scale(), s), "hd32")
        ratio = fw._ctx_ratio(ctx.cpu(), ref, A)
        print(f"hd32 attention L={L} heads={heads} {data} {mk}: ctx error {ratio:.3f} u A")
        if not ratio <= 2.5:
            bad.append(f"{mk}: {ratio:.3f} u A")
    assert not bad, f"L={L} heads={heads} {data}: " + "; ".join(bad)


@pytest.mark.parametrize("mode", ["one", "classes", "listed"])
def test_attention_hd32_varlen_vs_fp64(dev, mode):
    """One launch over the batch; the per-class launches of a PackingPlan; and a seq_ids list with a
    clamping max_len and an empty sequence: unlisted sequences and rows past the clamp keep their NaN."""
    import torch
    from denseretrievaltoolkits_amd import _native
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    lib, s, heads = _native.load(), _native.stream_ptr(dev), 12
    lens = list(LENS) if mode != "listed" else [0] + list(LENS)
    T = sum(lens)
    qkv = fw._qkv("gauss", 1, T, heads // 2, None, fw._gen("hd32 varlen"))
    cu = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to(dev)
    written = list(lens)                     # rows of each sequence the launches must write
    if mode == "one":
        launches = [(None, len(lens), max(lens))]
    elif mode == "classes":
        plan = plan_packing((torch.arange(512)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64).to(dev), 512)
        assert torch.equal(plan.cu_seqlens, cu) and len(plan.classes()) > 1
        cu, launches = plan.cu_seqlens, plan.launches(True)
    else:
        ids = torch.tensor([9, 0, 3, 6], dtype=torch.int32, device=dev)      # lengths 512, 0, 32, 160
        launches, written = [(ids.data_ptr(), 4, 100)], [min(n, 100) if b in (9, 3, 6) else 0 for b, n in enumerate(lens)]
    qd, ctx = qkv.to(dev), _nan(dev, T, heads * 32)
    for sp, n, ml in launches:
        _native.check(lib.drt_attention_hd32_varlen_forward_bf16(qd.data_ptr(), cu.data_ptr(), sp, n, ml,
                                                                 ctx.data_ptr(), heads, _scale(), s), "hd32 varlen")
    ctx, r0 = ctx.cpu(), 0
    for n, w in zip(lens, written):
        assert torch.isnan(ctx[r0 + w:r0 + n].float()).all(), f"{mode}: len {n}: rows past {w} written"
        if w:
            ref, A, _ = er.attention_ref(qkv[r0:r0 + w], None, 1, w, heads, _scale())
            ratio = fw._ctx_ratio(ctx[r0:r0 + w], ref, A)
            print(f"hd32 varlen {mode} len {n} ({w} keys): ctx error {ratio:.3f} u A")
            assert ratio <= 2.5, f"{mode}: len {n}"
        r0 += n


def test_row_kernels_h384_vs_fp64(dev):
    """embed_ln (padded, packed) and both LayerNorms at H = 384, 165 rows (4 per block: a tail of 1),
    within one bf16 rounding of fp64 (u |ref| + u |beta| + 1e-6); packed rows bit-equal to padded ones."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib, s, H, B, L, eps = _native.load(), _native.stream_ptr(dev), 384, 5, 33, 1e-12
    g = fw._gen("rows384")
    word, pos, typ = (0.02 * torch.randn(n, H, generator=g) for n in (fw.VOCAB, 512, 2))
    gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
    ids, tt = torch.randint(0, fw.VOCAB, (B, L), generator=g), torch.randint(0, 2, (B, L), generator=g)
    lens = [33, 1, 17, 32, 5]
    cu = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to(dev)
    T, Tp = B * L, sum(lens)
    d = [x.to(dev) for x in (ids, tt, word, pos, typ, gamma, beta)]
    tab = [x.data_ptr() for x in d[2:]]
    out, outp = _nan(dev, T + 4, H), _nan(dev, Tp + 4, H)
    _native.check(lib.drt_embed_ln(d[0].data_ptr(), d[1].data_ptr(), B, L, *tab, eps, H, out.data_ptr(), s), "embed_ln")
    _native.check(lib.drt_embed_ln_packed(d[0].data_ptr(), d[1].data_ptr(), cu.data_ptr(), B, L, Tp, *tab, eps, H,
                                          outp.data_ptr(), s), "embed_ln_packed")
    x = torch.randn(T, H, generator=g) * 3 + 0.5
    xb = x.to(torch.bfloat16)
    o32, o16 = _nan(dev, T + 4, H), _nan(dev, T + 4, H)
    _native.check(lib.drt_layernorm_f32_bf16(x.to(dev).data_ptr(), T, H, *tab[3:], eps, o32.data_ptr(), s), "ln f32")
    _native.check(lib.drt_layernorm_bf16(xb.to(dev).data_ptr(), T, H, *tab[3:], eps, o16.data_ptr(), s), "ln bf16")

    def ln64(v):
        v = v.double()
        mu = v.mean(1, keepdim=True)
        return (v - mu) / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + eps) * gamma.double() + beta.double()

    refs = {"embed_ln": (out, er.embed_ln_ref(ids, tt, L, word, pos, typ, gamma, beta, eps)),
            "ln f32": (o32, ln64(x)), "ln bf16": (o16, ln64(xb))}
    for tag, (got, ref) in refs.items():
        got = got.cpu()
        assert torch.isnan(got[T:].float()).all(), f"{tag}: rows past T written"
        err = (got[:T].double() - ref).abs()
        bound = fw.U * ref.abs() + fw.U * beta.double().abs()[None, :] + 1e-6
        print(f"{tag} H=384: worst err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), tag
    outp, rows = outp.cpu(), torch.cat([torch.arange(n) + b * L for b, n in enumerate(lens)])
    assert torch.isnan(outp[Tp:].float()).all()
    assert torch.equal(outp[:Tp].view(torch.int16), out.cpu()[rows].view(torch.int16))


def _minilm(seed):
    from transformers import BertModel
    cfg = bw.bert_config(layers=2, hidden=384, heads=12, intermediate=1536)
    return bw.init_model_(BertModel(cfg, add_pooling_layer=False).eval(), seed)


@pytest.mark.parametrize("B,L", [(4, 64), (3, 161)])
def test_minilm_tower_vs_hf_fp32(dev, B, L):
    import numpy as np
    import torch
    from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    m = _minilm(1)
    ids, mask = bw.token_batch(B, L, seed=L)
    with torch.no_grad():
        ref = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state.numpy()
    enc = HipBertEncoder.from_hf(m, dev)
    ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    plan = plan_packing(mask_d, L, force=True)
    valid = mask.astype(bool)
    for tag, got in (("padded", enc(ids_d, mask_d)[mask_d.bool()]), ("packed", enc.forward_packed(ids_d, plan))):
        cos = pk._cos_rows(got.float().cpu().numpy(), ref[valid])
        print(f"MiniLM tower {tag} B={B} L={L}: min cos {cos.min():.6f}")
        assert np.isfinite(cos).all() and cos.min() >= pk.COS_MIN


def test_minilm_models_encode_and_score(dev, monkeypatch):
    """DRModel.encode under no_grad with hip_packed off and on, and an RRModel pair batch at L = 160:
    the tolerances of tests/test_packed_encoder_gpu.py; the packed runs call the varlen entry."""
    import copy
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    lm = _minilm(2)
    spy = pk._Spy(monkeypatch, "drt_attention_hd32_varlen_forward_bf16")
    ids, mask = (torch.from_numpy(x) for x in bw.token_batch(5, 128, seed=9))
    with torch.no_grad():
        hid = lm(input_ids=ids, attention_mask=mask).last_hidden_state
    lm_d = copy.deepcopy(lm).to(dev)
    for flag in (False, True):
        model = DRModel(lm_d, lm_d, pooling="mean", normalize=True, model_args=SimpleNamespace(hip_packed=flag)).eval()
        with torch.no_grad():
            hidden, reps = model.encode({"input_ids": ids.to(dev), "attention_mask": mask.to(dev)}, lm_d, None)
        assert spy.calls == (2 if flag else 0)
        cos = torch.nn.functional.cosine_similarity(reps.double().cpu(), pk._want_reps(hid, mask, "mean", True, None).double())
        tok = torch.nn.functional.cosine_similarity(hidden.float().cpu()[mask.bool()].double(), hid[mask.bool()].double())
        assert cos.min() >= pk.COS_MIN and tok.min() >= pk.COS_MIN
        assert not flag or (hidden[~mask.bool().to(dev)] == 0).all()      # unpacked: zeros at the pads
    torch.manual_seed(3)
    head = LinearHead(384, 1)
    ids, mask = (torch.from_numpy(x) for x in bw.token_batch(8, 160, seed=31, min_len=40))
    tt = (torch.arange(160)[None, :] >= (mask.sum(1, keepdim=True) // 3)).to(torch.int64) * mask
    with torch.no_grad():
        want = head(lm(input_ids=ids, attention_mask=mask, token_type_ids=tt).last_hidden_state[:, 0])
    rr = RRModel(lm_d, copy.deepcopy(head).to(dev), pooling="first").eval()
    items = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": tt.to(dev)}
    with torch.no_grad():
        padded = rr.encode(items)
        rr.hip_packed = True
        packed = rr.encode(items)
    assert spy.calls == 4 and packed.shape == (8, 1)
    e_padded, e_packed = (float((x.cpu() - want).abs().max()) for x in (padded, packed))
    print(f"MiniLM RRModel: padded error {e_padded:.3e}, packed error {e_packed:.3e}, |score| <= {float(want.abs().max()):.3f}")
    assert e_packed <= 1.1 * e_padded

"""The fp64 references of tests/encoder_refs.py against HF BERT in .double() on the CPU
(2 layers, H = 256, 4 heads of 64, B = 3, L = 37): fp64 against fp64, tolerance 1e-10."""
import numpy as np
import pytest

import encoder_refs as er
from oracle import bert_weights as bw

B, L, H, HEADS, VOCAB = 3, 37, 256, 4, 1000
TOL = dict(atol=1e-10, rtol=1e-10)


@pytest.fixture(scope="module")
def hf():
    import torch
    from transformers import BertModel
    cfg = bw.bert_config(layers=2, hidden=H, heads=HEADS, intermediate=4 * H, vocab=VOCAB)
    try:
        cfg._attn_implementation = "eager"
    except Exception:   # versions without the switch have only the eager BertSelfAttention
        pass
    m = BertModel(cfg, add_pooling_layer=False).eval()
    bw.init_model_(m, 5)
    with torch.no_grad():   # random LayerNorm parameters, not near (1, 0)
        g = torch.Generator().manual_seed(1)
        m.embeddings.LayerNorm.weight.copy_(torch.randn(H, generator=g))
        m.embeddings.LayerNorm.bias.copy_(torch.randn(H, generator=g))
    return m.double()


def _holey_mask(g):
    import torch
    mask = (torch.rand(B, L, generator=g) < 0.6).to(torch.int64)
    mask[0, L - 1] = 1
    mask[1] = 0                 # one sequence with every key masked
    mask[2, :5] = 0
    mask[2, 5] = 1
    return mask


def test_attention_ref_vs_hf_self_attention(hf):
    """attention_ref on a packed bf16 QKV against BertSelfAttention (eager, fp64).  The module's
    query / key / value projections are set to column permutations (zero bias), so HF sees exactly
    the bf16 values of the packed tensor."""
    import torch
    att = hf.encoder.layer[1].attention.self
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, L, H, generator=g).to(torch.bfloat16)
    perms = [torch.arange(H), torch.randperm(H, generator=g), torch.randperm(H, generator=g)]
    with torch.no_grad():
        for lin, p in zip((att.query, att.key, att.value), perms):
            lin.weight.copy_(torch.eye(H, dtype=torch.float64)[p])
            lin.bias.zero_()
    qkv = torch.cat([x.reshape(B * L, H)[:, p] for p in perms], 1)
    mask = _holey_mask(g)
    ext = (1.0 - mask[:, None, None, :].double()) * torch.finfo(torch.float64).min
    with torch.no_grad():
        want = att(x.double(), attention_mask=ext)[0].reshape(B * L, H)
    ctx, A, lse = er.attention_ref(qkv, mask, B, L, HEADS, 1.0 / 8.0)
    torch.testing.assert_close(ctx, want, **TOL)
    # the all-masked sequence is the uniform mean of its V rows
    v = qkv[:, 2 * H:].double().reshape(B, L, H)
    torch.testing.assert_close(ctx.reshape(B, L, H)[1], v[1].mean(0, keepdim=True).expand(L, H), **TOL)
    assert torch.isfinite(lse).all() and torch.isfinite(A).all()
    # A and lse from their definitions
    q = x.double().reshape(B, L, HEADS, 64).transpose(1, 2) / 8.0
    k = qkv[:, H:2 * H].double().reshape(B, L, HEADS, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2) + ext
    live = [0, 2]
    torch.testing.assert_close(lse[live], torch.logsumexp(s, -1)[live], **TOL)
    pa = torch.softmax(s, -1) @ v.abs().reshape(B, L, HEADS, 64).transpose(1, 2)
    torch.testing.assert_close(A, pa.transpose(1, 2).reshape(B * L, H), **TOL)
    # no mask = all ones
    c0, _, l0 = er.attention_ref(qkv, None, B, L, HEADS, 1.0 / 8.0)
    c1, _, l1 = er.attention_ref(qkv, torch.ones(B, L, dtype=torch.int64), B, L, HEADS, 1.0 / 8.0)
    assert torch.equal(c0, c1) and torch.equal(l0, l1)
    with torch.no_grad():
        want0 = att(x.double(), attention_mask=None)[0].reshape(B * L, H)
    torch.testing.assert_close(c0, want0, **TOL)


@pytest.mark.parametrize("with_types", [False, True])
def test_embed_ln_ref_vs_hf_embeddings(hf, with_types):
    import torch
    emb = hf.embeddings
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, VOCAB, (B, L), generator=g)
    ids[0, 0], ids[0, 1] = 0, VOCAB - 1
    tt = torch.randint(0, 2, (B, L), generator=g) if with_types else None
    with torch.no_grad():
        want = emb(input_ids=ids, token_type_ids=tt).reshape(B * L, H)
    got = er.embed_ln_ref(ids, tt, L, emb.word_embeddings.weight, emb.position_embeddings.weight,
                          emb.token_type_embeddings.weight, emb.LayerNorm.weight, emb.LayerNorm.bias,
                          emb.LayerNorm.eps)
    assert got.dtype == torch.float64
    torch.testing.assert_close(got, want, **TOL)


def test_pool_and_l2_refs_vs_torch():
    import torch
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, L, H, generator=g, dtype=torch.float64)
    h[0] = -h[0].abs() - 0.1
    mask = _holey_mask(g)
    mk = mask.unsqueeze(-1).double()
    torch.testing.assert_close(er.pool_ref(h, mask, 0), h[:, 0, :], **TOL)
    torch.testing.assert_close(er.pool_ref(h, mask, 1), (h * mk).sum(1) / mk.sum(1).clamp(min=1e-9), **TOL)
    torch.testing.assert_close(er.pool_ref(h, mask, 2), (h * mk).max(1)[0], **TOL)
    assert (er.pool_ref(h, mask, 1)[1] == 0).all()            # every token masked: mean 0
    assert (er.pool_ref(h, mask, 2)[0] == 0).all()            # negative sequence with a masked token: max 0
    torch.testing.assert_close(er.pool_ref(h, None, 2)[0], h[0].max(0)[0], **TOL)
    torch.testing.assert_close(er.pool_ref(h, None, 1), h.mean(1), **TOL)
    x = torch.randn(5, 100, generator=g, dtype=torch.float64)
    x[3] = 0
    torch.testing.assert_close(er.l2_ref(x), torch.nn.functional.normalize(x, dim=1), **TOL)
    assert (er.l2_ref(x)[3] == 0).all()
    np.testing.assert_allclose(er.l2_ref(x).norm(dim=1).numpy()[[0, 1, 2, 4]], 1.0, rtol=1e-12)

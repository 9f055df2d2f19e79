"""CPU: the fp64 backward references of tests/encoder_bwd_refs.py against torch.autograd in float64 of
the plain formulas, and the bounds of tests/test_encoder_bwd_fp64_gpu.py on a torch emulation of the
kernels' roundings (tests/encoder_bwd_cases.py) over that test's own data and mask kinds: the bounds can
be met, so a kernel over one of them has a bug, not an unlucky rounding."""
import math

import pytest

import encoder_bwd_cases as bc
import encoder_bwd_refs as br


def _close(got, want, tag, A=None):
    """max |got - want| <= 1e-10 max |want| (both fp64); with A, relative to the sum of the absolute
    terms instead (a single live key has dS = dP - D = 0 in exact arithmetic)."""
    scale = max(float((want.abs() if A is None else A).max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= 1e-10 * scale, f"{tag}: {err:.3e} against a scale of {scale:.3e}"


@pytest.mark.parametrize("mask_kind", ["null", "prefix", "holes", "single"])
@pytest.mark.parametrize("L,with_rb,p", [(1, False, 0.0), (5, True, 0.3), (33, False, 0.3), (33, True, 0.0), (40, True, 0.5)])
def test_attention_bwd_ref_is_float64_autograd(L, with_rb, p, mask_kind):
    import torch
    B, heads, scale = 2, 3, 0.125
    H = heads * 64
    g = bc.gen("ref", L, with_rb, p, mask_kind)
    mask = bc.make_mask(mask_kind, B, L, g)
    qkv, dctx = bc.make_qkv_dctx("gauss", B, L, heads, mask, g)
    table = 2 * torch.randn(heads, 2 * L - 1, generator=g) if with_rb else None
    keep = bc.make_keep(B, L, heads, p, mask, g) if p > 0 else None
    ref = br.attention_bwd_ref(qkv, dctx, mask, B, L, heads, scale, relbias=table, keep=keep, p=p)

    def split(x):
        return x.reshape(B, L, heads, 64).transpose(1, 2)

    qs = split((qkv[:, :H].float() * scale).to(torch.bfloat16).double()).requires_grad_(True)
    k = split(qkv[:, H:2 * H].double()).requires_grad_(True)
    v = split(qkv[:, 2 * H:].double()).requires_grad_(True)
    s = qs @ k.transpose(-1, -2)
    tb = None
    if with_rb:
        tb = table.double().requires_grad_(True)
        idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
        s = s + tb[:, idx]
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], -math.inf)
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.double() / (1 - p)
    o = (pr @ v).transpose(1, 2).reshape(B * L, H)
    o.backward(dctx.double())

    def merge(x):
        return x.transpose(1, 2).reshape(B * L, H)

    tag = f"L={L} rb={with_rb} p={p} {mask_kind}"
    _close(ref.O, o.detach(), tag + " O")
    _close(ref.lse, torch.logsumexp(s.detach(), -1), tag + " lse")
    want = torch.cat([scale * merge(qs.grad), merge(k.grad), merge(v.grad)], 1)
    for i, name in enumerate(("dQ", "dK", "dV")):
        _close(ref.dqkv[:, i * H:(i + 1) * H], want[:, i * H:(i + 1) * H], f"{tag} {name}", ref.A[:, i * H:(i + 1) * H])
    if with_rb:
        _close(ref.dtable, tb.grad, tag + " dtable", ref.A_T)
    else:
        assert ref.dtable is None
    # the error scales dominate the values they scale, and vanish exactly on masked keys
    assert (ref.dqkv.abs() <= ref.A * (1 + 1e-12) + 1e-300).all()
    if mask is not None:
        gone = (mask == 0).reshape(B * L)
        assert (ref.A[gone][:, H:] == 0).all() and (ref.dqkv[gone][:, H:] == 0).all()


def test_attention_bwd_ref_dead_sequence_contract():
    """Every key masked: P uniform over the L keys whatever Q, K and relbias hold -- dQ, dK and the
    share of dtable are zero, dV = sum_q keep dO_q / (L (1 - p)); the other sequences as without it."""
    import torch
    B, L, heads, p = 3, 7, 2, 0.25
    H = heads * 64
    g = bc.gen("dead-ref")
    mask = bc.make_mask("prefix", B, L, g)
    mask[1] = 0
    qkv, dctx = bc.make_qkv_dctx("gauss", B, L, heads, mask, g, keep_v=(1,))
    table = 2 * torch.randn(heads, 2 * L - 1, generator=g)
    keep = bc.make_keep(B, L, heads, p, mask, g)
    ref = br.attention_bwd_ref(qkv, dctx, mask, B, L, heads, 1.0, relbias=table, keep=keep, p=p)
    d = ref.dqkv.reshape(B, L, 3 * H)
    assert (d[1, :, :2 * H] == 0).all() and (ref.A.reshape(B, L, 3 * H)[1, :, :2 * H] == 0).all()
    do = dctx.double().reshape(B, L, heads, 64)[1]
    want = torch.einsum("hqk,qhd->khd", keep[1].double(), do) / (L * (1 - p))
    _close(d[1, :, 2 * H:], want.reshape(L, H), "dead dV")
    v = qkv[:, 2 * H:].double().reshape(B, L, heads, 64)[1]
    o = torch.einsum("hqk,khd->qhd", keep[1].double(), v) / (L * (1 - p))
    _close(ref.O.reshape(B, L, H)[1], o.reshape(L, H), "dead O")
    sel = torch.tensor([0, 2])
    rows = (sel[:, None] * L + torch.arange(L)[None, :]).reshape(-1)
    ref2 = br.attention_bwd_ref(qkv.reshape(B, L, -1)[sel].reshape(2 * L, -1), dctx.reshape(B, L, -1)[sel].reshape(2 * L, -1),
                                mask[sel], 2, L, heads, 1.0, relbias=table, keep=keep[sel], p=p)
    assert torch.equal(ref.dqkv[rows], ref2.dqkv)
    _close(ref.dtable, ref2.dtable, "dtable without the dead sequence", ref.A_T)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("M,H", [(1, 256), (7, 768)])
def test_layernorm_bwd_ref_is_float64_autograd(M, H, with_res):
    import torch
    g = bc.gen("ln-ref", M, H, with_res)
    x = (30 + 0.5 * torch.randn(M, H, generator=g)).to(torch.bfloat16)
    dy = torch.randn(M, H, generator=g).to(torch.bfloat16)
    gamma = 1 + 0.2 * torch.randn(H, generator=g)
    dres = torch.randn(M, H, generator=g).to(torch.bfloat16) if with_res else None
    eps = 1e-12
    ref = br.layernorm_bwd_ref(dy, x, gamma, eps, dres)
    xf = x.double().requires_grad_(True)
    gf = gamma.double().requires_grad_(True)
    bf = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xf, (H,), gf, bf, eps).backward(dy.double())
    _close(ref.dx, xf.grad + (dres.double() if with_res else 0.0), "dx")
    _close(ref.dgamma, gf.grad, "dgamma")
    _close(ref.dbeta, bf.grad, "dbeta")
    assert (ref.dx.abs() <= ref.A_LN * (1 + 1e-12)).all()


def test_pack_bits_layout():
    """bit key & 31 of word (query, key >> 5), keys >= L zero, as include/drt.h states drop_bits."""
    import torch
    L = 70
    keep = torch.rand(1, 2, L, L, generator=bc.gen("bits")) < 0.5
    words = bc.pack_bits(keep)
    assert words.shape == (1, 2, L, 3) and words.dtype == torch.int32
    for q, key in ((0, 0), (3, 31), (69, 32), (5, 69), (64, 63)):
        for h in range(2):
            assert bool((int(words[0, h, q, key >> 5]) >> (key & 31)) & 1) == bool(keep[0, h, q, key])
    assert ((words[..., 2].to(torch.int64) & 0xFFFFFFFF) >> (L - 64) == 0).all()


EMU_LS = (1, 33, 160, 200)


@pytest.mark.parametrize("data", bc.DATA_KINDS)
@pytest.mark.parametrize("L", EMU_LS)
@pytest.mark.parametrize("variant", ["plain", "keep01", "keep05", "relbias", "relbias_keep01"])
def test_emulated_roundings_stay_under_the_gpu_bounds(L, data, variant):
    """The kernels' roundings alone (O in bf16, lse in fp32, P and dS in bf16, one bf16 rounding per
    output) stay under the bounds the GPU test asserts, under every mask kind and with a sequence whose
    every key is masked; masked keys give exact zeros."""
    import torch
    B, heads = 3, 2
    rb = variant.startswith("relbias")
    p = {"plain": 0.0, "keep01": 0.1, "keep05": 0.5, "relbias": 0.0, "relbias_keep01": 0.1}[variant]
    scale, qk = (1.0, 0.35) if rb else (0.125, 1.0)
    worst, bad = {}, []
    for mk in bc.MASK_KINDS + ("dead",):
        g = bc.gen("emu", L, data, variant, mk)
        if mk == "dead":
            mask = bc.make_mask("prefix", B, L, g)
            mask[1] = 0
        else:
            mask = bc.make_mask(mk, B, L, g)
        qkv, dctx = bc.make_qkv_dctx(data, B, L, heads, mask, g, keep_v=(1,) if mk == "dead" else (), qk_scale=qk)
        table = 2 * torch.randn(heads, 2 * L - 1, generator=g) if rb else None
        keep = bc.make_keep(B, L, heads, p, mask, g, starve=p == 0.5) if p > 0 else None
        ref = br.attention_bwd_ref(qkv, dctx, mask, B, L, heads, scale, relbias=table, keep=keep, p=p)
        dqkv, dtable = bc.emulate_attention_bwd(qkv, dctx, mask, B, L, heads, scale, ref, relbias=table, keep=keep, p=p)
        ratios = bc.attention_ratios(dqkv, dtable, ref)
        for n, r in ratios.items():
            worst[n] = max(worst.get(n, 0.0), r)
        bad += [f"{mk}: {t}" for t in bc.over_bounds(ratios)]
    print(f"emulation L={L} {data} {variant}: " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert not bad, f"L={L} {data} {variant}: " + "; ".join(bad)

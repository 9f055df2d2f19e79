"""The encoder forward kernels (csrc/encoder.hip) against the plain fp64 references of
tests/encoder_refs.py, through the native entry points: attention ctx / lse at every NB
instantiation, the 5-wave variant and both store paths under five mask kinds with poisoned masked
keys; embed_ln at every H / 64 instantiation with ragged token tails; the three pooling modes and
the L2 normalisation at widths that are no multiple of the block.

Bounds.  u = 2^-8 is bf16's unit roundoff.  Attention rounds P to bf16 before the P V product
(at most u A elementwise, A = P |V|) and rounds the output (at most u A), so the derived worst case
is 2 u A; the assertion allows 2.5 u A + 1e-7, the extra 0.5 u for the fp32 score chain and the
hardware exp2.  embed_ln rounds its output once.  Pooling modes 0 / 2 are exact, mode 1 is an fp32
sequential sum; the L2 norm is an fp32 tree sum of H squares.
"""
import math
import zlib

import pytest

import attention_abi as abi
import encoder_refs as er

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
B_ATT = 3
ATT_LS = (1, 31, 32, 33, 64, 96, 100, 128, 129, 160, 161, 192, 257, 512)
ATT_SHAPES = [(L, 12) for L in ATT_LS] + [(L, 4) for L in (33, 160, 161)]
MASK_KINDS = ("null", "prefix", "left", "holes", "single")
# ramp: k_j = slope j d, the row max climbs 16 log2 units per 32-key tile at slope 0.35 (the
# running max moves at every tile) and 6.9 at slope 0.15 (it moves at every other tile and P
# reaches 2^6.9 in between)
DATA_KINDS = ("gauss", "peaked", "ramp", "ramp_slow")


def _gen(*key):
    import torch
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _mask(kind, B, L, g):
    import torch
    if kind == "null":
        return None
    mask = torch.ones(B, L, dtype=torch.int64)
    if kind == "prefix":
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0] = max(1, L // 2)
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
    elif kind == "left":          # the whole first 32-key tile masked when L > 32
        mask[:, :min(L - 1, 40)] = 0
    elif kind == "holes":
        mask = (torch.rand(B, L, generator=g) < 0.6).to(torch.int64)
        mask[:, L - 1] = 1
    elif kind == "single":
        mask.zero_()
        mask[torch.arange(B), torch.randint(0, L, (B,), generator=g)] = 1
    else:
        raise ValueError(kind)
    return mask


def _qkv(kind, B, L, heads, mask, g, keep_v=()):
    """Packed bf16 [B*L, 3*H].  Masked keys are poisoned (K x 50, V = 1e4, finite): a masked key
    leaking at any weight, or a read running into a neighbour's rows, moves ctx by orders of
    magnitude.  Sequences listed in keep_v keep their V."""
    import torch
    shape = (B, L, heads, 64)

    def bf(x):
        return x.to(torch.bfloat16).float()

    q, k, v = (torch.randn(shape, generator=g) for _ in range(3))
    if kind == "peaked":
        q, k = q * 3, k * 3
    elif kind in ("ramp", "ramp_slow"):
        slope = 0.35 if kind == "ramp" else 0.15
        d = torch.randn(B, 1, heads, 64, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        q = 8 * d + 0.1 * q
        k = slope * torch.arange(L, dtype=torch.float32)[None, :, None, None] * d + 0.1 * k
    elif kind != "gauss":
        raise ValueError(kind)
    q, k, v = bf(q), bf(k), bf(v)
    if mask is not None:
        dead = (mask == 0)[:, :, None, None]
        k = torch.where(dead, bf(k * 50), k)
        vdead = dead.clone()
        vdead[list(keep_v)] = False
        v = torch.where(vdead, torch.full_like(v, 1e4), v)
    H = heads * 64
    return torch.cat([x.reshape(B * L, H) for x in (q, k, v)], 1).to(torch.bfloat16)


def _run_attention(lib, dev, qkv, mask, B, L, heads):
    """(ctx of drt_attention_forward_bf16 without lse, ctx and lse of the call with it) on the CPU.  The
    outputs start as NaN: an unwritten element fails the finiteness checks."""
    import torch
    from denseretrievaltoolkits_amd import _native
    H = heads * 64
    qd = qkv.to(dev)
    md = None if mask is None else mask.to(dev)
    ctx0 = torch.full((B * L, H), float("nan"), dtype=torch.bfloat16, device=dev)
    ctx1 = torch.full_like(ctx0, float("nan"))
    lse = torch.full((B, heads, L), float("nan"), device=dev)
    _native.check(abi.forward(lib, qd, ctx0, B, L, heads, mask=md, scale=0.125), "attention")
    _native.check(abi.forward(lib, qd, ctx1, B, L, heads, mask=md, lse=lse, scale=0.125), "attention lse")
    torch.cuda.synchronize()
    return ctx0.cpu(), ctx1.cpu(), lse.cpu()


def _ctx_ratio(ctx, ref, A):
    """max over elements of (|ctx - ref| - 1e-7) / (u A): the assertion is ratio <= 2.5."""
    err = (ctx.double() - ref).abs()
    return float(((err - 1e-7).clamp(min=0) / (U * A)).max())


@pytest.mark.parametrize("data", DATA_KINDS)
@pytest.mark.parametrize("L,heads", ATT_SHAPES)
def test_attention_ctx_lse_vs_fp64(dev, L, heads, data):
    """ctx within 2.5 u A + 1e-7 of fp64 and lse within the project's tolerance, under every mask
    kind; ctx of the two entry points bit-equal.

    Measured on an MI355X: worst ctx error 1.914 u A (L = 160, peaked), worst lse error 3.2e-5
    (L = 512, ramp); recorded in the attention paragraph of DESIGN.md."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B = B_ATT
    worst, worst_lse, bad = 0.0, 0.0, []
    for mk in MASK_KINDS:
        g = _gen("att", L, heads, data, mk)
        mask = _mask(mk, B, L, g)
        qkv = _qkv(data, B, L, heads, mask, g)
        ref, A, rlse = er.attention_ref(qkv, mask, B, L, heads, 0.125)
        ctx0, ctx1, lse = _run_attention(lib, dev, qkv, mask, B, L, heads)
        if not torch.equal(ctx0.view(torch.int16), ctx1.view(torch.int16)):
            bad.append(f"{mk}: ctx of the two entry points differs")
        if not (torch.isfinite(ctx0.float()).all() and torch.isfinite(lse).all()):
            bad.append(f"{mk}: non-finite output")
            continue
        ratio = _ctx_ratio(ctx1, ref, A)
        dl = (lse.double() - rlse).abs()
        worst, worst_lse = max(worst, ratio), max(worst_lse, float(dl.max()))
        if ratio > 2.5:
            bad.append(f"{mk}: ctx error {ratio:.3f} u A > 2.5 u A")
        if not (dl <= 1e-3 + 1e-4 * rlse.abs()).all():
            bad.append(f"{mk}: lse error {float(dl.max()):.3e} at |lse| <= {float(rlse.abs().max()):.1f}")
    print(f"attention L={L} heads={heads} {data}: worst ctx error {worst:.3f} u A, worst lse error {worst_lse:.2e}")
    assert not bad, f"L={L} heads={heads} {data}: " + "; ".join(bad)


@pytest.mark.parametrize("L", [32, 33, 100, 160, 161])
def test_attention_fully_masked_row(dev, L):
    """A sequence with every key masked gets the uniform mean of V over its L keys (HF's softmax of
    L equal finfo.min scores), not over the keys padded to the 32-key tile; everything is finite and
    the other sequences keep their bits.  The dead sequence keeps its own V (a poisoned V would make
    the mean trivial) and gets K x 50 like every masked key."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, heads = B_ATT, 12
    g = _gen("dead", L)
    mask = _mask("prefix", B, L, g)
    mask[1] = 0
    qkv = _qkv("gauss", B, L, heads, mask, g, keep_v=(1,))
    ref, A, rlse = er.attention_ref(qkv, mask, B, L, heads, 0.125)
    ctx0, ctx1, lse = _run_attention(lib, dev, qkv, mask, B, L, heads)
    assert torch.equal(ctx0.view(torch.int16), ctx1.view(torch.int16))
    assert torch.isfinite(ctx1.float()).all() and torch.isfinite(lse).all()
    H = heads * 64
    v = qkv[:, 2 * H:].double().reshape(B, L, H)
    torch.testing.assert_close(ref.reshape(B, L, H)[1], v[1].mean(0, keepdim=True).expand(L, H), atol=1e-12, rtol=1e-12)
    ratio = _ctx_ratio(ctx1, ref, A)
    dead_ratio = _ctx_ratio(ctx1.reshape(B, L, H)[1], ref.reshape(B, L, H)[1], A.reshape(B, L, H)[1])
    print(f"fully masked L={L}: worst ctx error {ratio:.3f} u A (dead sequence {dead_ratio:.3f} u A)")
    assert ratio <= 2.5
    live = [0, 2]
    dl = (lse.double() - rlse).abs()[live]
    assert (dl <= 1e-3 + 1e-4 * rlse.abs()[live]).all()
    # the other sequences do not see their neighbour's mask
    mask2 = mask.clone()
    mask2[1] = 1
    _, ctx2, lse2 = _run_attention(lib, dev, qkv, mask2, B, L, heads)
    c1, c2 = ctx1.reshape(B, L, H), ctx2.reshape(B, L, H)
    assert torch.equal(c1[live].view(torch.int16), c2[live].view(torch.int16))
    assert torch.equal(lse[live], lse2[live])


# ---------------------------------------------------------------------------------------------
# drt_embed_ln / drt_embed_ln_pre
# ---------------------------------------------------------------------------------------------
VOCAB = 1000


@pytest.mark.parametrize("B,L", [(1, 1), (3, 5), (2, 512), (5, 33)])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_embed_ln_vs_fp64(dev, H, B, L):
    """out within one bf16 rounding of the fp64 LayerNorm (2^-8 |ref| + 2^-8 |beta| + 1e-6; the fp32
    LayerNorm is far below that), pre = the bf16 rounding of the fp32 sum bit for bit, out of the two
    entry points bit-equal, and nothing written past token T - 1 (4 tokens per block: T % 4 =
    1, 3, 0, 1)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    T = B * L
    s = _native.stream_ptr(dev)
    runs = [(False, 0.02), (True, 0.02)] + ([(True, 1.0)] if (B, L) == (5, 33) else [])
    for with_types, scale in runs:
        g = _gen("emb", H, B, L, with_types, scale)
        word = scale * torch.randn(VOCAB, H, generator=g)
        pos = scale * torch.randn(512, H, generator=g)
        typ = scale * torch.randn(2, H, generator=g)
        gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
        ids = torch.randint(0, VOCAB, (B, L), generator=g)
        ids.view(-1)[T - 1] = VOCAB - 1            # both ends of the table (T = 1: one per run)
        ids.view(-1)[0] = 0 if T > 1 or with_types else VOCAB - 1
        tt = torch.randint(0, 2, (B, L), generator=g) if with_types else None
        eps = 1e-12
        ref = er.embed_ln_ref(ids, tt, L, word, pos, typ, gamma, beta, eps)
        d = [x.to(dev) for x in (ids, word, pos, typ, gamma, beta)]
        ttd = None if tt is None else tt.to(dev)
        ttp = None if ttd is None else ttd.data_ptr()
        # 4 guard rows behind each output
        out0, out1, pre = (torch.full((T + 4, H), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(3))
        _native.check(lib.drt_embed_ln(d[0].data_ptr(), ttp, B, L, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                       d[4].data_ptr(), d[5].data_ptr(), eps, H, out0.data_ptr(), s), "embed_ln")
        _native.check(lib.drt_embed_ln_pre(d[0].data_ptr(), ttp, B, L, d[1].data_ptr(), d[2].data_ptr(),
                                           d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), eps, H, out1.data_ptr(),
                                           pre.data_ptr(), s), "embed_ln_pre")
        torch.cuda.synchronize()
        out0, out1, pre = out0.cpu(), out1.cpu(), pre.cpu()
        tag = f"H={H} B={B} L={L} types={with_types} scale={scale}"
        for o in (out0, out1, pre):
            assert torch.isnan(o[T:].float()).all(), f"{tag}: rows past T written"
            assert torch.isfinite(o[:T].float()).all(), tag
        err = (out0[:T].double() - ref).abs()
        bound = U * ref.abs() + U * beta.double().abs()[None, :] + 1e-6
        over = err - bound
        print(f"embed_ln {tag}: worst err / bound {float((err / bound).max()):.3f}")
        assert (over <= 0).all(), f"{tag}: err exceeds the bound by {float(over.max()):.3e}"
        assert torch.equal(out0[:T].view(torch.int16), out1[:T].view(torch.int16)), tag
        want_pre = er.embed_sum(ids, tt, L, word, pos, typ, torch.float32).to(torch.bfloat16)
        assert torch.equal(pre[:T].view(torch.int16), want_pre.view(torch.int16)), tag


# ---------------------------------------------------------------------------------------------
# drt_pool_bf16 / drt_l2_normalize_f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(1, 1), (4, 37), (2, 512)])
@pytest.mark.parametrize("H", [64, 256, 768, 1000])
def test_pool_vs_fp64(dev, H, B, L):
    """Modes 0 (first) and 2 (max of hidden * mask) exact against fp64 on the bf16 inputs, mode 1
    within fp32 sequential summation of the mean; sequence 0 is all negative, so mode 2 must give 0
    where any of its tokens is masked and the true negative max where none is; a sequence with every
    token masked has mean 0; out_bf16 is the exact bf16 rounding of out."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    s = _native.stream_ptr(dev)
    g = _gen("pool", H, B, L)
    h = torch.randn(B, L, H, generator=g)
    h[0] = -h[0].abs() - 0.1
    h = h.to(torch.bfloat16)
    hd = h.to(dev)
    for mk in ("null", "prefix", "holes", "allzero"):
        if mk == "allzero":
            mask = _mask("prefix", B, L, g)
            mask[B - 1] = 0
        else:
            mask = _mask(mk, B, L, g)
            if mk == "holes" and L > 1:
                mask[0, 0] = 0
        md = None if mask is None else mask.to(dev)
        mp = None if md is None else md.data_ptr()
        for mode in (0, 1, 2):
            out = torch.full((B + 1, H), float("nan"), device=dev)
            ob = torch.full((B + 1, H), float("nan"), dtype=torch.bfloat16, device=dev)
            _native.check(lib.drt_pool_bf16(hd.data_ptr(), mp, B, L, H, mode, out.data_ptr(), ob.data_ptr(), s), "pool")
            torch.cuda.synchronize()
            out, ob = out.cpu(), ob.cpu()
            tag = f"H={H} B={B} L={L} mask={mk} mode={mode}"
            assert torch.isnan(out[B:]).all() and torch.isnan(ob[B:].float()).all(), f"{tag}: rows past B written"
            out, ob = out[:B], ob[:B]
            ref = er.pool_ref(h, mask, mode)
            if mode == 1:
                m = torch.ones(B, L, dtype=torch.float64) if mask is None else mask.double()
                sabs = (h.double().abs() * m[:, :, None]).sum(1)
                bound = L * 2.0 ** -24 * sabs / m.sum(1, keepdim=True).clamp(min=1e-9) + 1e-7
                err = (out.double() - ref).abs()
                assert (err <= bound).all(), f"{tag}: err / bound {float((err / bound).max()):.3f}"
                if mask is not None:
                    dead = mask.sum(1) == 0
                    assert (out[dead] == 0).all(), tag
            else:
                assert torch.equal(out.double(), ref), tag
            if mode == 2:
                full = mask is None or bool(mask[0].all())
                if full:
                    assert torch.equal(out[0].double(), h[0].double().max(0)[0]) and (out[0] < 0).all(), tag
                else:
                    assert (out[0] == 0).all(), tag
            assert torch.equal(ob.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), tag


@pytest.mark.parametrize("H", [1, 100, 128, 768, 1000])
def test_l2_normalize_vs_fp64(dev, H):
    """x / max(||x||, 1e-12) within rtol 4 2^-24 sqrt(H) of fp64 for any H (128 = a LinearHead's
    output), an all-zero row stays zero, out_bf16 is the exact bf16 rounding."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B = 5
    g = _gen("l2", H)
    x = torch.randn(B, H, generator=g) * torch.tensor([1.0, 1e-3, 1e3, 1.0, 7.0])[:, None]
    x[3] = 0
    ref = er.l2_ref(x)
    xd = torch.full((B + 1, H), float("nan"), device=dev)
    xd[:B] = x.to(dev)
    ob = torch.full((B + 1, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_l2_normalize_f32(xd.data_ptr(), B, H, ob.data_ptr(), _native.stream_ptr(dev)), "l2")
    torch.cuda.synchronize()
    out, ob = xd.cpu(), ob.cpu()
    assert torch.isnan(out[B:]).all() and torch.isnan(ob[B:].float()).all()
    out, ob = out[:B], ob[:B]
    assert (out[3] == 0).all()
    err = (out.double() - ref).abs()
    rtol = 4 * 2.0 ** -24 * math.sqrt(H)
    print(f"l2 H={H}: worst err / (rtol |ref|) {float((err / (rtol * ref.abs() + 1e-300)).max()):.3f}")
    assert (err <= rtol * ref.abs()).all()
    assert torch.equal(ob.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))

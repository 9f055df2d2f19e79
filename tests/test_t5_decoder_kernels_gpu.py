"""The one-step T5 decoder kernels (csrc/t5_decoder.hip) against the plain fp64 references of
tests/t5_decoder_refs.py, through the native entries.

Bounds.  u = 2^-8 is bf16's unit roundoff.  The cross-attention pool has the arithmetic of the
attention kernels (P rounded to bf16 before the P E product, fp32 accumulation, one output rounding):
the bound is theirs, 2.5 u A + 1e-7 with A = P |E| (tests/test_t5_kernels_gpu.py,
test_attention_relbias_vs_fp64).  The per-head projections use the project's linear-epilogue
tolerance (atol 3e-2, rtol 1e-2 against the exact result of the bf16 inputs).
"""
import pytest

import t5_decoder_refs as dr
from test_encoder_fwd_fp64_gpu import _gen, _mask

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
B_POOL = 3
POOL_LS = (1, 15, 16, 17, 33, 160, 161, 512)
POOL_SHAPES = ((2, 256), (6, 512), (12, 768), (16, 1024))
POOL_MASKS = ("null", "prefix", "holes", "single")
POISON = 1e4
LIN_TOL = dict(atol=3e-2, rtol=1e-2)


def _bits(x):
    import torch
    return x.view(torch.int16)


def _pool_inputs(B, L, heads, D, mask, g, score_std, keep=()):
    """bf16 qt [B, heads, D] and enc [B, L, D]: enc ~ N(0, 1), qt ~ N(0, score_std^2 / D), so a score
    has standard deviation score_std.  Masked rows of enc are poisoned with 1e4 (finite): a masked key
    leaking at any weight, or a read running into a neighbour's rows, moves the result by orders of
    magnitude.  Sequences listed in keep keep their rows."""
    import torch
    qt = (torch.randn(B, heads, D, generator=g) * (score_std / D ** 0.5)).to(torch.bfloat16)
    enc = torch.randn(B, L, D, generator=g)
    if mask is not None:
        deadrow = (mask == 0)[:, :, None].clone()
        deadrow[list(keep)] = False
        enc = torch.where(deadrow, torch.full_like(enc, POISON), enc)
    return qt, enc.to(torch.bfloat16)


def _run_pool(lib, dev, qt, enc, mask):
    """pooled of drt_t5_cross_pool_bf16 on the CPU, [B, heads, D]; the output starts as NaN and has two
    spare rows that must stay NaN."""
    import torch
    from denseretrievaltoolkits_amd import _native
    B, heads, D = qt.shape
    L = enc.shape[1]
    qd, ed = qt.contiguous().to(dev), enc.contiguous().to(dev)
    md = None if mask is None else mask.to(dev)
    out = torch.full((B * heads + 2, D), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_t5_cross_pool_bf16(qd.data_ptr(), ed.data_ptr(), None if md is None else md.data_ptr(),
                                             out.data_ptr(), B, L, heads, D, _native.stream_ptr(dev)), "cross_pool")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[B * heads:].float()).all(), "rows past B * heads written"
    return out[:B * heads].reshape(B, heads, D)


def _ratio(got, ref, A):
    """max over elements of (|got - ref| - 1e-7) / (u A): the assertion is ratio <= 2.5."""
    err = (got.double() - ref).abs()
    return float(((err - 1e-7).clamp(min=0) / (U * A)).max())


@pytest.mark.parametrize("heads,D", POOL_SHAPES)
@pytest.mark.parametrize("L", POOL_LS)
def test_cross_pool_vs_fp64(dev, L, heads, D):
    """pooled within 2.5 u A + 1e-7 of fp64 under every mask kind, masked rows of enc poisoned.  The
    null and holes masks run scores of standard deviation 1, the prefix and single masks 8.

    Measured on an MI355X: worst error 1.616 u A (L = 160, 12 heads, D = 768); recorded in the T5
    rerankers paragraph of DESIGN.md §4."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B = B_POOL
    worst, bad = 0.0, []
    for mk in POOL_MASKS:
        g = _gen("t5pool", L, heads, D, mk)
        mask = _mask(mk, B, L, g)
        qt, enc = _pool_inputs(B, L, heads, D, mask, g, 1.0 if mk in ("null", "holes") else 8.0)
        ref, A = dr.cross_pool_ref(qt, enc, mask)
        got = _run_pool(lib, dev, qt, enc, mask)
        if not torch.isfinite(got.float()).all():
            bad.append(f"{mk}: non-finite output")
            continue
        ratio = _ratio(got, ref, A)
        worst = max(worst, ratio)
        if ratio > 2.5:
            bad.append(f"{mk}: error {ratio:.3f} u A > 2.5 u A")
    print(f"cross pool L={L} heads={heads} D={D}: worst error {worst:.3f} u A")
    assert not bad, f"L={L} heads={heads} D={D}: " + "; ".join(bad)


@pytest.mark.parametrize("L", [33, 160])
def test_cross_pool_fully_masked_sequence(dev, L):
    """A sequence with every key masked gets the mean of its own L rows of enc, finite; the other
    sequences keep their bits when that sequence's mask is flipped to ones."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, heads, D = B_POOL, 12, 768
    g = _gen("t5pooldead", L)
    mask = _mask("prefix", B, L, g)
    mask[1] = 0
    qt, enc = _pool_inputs(B, L, heads, D, mask, g, 8.0, keep=(1,))
    ref, A = dr.cross_pool_ref(qt, enc, mask)
    torch.testing.assert_close(ref[1], enc[1].double().mean(0, keepdim=True).expand(heads, D), atol=1e-12, rtol=1e-12)
    got = _run_pool(lib, dev, qt, enc, mask)
    assert torch.isfinite(got.float()).all()
    ratio = _ratio(got, ref, A)
    print(f"cross pool fully masked L={L}: worst error {ratio:.3f} u A")
    assert ratio <= 2.5
    mask2 = mask.clone()
    mask2[1] = 1
    got2 = _run_pool(lib, dev, qt, enc, mask2)
    live = [0, 2]
    assert torch.equal(_bits(got[live]), _bits(got2[live]))
    assert not torch.equal(_bits(got[1]), _bits(got2[1]))      # the flip reached the kernel


@pytest.mark.parametrize("heads,D", [(6, 512), (12, 768)])
def test_cross_pool_heads_independent(dev, heads, D):
    """A one-head call with only head h's qt row gives the full call's row h bit for bit: heads do
    not mix and the rows that pad the head tile to 16 are inert."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, L = B_POOL, 161
    g = _gen("t5poolheads", heads, D)
    mask = _mask("prefix", B, L, g)
    qt, enc = _pool_inputs(B, L, heads, D, mask, g, 8.0)
    full = _run_pool(lib, dev, qt, enc, mask)
    assert torch.isfinite(full.float()).all()
    for h in range(heads):
        one = _run_pool(lib, dev, qt[:, h:h + 1], enc, mask)
        assert torch.equal(_bits(one[:, 0]), _bits(full[:, h])), f"head {h}"


def _run_head(fn, dev, x, w, B, heads, D, out_cols, name):
    import torch
    from denseretrievaltoolkits_amd import _native
    xd, wd = x.contiguous().to(dev), w.contiguous().to(dev)
    out = torch.full((B + 1, out_cols), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(fn(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), B, heads, D, _native.stream_ptr(dev)), name)
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[B:].float()).all(), "rows past B written"
    assert torch.isfinite(out[:B].float()).all()
    return out[:B]


def _far_outside(a, b):
    """Somewhere |a - b| exceeds ten times the linear tolerance."""
    return bool(((a - b).abs() > 10 * (LIN_TOL["atol"] + LIN_TOL["rtol"] * b.abs())).any())


@pytest.mark.parametrize("heads,D", [(2, 256), (6, 512), (12, 768)])
@pytest.mark.parametrize("B", [1, 5, 300])
def test_head_expand_reduce_vs_fp64(dev, B, heads, D):
    """qt = q through Wk's head blocks and ctx = pooled through Wv's, each within atol 3e-2, rtol 1e-2
    of fp64 of the bf16 inputs; nothing written past row B - 1.  The inputs discriminate: a reference in
    which head h used head h + 1's weight block is far outside that tolerance."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    I = heads * 64
    g = _gen("t5heads", B, heads, D)
    q = torch.randn(B, I, generator=g).to(torch.bfloat16)
    pooled = torch.randn(B, heads, D, generator=g).to(torch.bfloat16)
    wk = (0.05 * torch.randn(I, D, generator=g)).to(torch.bfloat16)
    wv = (0.05 * torch.randn(I, D, generator=g)).to(torch.bfloat16)
    ref_qt = dr.head_expand_ref(q, wk, heads)
    ref_ctx = dr.head_reduce_ref(pooled, wv, heads)
    assert _far_outside(dr.head_expand_ref(q, wk.roll(-64, 0), heads), ref_qt)
    assert _far_outside(dr.head_reduce_ref(pooled, wv.roll(-64, 0), heads), ref_ctx)
    qt = _run_head(lib.drt_t5_head_expand_bf16, dev, q, wk, B, heads, D, heads * D, "head_expand")
    torch.testing.assert_close(qt.double().reshape(B, heads, D), ref_qt, **LIN_TOL)
    ctx = _run_head(lib.drt_t5_head_reduce_bf16, dev, pooled, wv, B, heads, D, I, "head_reduce")
    torch.testing.assert_close(ctx.double(), ref_ctx, **LIN_TOL)

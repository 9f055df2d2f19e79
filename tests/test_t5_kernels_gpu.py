"""The T5 kernels (csrc/t5.hip, the RB attention of csrc/encoder.hip, the ReLU epilogue of
csrc/gemm.hip) against the plain fp64 references of tests/t5_refs.py, through the native entries.

Bounds.  u = 2^-8 is bf16's unit roundoff.  RMSNorm and the embedding gather round once.  The
attention bound is the one of tests/test_encoder_fwd_fp64_gpu.py (P rounded to bf16 before P V and
the output rounded: 2 u A with A = P |V|, asserted as 2.5 u A + 1e-7); the relative bias adds one
fp32 add to the score chain, inside that bound's 0.5 u slack.  The linear epilogues use the project's
bf16 bounds (tests/test_encoder_gpu.py: atol 3e-2, rtol 1e-2 against the exact result of the bf16
inputs).
"""
import pytest

import attention_abi as abi
import t5_refs as tr
from test_encoder_fwd_fp64_gpu import _ctx_ratio, _gen, _mask, _qkv

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
B_ATT = 3
ATT_LS = (1, 31, 33, 128, 129, 160, 161, 257, 512)
ATT_MASKS = ("null", "prefix", "holes", "single")


def _bits(x):
    import torch
    return x.view(torch.int16)


# ---------------------------------------------------------------------------------------------
# drt_rmsnorm_bf16 / drt_t5_embed_bf16
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 1031])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_rmsnorm_vs_fp64(dev, H, M):
    """|err| <= u |ref| + 1e-6 at row scales 1e-2, 1 and 1e3 with |w| <= 4 (one output rounding; the
    fp32 statistics error is far below it); nothing written past row M - 1; in place gives the same bits."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    s = _native.stream_ptr(dev)
    g = _gen("rms", H, M)
    scale = torch.tensor([1e-2, 1.0, 1e3])[torch.arange(M) % 3]
    x = (torch.randn(M, H, generator=g) * scale[:, None]).to(torch.bfloat16)
    w = torch.rand(H, generator=g) * 8 - 4
    eps = 1e-6
    ref = tr.rmsnorm_ref(x, w, eps)
    xd, wd = x.to(dev), w.to(dev)
    out = torch.full((M + 4, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_rmsnorm_bf16(xd.data_ptr(), M, H, wd.data_ptr(), eps, out.data_ptr(), s), "rmsnorm")
    inplace = xd.clone()
    _native.check(lib.drt_rmsnorm_bf16(inplace.data_ptr(), M, H, wd.data_ptr(), eps, inplace.data_ptr(), s), "rmsnorm")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[M:].float()).all(), "rows past M written"
    assert torch.isfinite(out[:M].float()).all()
    err = (out[:M].double() - ref).abs()
    bound = U * ref.abs() + 1e-6
    print(f"rmsnorm H={H} M={M}: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(_bits(inplace.cpu()), _bits(out[:M]))


@pytest.mark.parametrize("H", [256, 768])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (2, 130)])
def test_t5_embed_exact(dev, B, L, H):
    """The exact bf16 rounding of the gathered fp32 rows, id 0 and the last id included; nothing
    written past token T - 1 (4 tokens per block: T % 4 = 1, 1, 0)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    g = _gen("t5emb", B, L, H)
    vocab, T = 500, B * L
    table = torch.randn(vocab, H, generator=g)
    ids = torch.randint(0, vocab, (B, L), generator=g)
    ids.view(-1)[T - 1] = vocab - 1
    ids.view(-1)[0] = 0 if T > 1 else vocab - 1
    td, idd = table.to(dev), ids.to(dev)
    out = torch.full((T + 4, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_t5_embed_bf16(idd.data_ptr(), B, L, td.data_ptr(), H, out.data_ptr(), _native.stream_ptr(dev)),
                  "t5_embed")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[T:].float()).all(), "rows past T written"
    assert torch.equal(_bits(out[:T]), _bits(table[ids.view(-1)].to(torch.bfloat16)))


# ---------------------------------------------------------------------------------------------
# drt_attention_forward_bf16 with relbias
# ---------------------------------------------------------------------------------------------
def _table(kind, heads, L, g):
    """fp32 [heads, 2L-1] over k - q, asymmetric: a transposed index or a sign error moves ctx far
    beyond the bound.  gauss: N(0, 1.5^2); ramp: monotone from -20 to +20 (per head: times
    (h + 1) / heads, so that heads differ)."""
    import torch
    n = 2 * L - 1
    if kind == "gauss":
        return 1.5 * torch.randn(heads, n, generator=g)
    if kind == "ramp":
        ramp = torch.linspace(-20.0, 20.0, n) if n > 1 else torch.zeros(1)
        return ramp[None, :] * ((torch.arange(heads) + 1.0) / heads)[:, None]
    if kind == "zero":
        return torch.zeros(heads, n)
    raise ValueError(kind)


def _soften(qkv, heads):
    """Q / 8 (exact in bf16): scores of a few units, where the bias decides the softmax."""
    qkv = qkv.clone()
    qkv[:, :heads * 64] = (qkv[:, :heads * 64].float() * 0.125).to(qkv.dtype)
    return qkv


def _run_relbias(lib, dev, qkv, mask, table, B, L, heads, scale=1.0):
    """ctx of drt_attention_forward_bf16 with relbias on the CPU; the output starts as NaN."""
    import torch
    from denseretrievaltoolkits_amd import _native
    qd, td = qkv.to(dev), table.to(dev).contiguous()
    md = None if mask is None else mask.to(dev)
    ctx = torch.full((B * L, heads * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(abi.forward(lib, qd, ctx, B, L, heads, mask=md, relbias=td, scale=scale), "attention_relbias")
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("kind", ["gauss", "ramp"])
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("L", ATT_LS)
def test_attention_relbias_vs_fp64(dev, L, heads, kind):
    """ctx within 2.5 u A + 1e-7 of fp64 at scale = 1 under every mask kind, masked keys poisoned.
    The null and holes masks run softened queries (Q / 8), the prefix and single masks the plain
    N(0, 1) ones, whose unscaled scores have a standard deviation of 8.

    Measured on an MI355X: worst ctx error 1.900 u A (L = 128, 12 heads, ramp table); recorded in the
    T5 paragraph of DESIGN.md §4."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B = B_ATT
    worst, bad = 0.0, []
    for mk in ATT_MASKS:
        g = _gen("t5att", L, heads, kind, mk)
        mask = _mask(mk, B, L, g)
        qkv = _qkv("gauss", B, L, heads, mask, g)
        if mk in ("null", "holes"):
            qkv = _soften(qkv, heads)
        table = _table(kind, heads, L, g)
        ref, A = tr.attention_relbias_ref(qkv, mask, table, B, L, heads, 1.0)
        ctx = _run_relbias(lib, dev, qkv, mask, table, B, L, heads)
        if not torch.isfinite(ctx.float()).all():
            bad.append(f"{mk}: non-finite output")
            continue
        ratio = _ctx_ratio(ctx, ref, A)
        worst = max(worst, ratio)
        if ratio > 2.5:
            bad.append(f"{mk}: ctx error {ratio:.3f} u A > 2.5 u A")
    print(f"relbias attention L={L} heads={heads} {kind}: worst ctx error {worst:.3f} u A")
    assert not bad, f"L={L} heads={heads} {kind}: " + "; ".join(bad)


@pytest.mark.parametrize("L", [33, 160])
def test_attention_relbias_fully_masked_row(dev, L):
    """A sequence with every key masked gets the uniform mean of its own V over its L keys (finfo.min
    absorbs scores and biases), finite; the other sequences keep their bits."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, heads = B_ATT, 12
    g = _gen("t5dead", L)
    mask = _mask("prefix", B, L, g)
    mask[1] = 0
    qkv = _qkv("gauss", B, L, heads, mask, g, keep_v=(1,))
    table = _table("gauss", heads, L, g)
    ref, A = tr.attention_relbias_ref(qkv, mask, table, B, L, heads, 1.0)
    ctx = _run_relbias(lib, dev, qkv, mask, table, B, L, heads)
    assert torch.isfinite(ctx.float()).all()
    H = heads * 64
    v = qkv[:, 2 * H:].double().reshape(B, L, H)
    torch.testing.assert_close(ref.reshape(B, L, H)[1], v[1].mean(0, keepdim=True).expand(L, H), atol=1e-12, rtol=1e-12)
    ratio = _ctx_ratio(ctx, ref, A)
    print(f"relbias fully masked L={L}: worst ctx error {ratio:.3f} u A")
    assert ratio <= 2.5
    mask2 = mask.clone()
    mask2[1] = 1
    ctx2 = _run_relbias(lib, dev, qkv, mask2, table, B, L, heads)
    live = [0, 2]
    assert torch.equal(_bits(ctx.reshape(B, L, H)[live]), _bits(ctx2.reshape(B, L, H)[live]))


@pytest.mark.parametrize("scale", [0.125, 1.0])
@pytest.mark.parametrize("L", [1, 33, 128, 160, 161, 512])
def test_attention_relbias_zero_table_bit_identical(dev, L, scale):
    """An all-zero table gives the bits of relbias = NULL at the same scale: the variant is the kernel
    the fp64 suite of tests/test_encoder_fwd_fp64_gpu.py covers."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, heads = B_ATT, 4
    for mk in ("null", "prefix"):
        g = _gen("t5zero", L, mk)
        mask = _mask(mk, B, L, g)
        qkv = _qkv("gauss", B, L, heads, mask, g)
        got = _run_relbias(lib, dev, qkv, mask, _table("zero", heads, L, g), B, L, heads, scale)
        qd = qkv.to(dev)
        md = None if mask is None else mask.to(dev)
        want = torch.full((B * L, heads * 64), float("nan"), dtype=torch.bfloat16, device=dev)
        _native.check(abi.forward(lib, qd, want, B, L, heads, mask=md, scale=scale), "attention")
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want.cpu())), f"L={L} scale={scale} mask={mk}"


# ---------------------------------------------------------------------------------------------
# FFN activations: the ReLU epilogue flag and drt_gated_gelu_new_bf16
# ---------------------------------------------------------------------------------------------
LIN_TOL = dict(atol=3e-2, rtol=1e-2)


def _linear(lib, dev, x, w, b, r, flags, split):
    """drt_linear_bf16_ws with the split-K scratch the plan asks for (split) or drt_linear_bf16
    without one (the direct plan); bf16 [M, N] on the CPU, pre-filled with NaN."""
    import torch
    from denseretrievaltoolkits_amd import _native
    M, K = x.shape
    N = w.shape[0]
    s = _native.stream_ptr(dev)
    xd, wd = x.to(dev), w.to(dev)
    bd = None if b is None else b.to(dev)
    rd = None if r is None else r.to(dev)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    args = (xd.data_ptr(), wd.data_ptr(), None if bd is None else bd.data_ptr(), None if rd is None else rd.data_ptr(),
            out.data_ptr(), M, N, K, flags)
    if split:
        nb = int(lib.drt_linear_workspace(M, N, K))
        assert nb > 0, "this shape was chosen to split K"
        ws = torch.empty(nb // 4, dtype=torch.float32, device=dev)
        _native.check(lib.drt_linear_bf16_ws(*args, ws.data_ptr(), nb, s), "linear_ws")
    else:
        _native.check(lib.drt_linear_bf16(*args, s), "linear")
    torch.cuda.synchronize()
    return out.cpu()


# (4096, 2112, 256): the whole-line 256^2 kernel the encode-sized FFN1 runs, with full tiles (the
# epilogue through LDS) and a partial column tile (the direct epilogue)
@pytest.mark.parametrize("M,N,K,split", [(5, 512, 256, True), (5, 512, 256, False), (300, 512, 256, True),
                                         (300, 512, 256, False), (4096, 2112, 256, False)])
@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_linear_relu_epilogue_vs_fp64(dev, M, N, K, split, resid, bias):
    """relu(X W^T (+ b)) (+ R) in bf16 within atol 3e-2, rtol 1e-2 of fp64 of the bf16 inputs, on the
    split-K finish and on the direct plan; no NaN, and without a residual no negative element."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    g = _gen("relu", M, N, K, resid, bias)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(M, N, generator=g).to(torch.bfloat16) if resid else None
    ref = x.double() @ w.double().T + (b.double() if bias else 0.0)
    ref = ref.clamp(min=0) + (r.double() if resid else 0.0)
    out = _linear(lib, dev, x, w, b, r, 8, split)
    assert not torch.isnan(out.float()).any()
    if not resid:
        assert (out.float() >= 0).all()
        assert ((out.float() == 0) == (ref <= 0))[ref.abs() > 1e-3].all()
    torch.testing.assert_close(out.double(), ref, **LIN_TOL)


@pytest.mark.parametrize("M,split", [(5, True), (5, False), (300, True), (300, False)])
def test_gated_gelu_new_vs_fp64(dev, M, split):
    """The gated-gelu FFN1 as the encoder runs it: one GEMM over [wi_0; wi_1] (N = 2F = 512, K = 256),
    then drt_gated_gelu_new_bf16.  The gate against fp64 of its own bf16 input within one rounding
    (u |ref| + 1e-6: fp32 math, one rounding), and the pair against fp64 of the bf16 GEMM inputs
    within the linear-epilogue bounds."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    F, K = 256, 256
    g = _gen("gated", M)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.08 * torch.randn(2 * F, K, generator=g)).to(torch.bfloat16)
    mid = _linear(lib, dev, x, w, None, None, 0, split)
    md = mid.to(dev)
    out = torch.full((M + 1, F), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_gated_gelu_new_bf16(md.data_ptr(), M, F, out.data_ptr(), _native.stream_ptr(dev)), "gated")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[M:].float()).all(), "rows past M written"
    out = out[:M]
    assert torch.isfinite(out.float()).all()
    own = tr.gelu_new_ref(mid[:, :F]) * mid[:, F:].double()
    err = (out.double() - own).abs()
    bound = U * own.abs() + 1e-6
    print(f"gated gelu_new M={M}: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    y = x.double() @ w.double().T
    torch.testing.assert_close(out.double(), tr.gelu_new_ref(y[:, :F]) * y[:, F:], **LIN_TOL)

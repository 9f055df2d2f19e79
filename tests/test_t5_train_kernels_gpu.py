"""GPU: the T5 training kernels (csrc/t5_bwd.hip, the RB instantiations of the attention forward /
backward) against fp64 references on the kernels' own bf16 inputs.

Attention shapes: heads 4, B in {2, 3} with t5_refs.t5_batch's masks (full, half prefix, prefix of
5), L in {32, 50, 128, 156, 200, 512}: one block, a ragged block, NB = 4, NB = 5 with 8 waves, the
streamed kernels with a ragged second group, and the maximum.  Each (B, L) builds its inputs and its
fp64 autograd reference once (``_case``); the tests share them.
"""
import functools

import pytest

import attention_abi as abi
import t5_refs as tr
import t5_train_refs as ttr

pytestmark = pytest.mark.gpu

HEADS = 4
ATT_CASES = [(B, L) for L in (32, 50, 128, 156, 200, 512) for B in (2, 3)]
SEED, SITE, P = 13579, 6, 0.1


# ---------------------------------------------------------------------------------------------
# RMSNorm / feed-forward / embedding backwards
# ---------------------------------------------------------------------------------------------
def _rms_bwd(lib, dev, dy, x, gamma, eps, dres):
    import torch
    from denseretrievaltoolkits_amd import _native
    M, H = x.shape
    nb = int(lib.drt_rmsnorm_bwd_workspace(M, H))
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    dg = torch.empty(H, device=dev)
    _native.check(lib.drt_rmsnorm_bwd_bf16(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), eps, M, H,
                                           dres.data_ptr() if dres is not None else None, dx.data_ptr(),
                                           dg.data_ptr(), ws.data_ptr(), nb, _native.stream_ptr(dev)), "rmsnorm bwd")
    return dx, dg


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("M", [1, 150, 1024])
def test_rmsnorm_bwd_vs_fp64(dev, M, H, resid):
    """dx and dgamma of y = x rsqrt(mean x^2 + eps) gamma against fp64 autograd on the same bf16 x / dy
    (tolerances of test_encoder_bwd_gpu.test_layernorm_bwd_vs_torch); dgamma bit-equal across two runs."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    eps = 1e-6
    g = torch.Generator(device=dev).manual_seed(M + H)
    x = (2.0 * torch.randn(M, H, generator=g, device=dev) + 0.3).to(torch.bfloat16)
    gamma = 1.0 + 0.2 * torch.randn(H, generator=g, device=dev)
    dy = torch.randn(M, H, generator=g, device=dev).to(torch.bfloat16)
    dres = torch.randn(M, H, generator=g, device=dev).to(torch.bfloat16) if resid else None
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    (xd * torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + eps) * gd).backward(dy.double())
    want_dx = xd.grad + (dres.double() if resid else 0.0)
    dx, dg = _rms_bwd(lib, dev, dy, x, gamma, eps, dres)
    torch.testing.assert_close(dx.double(), want_dx, atol=3e-2, rtol=1e-2)
    torch.testing.assert_close(dg.double(), gd.grad, atol=1e-3 * max(1.0, M ** 0.5), rtol=1e-4)
    _, dg2 = _rms_bwd(lib, dev, dy, x, gamma, eps, dres)
    assert torch.equal(dg, dg2)


def _keep(dev, n, p):
    import torch
    return ttr.keep_mask(SEED, SITE, torch.arange(n, device=dev, dtype=torch.int64), p)


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("M,F", [(37, 520), (300, 1024)])
def test_gated_gelu_new_bwd_vs_fp64(dev, M, F, p):
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    g = torch.Generator(device=dev).manual_seed(M + F)
    X = (2.0 * torch.randn(M, 2 * F, generator=g, device=dev)).to(torch.bfloat16)
    dy = torch.randn(M, F, generator=g, device=dev).to(torch.bfloat16)
    dX = torch.empty_like(X)
    _native.check(lib.drt_gated_gelu_new_bwd_bf16(dy.data_ptr(), X.data_ptr(), M, F, p, SEED, SITE, dX.data_ptr(),
                                                  _native.stream_ptr(dev)), "gated gelu bwd")
    xd = X.double().requires_grad_(True)
    a, b = xd[:, :F], xd[:, F:]              # NewGELUActivation with autograd (t5_refs' one detaches)
    f = 0.5 * a * (1.0 + torch.tanh((2.0 / torch.pi) ** 0.5 * (a + 0.044715 * a.pow(3)))) * b
    up = dy.double()
    if p > 0:
        up = torch.where(_keep(dev, M * F, p).view(M, F), up / (1 - p), torch.zeros_like(up))
    f.backward(up)
    torch.testing.assert_close(dX.double(), xd.grad, atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("M,F", [(37, 520), (300, 1024)])
def test_relu_bwd_vs_fp64(dev, M, F, p):
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    g = torch.Generator(device=dev).manual_seed(M + F + 1)
    pre = torch.randn(M, F, generator=g, device=dev).to(torch.bfloat16)
    f = torch.relu(pre)
    dy = torch.randn(M, F, generator=g, device=dev).to(torch.bfloat16)
    dx = torch.empty_like(dy)
    _native.check(lib.drt_relu_bwd_bf16(dy.data_ptr(), f.data_ptr(), M * F, p, SEED, SITE, dx.data_ptr(),
                                        _native.stream_ptr(dev)), "relu bwd")
    up = dy.double()
    if p > 0:
        up = torch.where(_keep(dev, M * F, p).view(M, F), up / (1 - p), torch.zeros_like(up))
    want = up * (pre.double() > 0)
    torch.testing.assert_close(dx.double(), want, atol=1e-2, rtol=1e-2)
    assert bool((dx[pre <= 0] == 0).all())


def test_t5_embedding_bwd_vs_index_add(dev):
    """Scatter-add into shared.weight's gradient, with repeated ids and id 0 (T5 has no padding row)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, L, H, V = 3, 50, 256, 64                  # 150 tokens over 64 rows: every row repeats
    g = torch.Generator(device=dev).manual_seed(4)
    ids = torch.randint(0, V, (B, L), generator=g, device=dev)
    ids[0, :7] = 0
    ids[2, 10:] = 0
    d = torch.randn(B * L, H, generator=g, device=dev).to(torch.bfloat16)
    out = torch.zeros(V, H, device=dev)
    _native.check(lib.drt_t5_embedding_bwd(ids.data_ptr(), d.data_ptr(), B, L, H, V, out.data_ptr(),
                                           _native.stream_ptr(dev)), "t5 embedding bwd")
    want = torch.zeros(V, H, dtype=torch.float64, device=dev).index_add_(0, ids.flatten(), d.double())
    assert float(want[0].abs().max()) > 0
    # fp32 sums of <= 150 bf16 values in any order: |err| <= n 2^-24 sum|terms|
    bound = 150 * 2.0 ** -24 * torch.zeros(V, H, dtype=torch.float64, device=dev).index_add_(
        0, ids.flatten(), d.double().abs()) + 1e-12
    assert bool(((out.double() - want).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------
# attention with the relative-position bias: training forward and backward
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(B, L):
    """Inputs (CPU) and the fp64 references of one (B, L), built once."""
    import torch
    H = HEADS * 64
    g = torch.Generator().manual_seed(1000 * B + L)
    qkv = torch.randn(B * L, 3 * H, generator=g).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    table = 1.5 * torch.randn(HEADS, 2 * L - 1, generator=g)
    _, mask = tr.t5_batch(B, L, seed=L)
    dqkv, dtable, lse, ctx = ttr.attention_relbias_grads(qkv, dctx, mask, table, B, L, HEADS)
    return dict(qkv=qkv, dctx=dctx, table=table, mask=mask, dqkv=dqkv, dtable=dtable, lse=lse, ctx=ctx)


def _fwd(lib, dev, qkv, mask, table, B, L, p=0.0, bits=False):
    import torch
    from denseretrievaltoolkits_amd import _native
    H = HEADS * 64
    ctx = torch.empty(B * L, H, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, HEADS, L, device=dev)
    kb = torch.zeros(B, HEADS, L, (L + 31) // 32, dtype=torch.int32, device=dev) if bits else None
    _native.check(abi.forward(lib, qkv, ctx, B, L, HEADS, mask=mask, relbias=table, lse=lse, bits=kb, scale=1.0,
                              drop=(p, SEED, SITE)), "fwd")
    return ctx, lse, kb


def _bwd(lib, dev, qkv, ctx, dctx, lse, mask, table, kb, B, L, p=0.0):
    import torch
    from denseretrievaltoolkits_amd import _native
    dqkv = torch.zeros_like(qkv)
    if table is None:
        _native.check(abi.backward(lib, qkv, ctx, dctx, lse, dqkv, B, L, HEADS, mask=mask, bits=kb, scale=1.0,
                                   drop=(p, SEED, SITE)), "bwd")
        return dqkv, None
    nb = int(lib.drt_attention_backward_workspace(B, L, HEADS, 64, 1))
    ws = torch.empty((nb + 3) // 4, device=dev)
    dtable = torch.full((HEADS, 2 * L - 1), float("nan"), device=dev)
    _native.check(abi.backward(lib, qkv, ctx, dctx, lse, dqkv, B, L, HEADS, mask=mask, relbias=table, bits=kb,
                               scale=1.0, drop=(p, SEED, SITE), dtable=dtable, ws=ws, ws_bytes=nb), "relbias bwd")
    return dqkv, dtable


def _check_grads(tag, dqkv, dtable, want_dqkv, want_dtable):
    """The bounds of test_encoder_bwd_gpu.test_attention_bwd_vs_torch, on dQ, dK, dV and dtable each."""
    import torch
    H = HEADS * 64
    items = [(n, dqkv[:, sl].double().cpu(), want_dqkv[:, sl]) for n, sl in
             (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H)))]
    items.append(("dtable", dtable.double().cpu(), want_dtable))
    for name, got, want in items:
        assert bool(torch.isfinite(got).all()), (tag, name)
        err = (got - want).abs().max().item()
        cos = torch.nn.functional.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
        print(f"{tag} {name}: max err {err:.4g} (max |want| {want.abs().max().item():.4g}), cos {cos:.6f}")
        assert err <= 2e-2 * max(1.0, want.abs().max().item()), (tag, name, err, want.abs().max().item())
        assert cos > 0.999, (tag, name, cos)


@pytest.mark.parametrize("B,L", ATT_CASES)
def test_relbias_train_fwd(dev, B, L):
    """At p = 0 ctx has the bits of the inference call (no lse, no dropout arguments); lse against fp64."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(B, L)
    qkv, mask, table = c["qkv"].to(dev), c["mask"].to(dev), c["table"].to(dev)
    ctx, lse, _ = _fwd(lib, dev, qkv, mask, table, B, L)
    ctx0 = torch.empty_like(ctx)
    _native.check(abi.forward(lib, qkv, ctx0, B, L, HEADS, mask=mask, relbias=table, scale=1.0), "relbias fwd")
    torch.cuda.synchronize()
    assert torch.equal(ctx.view(torch.int16), ctx0.view(torch.int16))
    torch.testing.assert_close(lse.double().cpu(), c["lse"], atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("B,L", ATT_CASES)
def test_relbias_bwd_vs_fp64(dev, B, L):
    """dQKV and dtable against fp64 autograd on the same bf16 qkv / dctx (the kernel reads the
    forward's bf16 ctx)."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(B, L)
    qkv, mask, table, dctx = (c[k].to(dev) for k in ("qkv", "mask", "table", "dctx"))
    ctx, lse, _ = _fwd(lib, dev, qkv, mask, table, B, L)
    dqkv, dtable = _bwd(lib, dev, qkv, ctx, dctx, lse, mask, table, None, B, L)
    _check_grads(f"B={B} L={L}", dqkv, dtable, c["dqkv"], c["dtable"])


@pytest.mark.parametrize("B,L", [(3, 50), (3, 156), (3, 200)])
def test_dtable_is_zero_under_masked_and_padded_keys(dev, B, L):
    """Sequences 1.. of the batch (valid prefixes L / 2 and 5): a diagonal k - q = d >= L / 2 meets only
    masked keys (and, in the kernels' tiles, padding keys and padding rows) -- its entry is exactly 0."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(B, L)
    H = HEADS * 64
    qkv, dctx = c["qkv"][L:].to(dev).contiguous(), c["dctx"][L:].to(dev).contiguous()
    mask, table = c["mask"][1:].to(dev).contiguous(), c["table"].to(dev)
    ctx, lse, _ = _fwd(lib, dev, qkv, mask, table, B - 1, L)
    _, dtable = _bwd(lib, dev, qkv, ctx, dctx, lse, mask, table, None, B - 1, L)
    valid = int(mask.sum(1).max())
    assert valid == max(1, L // 2)
    tail = dtable[:, L - 1 + valid:]
    assert tail.numel() > 0 and bool((tail == 0).all())
    assert bool(torch.isfinite(dtable).all()) and float(dtable[:, :L - 1 + valid].abs().max()) > 0


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("B,L", ATT_CASES)
def test_zero_table_gives_the_plain_kernels_bits(dev, B, L, p):
    """With an all-zero table dQKV equals the bits of relbias = NULL: without
    dropout, on the keep-bits path and (L <= 160, where the plain kernel has it) on the hashed path."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(B, L)
    qkv, mask, dctx = (c[k].to(dev) for k in ("qkv", "mask", "dctx"))
    zero = torch.zeros(HEADS, 2 * L - 1, device=dev)
    ctx, lse, kb = _fwd(lib, dev, qkv, mask, None, B, L, p=p, bits=p > 0)
    ctx_z, lse_z, kb_z = _fwd(lib, dev, qkv, mask, zero, B, L, p=p, bits=p > 0)
    torch.cuda.synchronize()
    assert torch.equal(ctx.view(torch.int16), ctx_z.view(torch.int16)) and torch.equal(lse, lse_z)
    paths = [kb] if p > 0 else [None]
    if p > 0:
        assert torch.equal(kb, kb_z)
        if L <= 160:
            paths.append(None)          # hashed: the keep words drawn again
    for bits in paths:
        want, _ = _bwd(lib, dev, qkv, ctx, dctx, lse, mask, None, bits, B, L, p=p)
        got, dtable = _bwd(lib, dev, qkv, ctx, dctx, lse, mask, zero, bits, B, L, p=p)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("bits" if bits is not None else "hash")
        assert bool(torch.isfinite(dtable).all())


@pytest.mark.parametrize("B,L", ATT_CASES)
def test_relbias_bwd_with_dropout(dev, B, L):
    """p = 0.1: the keep-bits path equals the hashed path bit for bit (L <= 160), and the result matches
    the fp64 reference under the same keep mask within the same bounds."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(B, L)
    qkv, mask, table, dctx = (c[k].to(dev) for k in ("qkv", "mask", "table", "dctx"))
    ctx, lse, kb = _fwd(lib, dev, qkv, mask, table, B, L, p=P, bits=True)
    dqkv, dtable = _bwd(lib, dev, qkv, ctx, dctx, lse, mask, table, kb, B, L, p=P)
    if L <= 160:
        dqkv_h, dtable_h = _bwd(lib, dev, qkv, ctx, dctx, lse, mask, table, None, B, L, p=P)
        torch.cuda.synchronize()
        assert torch.equal(dqkv.view(torch.int16), dqkv_h.view(torch.int16))
        # dtable: the same fp32 dS on both paths, summed by LDS atomics in hardware order: per entry
        # <= 160 terms per (sequence, head), so a reordering moves it by <= 160 * 2^-24 ~ 1e-5 of the
        # terms' absolute sum
        torch.testing.assert_close(dtable_h, dtable, atol=1e-4 * max(1.0, float(dtable.abs().max())), rtol=1e-5)
    keep = ttr.attn_keep_mask(SEED, SITE, B, HEADS, L, P, torch.device("cpu"))
    want_dqkv, want_dtable, _, want_ctx = ttr.attention_relbias_grads(c["qkv"], c["dctx"], c["mask"], c["table"], B, L,
                                                                      HEADS, keep=keep, p=P)
    # the forward drew the reference's mask: ctx agrees to bf16 rounding
    err = (ctx.double().cpu() - want_ctx).abs().max().item()
    assert err <= 2e-2 * max(1.0, want_ctx.abs().max().item()), err
    _check_grads(f"B={B} L={L} p={P}", dqkv, dtable, want_dqkv, want_dtable)

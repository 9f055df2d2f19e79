"""The encoder backward kernels (csrc/encoder_bwd.hip) against the plain fp64 references of
tests/encoder_bwd_refs.py, through the native entry points: the attention backward at every NB
instantiation of the whole-sequence kernel and at the 128-row group boundaries of the streamed pair,
plain, with keep bits and with a relative-position bias, under five mask kinds with poisoned masked
keys; a sequence with every key masked (the contract of include/drt.h); run-to-run determinism; the
LayerNorm backward at every H / 64 instantiation either side of a full grid pass.

Bounds (derived in tests/encoder_bwd_cases.py, shown reachable by tests/test_encoder_bwd_refs_cpu.py):
elementwise, u = 2^-8, dV <= 2.5 u A_V, dQ / dK <= 3.5 u A, dtable <= 1.5 u A_T + 1e-6, an exact 0
wherever A = 0 (masked keys' dK and dV, a sequence with every key masked).  The backward is fed
ctx = bf16(O_ref) and lse = fp32(lse_ref), so a failure belongs to the backward; one test per kernel
family runs it on the forward kernel's own ctx, lse and keep bits (dQ / dK <= 5 u A there).
"""
import pytest

import attention_abi as abi
import encoder_bwd_cases as bc
import encoder_bwd_refs as br

pytestmark = pytest.mark.gpu

B_ATT = 3
ATT_LS = (1, 31, 32, 33, 64, 65, 96, 128, 129, 159, 160, 161, 255, 256, 257, 300, 384, 385, 512)
ATT_SHAPES = [(L, 4) for L in ATT_LS] + [(L, 12) for L in (33, 160, 161, 512)] + [(L, 1) for L in (33, 161)]
RB_LS = (32, 50, 128, 160, 161, 300, 512)
# (L, heads, variant): plain and keep bits at p = 0.1 everywhere; p = 0.5 with one query row whose every
# live key is dropped at L = 33, 161; the relative-position bias (scale = 1, q and k x 0.35, table ~ 2 randn)
ATT_CASES = ([(L, h, v) for L, h in ATT_SHAPES for v in ("plain", "keep01")] +
             [(L, h, "keep05") for L, h in ATT_SHAPES if L in (33, 161)] +
             [(L, 4, v) for L in RB_LS for v in ("relbias", "relbias_keep01")])
VARIANT_P = {"plain": 0.0, "keep01": 0.1, "keep05": 0.5, "relbias": 0.0, "relbias_keep01": 0.1}
SEED, SITE = 1234, 7     # unused by the kernels when drop_bits is given


def _batch(L, heads):
    """B = 3; 2 at L = 512 with 12 heads, where the fp64 reference of 3 sequences takes too long."""
    return 2 if (L, heads) == (512, 12) else B_ATT


def _case(tag, data, variant, L, heads, mask_kind, B=B_ATT, dead=None, zero_dead_dctx=False):
    """One attention backward problem on the CPU: inputs, keep mask, table and the fp64 reference."""
    import torch
    rb = variant.startswith("relbias")
    p = VARIANT_P[variant]
    scale, qk = (1.0, 0.35) if rb else (0.125, 1.0)
    g = bc.gen(tag, L, heads, data, variant, mask_kind)
    mask = bc.make_mask(mask_kind, B, L, g)
    if dead is not None:
        mask[dead] = 0
    qkv, dctx = bc.make_qkv_dctx(data, B, L, heads, mask, g, keep_v=() if dead is None else (dead,), qk_scale=qk)
    if zero_dead_dctx:
        dctx.reshape(B, L, -1)[dead] = 0
    table = 2 * torch.randn(heads, 2 * L - 1, generator=g) if rb else None
    keep = bc.make_keep(B, L, heads, p, mask, g, starve=p == 0.5) if p > 0 else None
    ref = br.attention_bwd_ref(qkv, dctx, mask, B, L, heads, scale, relbias=table, keep=keep, p=p)
    return dict(qkv=qkv, dctx=dctx, mask=mask, table=table, keep=keep, p=p, scale=scale, ref=ref, B=B, L=L, heads=heads)


def _run_bwd(lib, dev, c, *, ctx=None, lse=None, bits=None, mask="case", want_dbias=False):
    """drt_attention_backward_bf16 on case c; ctx / lse default to bf16(O_ref) / fp32(lse_ref), the keep
    bits to the packed keep mask.  Outputs start as NaN.  Returns CPU (dqkv, dtable or None, dbias or
    None, the partial-sum rows left in ws or None)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    B, L, heads = c["B"], c["L"], c["heads"]
    H = heads * 64
    ref = c["ref"]
    to = lambda t: None if t is None else t.to(dev)   # noqa: E731
    ctx = to(ref.O.to(torch.bfloat16)) if ctx is None else ctx
    lse = to(ref.lse.float()) if lse is None else lse
    if bits is None and c["keep"] is not None:
        bits = to(bc.pack_bits(c["keep"]))
    mask = c["mask"] if isinstance(mask, str) else mask
    table = to(c["table"])
    dqkv = torch.full((B * L, 3 * H), float("nan"), dtype=torch.bfloat16, device=dev)
    dtable = dbias = ws = None
    nb = 0
    if table is not None:
        dtable = torch.full((heads, 2 * L - 1), float("nan"), device=dev)
        nb = int(lib.drt_attention_backward_workspace(B, L, heads, 64, 1))
    elif want_dbias:
        dbias = torch.full((3 * H,), float("nan"), device=dev)
        nb = int(lib.drt_attention_backward_workspace(B, L, heads, 64, 0))
    if nb:
        ws = torch.full(((nb + 3) // 4,), float("nan"), device=dev)
    _native.check(abi.backward(lib, to(c["qkv"]), ctx, to(c["dctx"]), lse, dqkv, B, L, heads, mask=to(mask),
                               relbias=table, bits=bits, scale=c["scale"], drop=(c["p"], SEED, SITE), dbias=dbias,
                               dtable=dtable, ws=ws, ws_bytes=nb), "attention backward")
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()   # noqa: E731
    return cpu(dqkv), cpu(dtable), cpu(dbias), cpu(ws)


def _dbias_problems(dqkv, dqkv_b, dbias):
    """The existing rule: dqkv bit-equal with and without dbias, dbias within 1e-5 sum|dqkv| + 1e-6 of
    the fp64 column sums of the stored dqkv."""
    import torch
    bad = []
    if not torch.equal(dqkv.view(torch.int16), dqkv_b.view(torch.int16)):
        bad.append("dqkv differs with dbias")
    d = dqkv.double()
    if not ((dbias.double() - d.sum(0)).abs() <= 1e-5 * d.abs().sum(0) + 1e-6).all():
        bad.append("dbias off the column sums of dqkv")
    return bad


@pytest.mark.parametrize("data", bc.DATA_KINDS)
@pytest.mark.parametrize("L,heads,variant", ATT_CASES, ids=[f"{L}-{h}-{v}" for L, h, v in ATT_CASES])
def test_attention_bwd_vs_fp64(dev, L, heads, variant, data):
    """dQ, dK, dV (and dtable) elementwise within their bounds of fp64 under every mask kind, every
    element written and finite, exact zeros where A = 0; without a table, dbias by the existing rule.

    Measured on an MI355X (worst over all cases; L <= 160 / L > 160): dQ 1.441 / 1.534, dK 1.408 / 1.526,
    dV 1.871 / 1.922, dtable 0.262 / 0.331 u A; recorded in the "Attention backward vs
    fp64" paragraph of DESIGN.md."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B = _batch(L, heads)
    worst, bad = {}, []
    for mk in bc.MASK_KINDS:
        c = _case("bwd", data, variant, L, heads, mk, B=B)
        dqkv, dtable, _, _ = _run_bwd(lib, dev, c)
        ratios = bc.attention_ratios(dqkv, dtable, c["ref"])
        for n, r in ratios.items():
            worst[n] = max(worst.get(n, 0.0), r)
        bad += [f"{mk}: {t}" for t in bc.over_bounds(ratios)]
        if c["table"] is None:
            dqkv_b, _, dbias, _ = _run_bwd(lib, dev, c, want_dbias=True)
            bad += [f"{mk}: {t}" for t in _dbias_problems(dqkv, dqkv_b, dbias)]
    print(f"attention bwd L={L} heads={heads} {variant} {data}: worst u A " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert not bad, f"L={L} heads={heads} {variant} {data}: " + "; ".join(bad)


def _unpack_bits(words, L):
    """bool [B, heads, L, L] from drop_bits [B, heads, L, ceil(L / 32)]."""
    import torch
    w = words.to(torch.int64) & 0xFFFFFFFF
    k = torch.arange(L)
    return ((w[..., k >> 5] >> (k & 31)) & 1).bool()


@pytest.mark.parametrize("L", [100, 160, 300])
def test_attention_bwd_on_the_forward_kernels_outputs(dev, L):
    """One run per kernel family (NB = 4, the 8-wave NB = 5, the streamed pair) on the forward kernel's
    own ctx, lse and keep bits at p = 0.1, without and with a relative-position bias, under every mask
    kind.  D then carries the forward's 2.5 u instead of u: dQ, dK <= 5 u A, dtable <= 3 u A_T + 1e-6.

    Measured on an MI355X: dQ 0.557, dK 0.318, dV 1.314, dtable 0.276 u A."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, heads, p = B_ATT, 4, 0.1
    H = heads * 64
    worst, bad = {}, []
    for variant in ("keep01", "relbias_keep01"):
        for mk in bc.MASK_KINDS:
            c = _case("fwd-fed", "gauss", variant, L, heads, mk)
            qd = c["qkv"].to(dev)
            md = None if c["mask"] is None else c["mask"].to(dev)
            td = None if c["table"] is None else c["table"].to(dev)
            ctx = torch.full((B * L, H), float("nan"), dtype=torch.bfloat16, device=dev)
            lse = torch.full((B, heads, L), float("nan"), device=dev)
            bits = torch.zeros(B, heads, L, (L + 31) // 32, dtype=torch.int32, device=dev)
            _native.check(abi.forward(lib, qd, ctx, B, L, heads, mask=md, relbias=td, lse=lse, bits=bits, scale=c["scale"],
                                      drop=(p, SEED, SITE)), "attention forward")
            torch.cuda.synchronize()
            c["keep"] = _unpack_bits(bits.cpu(), L)
            c["ref"] = br.attention_bwd_ref(c["qkv"], c["dctx"], c["mask"], B, L, heads, c["scale"], relbias=c["table"],
                                            keep=c["keep"], p=p)
            dqkv, dtable, _, _ = _run_bwd(lib, dev, c, ctx=ctx, lse=lse, bits=bits)
            ratios = bc.attention_ratios(dqkv, dtable, c["ref"])
            for n, r in ratios.items():
                worst[n] = max(worst.get(n, 0.0), r)
            bad += [f"{variant} {mk}: {t}" for t in bc.over_bounds(ratios, dqk=bc.BOUND_DQK_FWD, dt=bc.BOUND_DT_FWD)]
    print(f"attention bwd on the forward's outputs L={L}: worst u A " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert not bad, f"L={L}: " + "; ".join(bad)


@pytest.mark.parametrize("zero_dctx", [False, True], ids=["dctx", "dctx0"])
@pytest.mark.parametrize("variant", ["plain", "keep01", "relbias"])
@pytest.mark.parametrize("L", [33, 160, 161, 300])
def test_attention_bwd_fully_masked_sequence(dev, L, variant, zero_dctx):
    """The middle sequence of three has every key masked and keeps its own V (include/drt.h): its dQ and
    dK rows are exact zeros, it adds exact zeros to dtable, its dV = sum_q keep dO_q / (L (1 - p)) within
    the dV bound, everything is finite, dctx = 0 on it gives all-zero rows; the other sequences' rows and
    their partial sums of dbias keep the bits they have when that sequence gets an all-ones mask."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    B, heads, dead = B_ATT, 4, 1
    H = heads * 64
    c = _case("dead", "gauss", variant, L, heads, "prefix", dead=dead, zero_dead_dctx=zero_dctx)
    ref = c["ref"]
    dqkv, dtable, dbias, ws = _run_bwd(lib, dev, c, want_dbias=True)
    assert torch.isfinite(dqkv.float()).all()
    ratios = bc.attention_ratios(dqkv, dtable, ref)
    print(f"fully masked L={L} {variant} dctx0={zero_dctx}: u A " + " ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert not bc.over_bounds(ratios), bc.over_bounds(ratios)
    rows = dqkv.reshape(B, L, 3 * H)
    assert (rows[dead, :, :2 * H] == 0).all()
    want_dv = ref.dqkv.reshape(B, L, 3 * H)[dead, :, 2 * H:]
    if zero_dctx:
        assert (rows[dead] == 0).all() and (want_dv == 0).all()
    else:
        assert float(want_dv.abs().max()) > 0
    live = [0, 2]
    G = (L + 127) // 128 if L > 160 else 1           # rows of partial sums per sequence
    if dtable is not None:
        assert torch.isfinite(dtable).all()
        n = heads * (2 * L - 1)
        part = ws[:B * G * n].reshape(B, G * n)
        assert (part[dead] == 0).all(), "the dead sequence's diagonal sums are not exact zeros"
    else:
        assert not _dbias_problems(dqkv, dqkv, dbias)
    # the same call with an all-ones mask on that sequence (and that mask's own ctx / lse for it)
    mask2 = c["mask"].clone()
    mask2[dead] = 1
    ref2 = br.attention_bwd_ref(c["qkv"], c["dctx"], mask2, B, L, heads, c["scale"], relbias=c["table"], keep=c["keep"], p=c["p"])
    dqkv2, _, _, ws2 = _run_bwd(lib, dev, c, ctx=ref2.O.to(torch.bfloat16).to(dev), lse=ref2.lse.float().to(dev),
                                mask=mask2, want_dbias=True)
    rows2 = dqkv2.reshape(B, L, 3 * H)
    assert torch.equal(rows[live].view(torch.int16), rows2[live].view(torch.int16))
    if dtable is None:
        n = 3 * H
        p1, p2 = ws[:B * G * n].reshape(B, G * n), ws2[:B * G * n].reshape(B, G * n)
        assert torch.equal(p1[live], p2[live])


@pytest.mark.parametrize("variant", ["plain", "relbias_keep01"])
@pytest.mark.parametrize("L", [100, 160, 300])
def test_attention_bwd_is_bit_reproducible(dev, L, variant):
    """Two runs of each kernel family give bit-equal dqkv (the relative-bias reads of the 8-wave NB = 5
    instance once did not: the comment above attention_bwd_rk_kernel)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case("det", "gauss", variant, L, 12, "prefix")
    a, _, _, _ = _run_bwd(lib, dev, c)
    b, _, _, _ = _run_bwd(lib, dev, c)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------------------------
# drt_layernorm_backward_bf16
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dres", [False, True], ids=["nores", "dres"])
@pytest.mark.parametrize("M", [1, 3, 4095, 4097])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_layernorm_bwd_vs_fp64(dev, H, M, with_dres):
    """dx within 1.5 u A_LN + 1e-7 of fp64 (one bf16 rounding plus slack), dgamma / dbeta within
    1e-5 sum|terms| + 1e-6 of the fp64 sums, dsum within the same of the fp64 column sums of the stored
    dx, and dx / dgamma / dbeta bit-equal with and without dsum.  M is one row either side of a full
    grid pass (1024 blocks x 4 waves).  Every third row has mean 30 and std 0.5 (its variance cancels),
    row 0 of dy is all zero when M > 1.

    Measured on an MI355X: dx 0.896 u A_LN; dgamma 0.115, dbeta 0.001, dsum 0.001 of their bounds (dgamma was at
    2.3 on a mean-30 row before the kernel shifted the row by its first element)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    g = bc.gen("ln", H, M, with_dres)
    x = 2.0 * torch.randn(M, H, generator=g) + 0.3
    x[1::3] = 30 + 0.5 * torch.randn(x[1::3].shape, generator=g)
    x = x.to(torch.bfloat16)
    dy = torch.randn(M, H, generator=g)
    if M > 1:
        dy[0] = 0
    dy = dy.to(torch.bfloat16)
    gamma = 1.0 + 0.2 * torch.randn(H, generator=g)
    dres = torch.randn(M, H, generator=g).to(torch.bfloat16) if with_dres else None
    eps = 1e-12
    ref = br.layernorm_bwd_ref(dy, x, gamma, eps, dres)
    xd, dyd, gd = x.to(dev), dy.to(dev), gamma.to(dev)
    rd = None if dres is None else dres.to(dev)
    nb = int(lib.drt_layernorm_bwd_workspace(M, H))
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
    outs = []
    for with_dsum in (False, True):
        dx = torch.full((M + 4, H), float("nan"), dtype=torch.bfloat16, device=dev)   # 4 guard rows
        dgam, dbet = torch.full((H,), float("nan"), device=dev), torch.full((H,), float("nan"), device=dev)
        dsum = torch.full((H,), float("nan"), device=dev) if with_dsum else None
        _native.check(lib.drt_layernorm_backward_bf16(dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), eps, M, H,
                                                      None if rd is None else rd.data_ptr(), dx.data_ptr(), None, 0.0,
                                                      0, 0, dgam.data_ptr(), dbet.data_ptr(),
                                                      None if dsum is None else dsum.data_ptr(), ws.data_ptr(), nb,
                                                      _native.stream_ptr(dev)), "layernorm backward")
        torch.cuda.synchronize()
        outs.append((dx.cpu(), dgam.cpu(), dbet.cpu(), None if dsum is None else dsum.cpu()))
    (dx, dgam, dbet, _), (dx1, dgam1, dbet1, dsum) = outs
    tag = f"H={H} M={M} dres={with_dres}"
    assert torch.isnan(dx[M:].float()).all() and torch.isnan(dx1[M:].float()).all(), f"{tag}: rows past M written"
    dx, dx1 = dx[:M], dx1[:M]
    assert torch.equal(dx.view(torch.int16), dx1.view(torch.int16)), f"{tag}: dx differs with dsum"
    assert torch.equal(dgam, dgam1) and torch.equal(dbet, dbet1), f"{tag}: dgamma / dbeta differ with dsum"
    ratio = br.bound_ratio(dx, ref.dx, ref.A_LN, 1e-7)

    def sum_ratio(got, want, terms_abs):   # |err| / (1e-5 sum|terms| + 1e-6)
        if not torch.isfinite(got).all():
            return float("inf")
        return float(((got.double() - want).abs() / (1e-5 * terms_abs + 1e-6)).max())

    rg = sum_ratio(dgam, ref.dgamma, ref.dgamma_abs)
    rb = sum_ratio(dbet, ref.dbeta, ref.dbeta_abs)
    rs = sum_ratio(dsum, dx.double().sum(0), dx.double().abs().sum(0))
    print(f"layernorm bwd {tag}: dx {ratio:.3f} u A, dgamma {rg:.3f} dbeta {rb:.3f} dsum {rs:.3f} of their bounds")
    assert ratio <= 1.5, f"{tag}: dx error {ratio:.3f} u A_LN > 1.5 u A_LN"
    assert rg <= 1 and rb <= 1 and rs <= 1, f"{tag}: dgamma {rg:.3f} dbeta {rb:.3f} dsum {rs:.3f} of their bounds"
    if M > 1 and not with_dres:
        assert (dx[0] == 0).all(), f"{tag}: dy = 0 gives dx = 0"

"""The kernels of padding-free training through their native entry points: the varlen attention
backward and training forward over one packed batch that mixes every length class, against the plain
fp64 references of tests/encoder_bwd_refs.py (per sequence) with the bounds of
tests/encoder_bwd_cases.py; bit for bit against the padded kernels where the contract says so
(include/drt.h, "Padding-free BERT training"); the pack copy and the packed embedding with its pre-LN sum.

Bounds: u = 2^-8, dV <= 2.5 u A_V, dQ / dK <= 3.5 u A, fed ctx = bf16(O_ref) and lse = fp32(lse_ref);
5 u A for dQ / dK on the varlen forward's own ctx, lse and keep bits.
"""
import random

import pytest

import attention_abi as abi
import encoder_bwd_cases as bc
import encoder_bwd_refs as br

pytestmark = pytest.mark.gpu

LENS = (1, 31, 32, 33, 64, 65, 96, 128, 129, 159, 160)
L_PAD = 160
W = 5              # keep words per query of the batch: ceil(160 / 32)
GUARD = 8          # NaN rows before row 0 and after row T of every output
VARIANT_P = {"plain": 0.0, "keep01": 0.1, "keep05": 0.5}
SEED, SITE = 4321, 9
SCALE = 0.125

_CASES = {}


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def _pad_words(words, w):
    """[heads, n, ceil(n / 32)] -> [heads, n, w] (zero words behind)."""
    import torch
    out = torch.zeros(words.shape[0], words.shape[1], w, dtype=torch.int32)
    out[:, :, :words.shape[2]] = words
    return out


def _case(heads, data, variant, keeps=None, tag="packed-train"):
    """The one packed batch of (heads, data, variant), built once and left unchanged: per-sequence fp64
    references, the packed qkv / dctx / ctx = bf16(O_ref) / lse = fp32(lse_ref) / keep words.  ``keeps``
    (bool [heads, n, n] per sequence) replaces the drawn keep masks (not cached)."""
    import torch
    key = (heads, data, variant, tag)
    if keeps is None and key in _CASES:
        return _CASES[key]
    lens = list(LENS)
    random.Random(11 + heads).shuffle(lens)
    H = heads * 64
    p = VARIANT_P[variant]
    seqs = []
    for b, n in enumerate(lens):
        g = bc.gen(tag, heads, data, b, n)
        qkv_b, dctx_b = bc.make_qkv_dctx(data, 1, n, heads, None, g)
        qkv_b = qkv_b.float()
        qkv_b[:, 2 * H:] *= 4.0 ** (b % 6)          # exact in bf16: a neighbour's V is far off the bound
        qkv_b = qkv_b.to(torch.bfloat16)
        keep = None
        if p > 0:
            gk = bc.gen(tag, "keep", heads, variant, b, n)
            keep = bc.make_keep(1, n, heads, p, None, gk, starve=p == 0.5 and n in (33, 129))
            if keeps is not None:
                keep = keeps[b][None]
        ref = br.attention_bwd_ref(qkv_b, dctx_b, None, 1, n, heads, SCALE, keep=keep, p=p)
        seqs.append(dict(n=n, qkv=qkv_b, dctx=dctx_b, keep=keep, ref=ref))
    c = dict(heads=heads, p=p, lens=lens, cu=_cu(lens), seqs=seqs,
             qkv=torch.cat([s["qkv"] for s in seqs], 0), dctx=torch.cat([s["dctx"] for s in seqs], 0),
             ctx=torch.cat([s["ref"].O.to(torch.bfloat16) for s in seqs], 0),
             lse=torch.cat([s["ref"].lse[0].float() for s in seqs], 1).contiguous(),          # [heads][T]
             bits=None if p == 0 else torch.cat([_pad_words(bc.pack_bits(s["keep"])[0], W) for s in seqs], 1).contiguous())
    if keeps is None:
        _CASES[key] = c
    return c


def _run_bwd(dev, c, seq_ids, n_seqs, max_len, *, want_dsum=False, ctx=None, lse=None, bits="case", cu=None,
             l_pad=L_PAD):
    """drt_attention_varlen_backward_bf16 on the packed batch; outputs start as NaN.  Returns CPU
    (dqkv with its guard rows, dsum [B, 3H] or None)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads = c["heads"]
    H = heads * 64
    cu = c["cu"] if cu is None else cu
    T, B = c["qkv"].shape[0], len(cu) - 1
    to = lambda t: None if t is None else t.to(dev)   # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    qd, dod = to(c["qkv"]), to(c["dctx"])
    ctxd = to(c["ctx"]) if ctx is None else ctx
    lsed = to(c["lse"]) if lse is None else lse
    bitsd = to(c["bits"]) if isinstance(bits, str) else bits
    cud = torch.tensor(cu, dtype=torch.int32, device=dev)
    sd = None if seq_ids is None else torch.tensor(seq_ids, dtype=torch.int32, device=dev)
    buf = torch.full((GUARD + T + GUARD, 3 * H), float("nan"), dtype=torch.bfloat16, device=dev)
    dsum = torch.full((B, 3 * H), float("nan"), device=dev) if want_dsum else None
    _native.check(lib.drt_attention_varlen_backward_bf16(
        qd.data_ptr(), ctxd.data_ptr(), dod.data_ptr(), lsed.data_ptr(), cud.data_ptr(), ptr(sd), n_seqs, max_len,
        l_pad, T, W, ptr(bitsd), buf[GUARD:].data_ptr(), ptr(dsum), heads, 64, SCALE, c["p"], SEED, SITE,
        _native.stream_ptr(dev)), "varlen attention backward")
    torch.cuda.synchronize()
    return buf.cpu(), None if dsum is None else dsum.cpu()


def _check_rows(buf, c, listed, tag, dqk=bc.BOUND_DQK):
    """Listed sequences within the bounds of their own fp64 reference, every other row (guards
    included) still NaN.  Returns the worst ratios."""
    import torch
    cu, T = c["cu"], c["qkv"].shape[0]
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + T:].float()).all(), \
        f"{tag}: guard rows written"
    dqkv = buf[GUARD:GUARD + T]
    worst, bad = {}, []
    for b, s in enumerate(c["seqs"]):
        rows = slice(cu[b], cu[b + 1])
        if b not in listed:
            assert torch.isnan(dqkv[rows].float()).all(), f"{tag}: unlisted sequence {b} (len {s['n']}) written"
            continue
        ratios = bc.attention_ratios(dqkv[rows], None, s["ref"])
        for n, r in ratios.items():
            worst[n] = max(worst.get(n, 0.0), r)
        bad += [f"sequence {b} (len {s['n']}): {t}" for t in bc.over_bounds(ratios, dqk=dqk)]
    assert not bad, f"{tag}: " + "; ".join(bad)
    return worst


def _classes(lens):
    out = {}
    for b, n in enumerate(lens):
        out.setdefault((n + 31) // 32, []).append(b)
    return out


def _colsum(dev, dsum):
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    x = dsum.to(dev)
    M, N = x.shape
    out = torch.full((N,), float("nan"), device=dev)
    nb = int(lib.drt_colsum_workspace(M, N))
    ws = torch.empty((nb + 3) // 4 + 1, device=dev)
    _native.check(lib.drt_colsum_f32(x.data_ptr(), M, N, out.data_ptr(), ws.data_ptr(), nb, _native.stream_ptr(dev)),
                  "drt_colsum_f32")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("data", bc.DATA_KINDS)
@pytest.mark.parametrize("variant", ["plain", "keep01", "keep05"])
@pytest.mark.parametrize("heads", [4, 12])
def test_varlen_bwd_vs_fp64(dev, heads, variant, data):
    """One packed batch of lengths 1 .. 160 in shuffled order, each sequence's dQ, dK, dV within the
    bounds of the fp64 reference of that sequence alone: the whole batch in one launch (max_len 160),
    one launch per length class, a subset with a smaller max_len (every other row still NaN), and
    short sequences inside classes 4 and 5 (row blocks without a token).  In the one-launch run: dqkv
    bit-equal with and without dsum and between two runs, and drt_colsum_f32 of dsum by the existing
    dbias rule.

    Measured on an MI355X (worst over all cases and launches): dQ 1.488, dK 1.295, dV 1.893 u A."""
    import torch
    c = _case(heads, data, variant)
    lens, B = c["lens"], len(c["lens"])
    T = c["qkv"].shape[0]
    tag = f"heads={heads} {variant} {data}"
    buf, _ = _run_bwd(dev, c, None, B, 160)
    worst = _check_rows(buf, c, set(range(B)), f"{tag} one launch")
    print(f"varlen bwd {tag} one launch: worst u A " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    buf2, dsum = _run_bwd(dev, c, None, B, 160, want_dsum=True)
    assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16)), f"{tag}: dqkv differs with dsum / between runs"
    dqkv = buf[GUARD:GUARD + T]
    d = dqkv.double()
    for b in range(B):   # row b of dsum: the column sums of sequence b's stored rows
        rows = d[c["cu"][b]:c["cu"][b + 1]]
        assert ((dsum[b].double() - rows.sum(0)).abs() <= 1e-5 * rows.abs().sum(0) + 1e-6).all(), f"{tag}: dsum row {b}"
    dbias = _colsum(dev, dsum)
    assert ((dbias.double() - d.sum(0)).abs() <= 1e-5 * d.abs().sum(0) + 1e-6).all(), f"{tag}: dbias"
    # one launch per length class, as PackingPlan.classes() issues them; dsum rows of the others untouched
    whole = torch.full((B, 3 * heads * 64), float("nan"))
    for nb, ids in sorted(_classes(lens).items()):
        ml = max(lens[b] for b in ids)
        bufc, dsc = _run_bwd(dev, c, ids, len(ids), ml, want_dsum=True)
        wc = _check_rows(bufc, c, set(ids), f"{tag} class {nb} max_len {ml}")
        print(f"varlen bwd {tag} class {nb} (lens {[lens[b] for b in ids]}): worst u A "
              + " ".join(f"{n} {r:.3f}" for n, r in wc.items()))
        others = [b for b in range(B) if b not in ids]
        assert torch.isnan(dsc[others]).all(), f"{tag} class {nb}: dsum rows of unlisted sequences written"
        whole[ids] = dsc[ids]
        for b in ids:   # a sequence at its own class: the bits of the wide launch (skipped blocks add exact zeros)
            rows = slice(GUARD + c["cu"][b], GUARD + c["cu"][b + 1])
            assert torch.equal(bufc[rows].view(torch.int16), buf[rows].view(torch.int16)), \
                f"{tag}: sequence {b} differs between its class launch and the one launch"
    assert torch.equal(whole, dsum), f"{tag}: dsum differs between the launch policies"
    for ml, pick in ((64, (1, 33, 64)), (128, (1, 33, 96)), (160, (1, 31, 64, 96, 129, 160))):
        ids = [b for b, n in enumerate(lens) if n in pick]
        bufs, _ = _run_bwd(dev, c, ids, len(ids), ml)
        _check_rows(bufs, c, set(ids), f"{tag} subset max_len {ml}")


def _run_fwd(dev, c, launches, p, *, want_lse=True, want_bits=True, inference=False):
    """The varlen training forward (or the inference entry) over ``launches`` = [(seq_ids, n, max_len)].
    Returns device (ctx with guard rows, lse [heads, GUARD + T + GUARD], bits [heads, T, W])."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads = c["heads"]
    H = heads * 64
    T = c["qkv"].shape[0]
    qd = c["qkv"].to(dev)
    cud = torch.tensor(c["cu"], dtype=torch.int32, device=dev)
    ctx = torch.full((GUARD + T + GUARD, H), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((heads, T), float("nan"), device=dev) if want_lse else None
    bits = torch.zeros((heads, T, W), dtype=torch.int32, device=dev) if (want_bits and p > 0) else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    s = _native.stream_ptr(dev)
    for ids, n, ml in launches:
        sd = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev)
        if inference:
            rc = lib.drt_attention_varlen_forward_bf16(qd.data_ptr(), cud.data_ptr(), ptr(sd), n, ml,
                                                       ctx[GUARD:].data_ptr(), heads, 64, SCALE, s)
        else:
            rc = lib.drt_attention_varlen_train_forward_bf16(qd.data_ptr(), cud.data_ptr(), ptr(sd), n, ml, L_PAD, T, W,
                                                             ctx[GUARD:].data_ptr(), ptr(lse), ptr(bits), heads, 64,
                                                             SCALE, p, SEED, SITE, s)
        _native.check(rc, "varlen attention forward")
        torch.cuda.synchronize()
    return ctx, lse, bits


def _unpack_words(words, n):
    """bool [heads, n, n] from keep words [heads, n, >= ceil(n / 32)]."""
    import torch
    w = words.to(torch.int64) & 0xFFFFFFFF
    k = torch.arange(n)
    return ((w[..., k >> 5] >> (k & 31)) & 1).bool()


@pytest.mark.parametrize("heads", [4, 12])
def test_varlen_train_forward(dev, heads):
    """lse within atol 1e-3, rtol 1e-4 of the reference; at p = 0 the ctx bits of
    drt_attention_varlen_forward_bf16, with and without lse, in one launch and per class; at p = 0.1
    the keep bits of every real (q, key) equal those of drt_attention_forward_bf16 on the padded batch
    with the same (p, seed, site) and L = L_pad, whatever the launch policy."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(heads, "gauss", "plain")
    lens, cu, B = c["lens"], c["cu"], len(c["lens"])
    T, H = c["qkv"].shape[0], heads * 64
    one = [(None, B, 160)]
    per_class = [(ids, len(ids), max(lens[b] for b in ids)) for _, ids in sorted(_classes(lens).items())]
    want, _, _ = _run_fwd(dev, c, one, 0.0, inference=True)
    for tag, launches in (("one launch", one), ("per class", per_class)):
        ctx, lse, _ = _run_fwd(dev, c, launches, 0.0)
        ctx0, _, _ = _run_fwd(dev, c, launches, 0.0, want_lse=False)
        assert torch.equal(ctx.view(torch.int16), want.view(torch.int16)), f"{tag}: ctx bits differ from the inference entry"
        assert torch.equal(ctx.view(torch.int16), ctx0.view(torch.int16)), f"{tag}: ctx differs without lse"
        assert torch.isnan(ctx[:GUARD].float()).all() and torch.isnan(ctx[GUARD + T:].float()).all()
        torch.testing.assert_close(lse.cpu(), c["lse"], atol=1e-3, rtol=1e-4)
    # the padded batch [B, L_PAD]: zeros at the pads, prefix mask
    p = 0.1
    padded = torch.zeros(B, L_PAD, 3 * H, dtype=torch.bfloat16)
    mask = torch.zeros(B, L_PAD, dtype=torch.int64)
    for b, n in enumerate(lens):
        padded[b, :n] = c["qkv"][cu[b]:cu[b + 1]]
        mask[b, :n] = 1
    pq, pm = padded.reshape(B * L_PAD, 3 * H).to(dev), mask.to(dev)
    pctx = torch.empty(B * L_PAD, H, dtype=torch.bfloat16, device=dev)
    pbits = torch.zeros(B, heads, L_PAD, W, dtype=torch.int32, device=dev)
    _native.check(abi.forward(lib, pq, pctx, B, L_PAD, heads, mask=pm, bits=pbits, scale=SCALE, drop=(p, SEED, SITE)),
                  "padded forward")
    torch.cuda.synchronize()
    pbits, pctx = pbits.cpu(), pctx.cpu().reshape(B, L_PAD, H)
    for tag, launches in (("one launch", one), ("per class", per_class)):
        ctx, _, bits = _run_fwd(dev, c, launches, p)
        bits, ctx = bits.cpu(), ctx.cpu()[GUARD:GUARD + T]
        dropped = 0
        for b, n in enumerate(lens):
            got = _unpack_words(bits[:, cu[b]:cu[b + 1]], n)
            ref = _unpack_words(pbits[b, :, :n], n)
            assert torch.equal(got, ref), f"{tag}: keeps of sequence {b} (len {n}) differ from the padded forward's"
            dropped += int((~got).sum())
        assert torch.isfinite(ctx.float()).all()
        total = heads * sum(n * n for n in lens)
        assert 0.08 < dropped / total < 0.12, f"{tag}: drop rate {dropped / total:.4f}"


def test_varlen_bwd_on_the_varlen_forwards_outputs(dev):
    """The backward on the varlen forward's own ctx, lse and keep bits at p = 0.1: dQ, dK <= 5 u A (D
    carries the forward's 2.5 u), dV <= 2.5 u A; with drop_bits = NULL the same keeps are drawn again:
    the same dqkv bits."""
    import torch
    heads, p = 4, 0.1
    base = _case(heads, "gauss", "keep01")
    lens, cu, B = base["lens"], base["cu"], len(base["lens"])
    T = base["qkv"].shape[0]
    ctx, lse, bits = _run_fwd(dev, base, [(None, B, 160)], p)
    words = bits.cpu()
    keeps = [_unpack_words(words[:, cu[b]:cu[b + 1]], n) for b, n in enumerate(lens)]
    c = _case(heads, "gauss", "keep01", keeps=keeps)
    ctxd = ctx[GUARD:GUARD + T].contiguous()
    buf, _ = _run_bwd(dev, c, None, B, 160, ctx=ctxd, lse=lse, bits=bits)
    worst = _check_rows(buf, c, set(range(B)), "on the forward's outputs", dqk=bc.BOUND_DQK_FWD)
    print("varlen bwd on the varlen forward's outputs: worst u A " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    again, _ = _run_bwd(dev, c, None, B, 160, ctx=ctxd, lse=lse, bits=None)
    assert torch.equal(buf.view(torch.int16), again.view(torch.int16)), "dqkv differs when the keeps are drawn again"


@pytest.mark.parametrize("variant", ["plain", "keep01"])
def test_sequence_alone_has_the_padded_kernels_bits(dev, variant):
    """A sequence run alone at its own class (max_len = len) gives the dqkv bits of
    drt_attention_backward_bf16 with B = 1, L = len, no mask, the same lse and keep bits."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads = 4
    H = heads * 64
    c = _case(heads, "gauss", variant)
    cu = c["cu"]
    for b, s in enumerate(c["seqs"]):
        n = s["n"]
        buf, _ = _run_bwd(dev, c, [b], 1, n)
        got = buf[GUARD + cu[b]:GUARD + cu[b + 1]]
        assert torch.isnan(buf[:GUARD + cu[b]].float()).all() and torch.isnan(buf[GUARD + cu[b + 1]:].float()).all()
        dqkv = torch.full((n, 3 * H), float("nan"), dtype=torch.bfloat16, device=dev)
        pb = None if s["keep"] is None else bc.pack_bits(s["keep"]).to(dev)
        _native.check(abi.backward(lib, s["qkv"].to(dev), s["ref"].O.to(torch.bfloat16).to(dev), s["dctx"].to(dev),
                                   s["ref"].lse.float().to(dev), dqkv, 1, n, heads, bits=pb, scale=SCALE,
                                   drop=(c["p"], SEED, SITE)), "padded backward")
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), dqkv.cpu().view(torch.int16)), f"{variant}: sequence {b} (len {n})"


def test_clamped_and_empty_lengths(dev):
    """A table entry longer than max_len is clamped: the first max_len tokens are differentiated as a
    sequence of that length, rows past it stay NaN (nothing past the LDS image is touched).  A
    zero-length entry writes nothing, in dqkv or in dsum."""
    import torch
    heads, n, ml = 4, 100, 64
    H = heads * 64
    g = bc.gen("packed-train-clamp")
    qkv, dctx = bc.make_qkv_dctx("gauss", 1, n, heads, None, g)
    ref = br.attention_bwd_ref(qkv[:ml], dctx[:ml], None, 1, ml, heads, SCALE)
    lse = torch.full((heads, n), float("nan"))
    lse[:, :ml] = ref.lse[0].float()
    ctx = torch.full((n, H), float("nan"), dtype=torch.bfloat16)
    ctx[:ml] = ref.O.to(torch.bfloat16)
    c = dict(heads=heads, p=0.0, qkv=qkv, dctx=dctx, ctx=ctx, lse=lse, bits=None, cu=[0, n], lens=[n])
    buf, dsum = _run_bwd(dev, c, None, 1, ml, want_dsum=True, l_pad=n)
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + ml:].float()).all()
    got = buf[GUARD:GUARD + ml]
    assert not bc.over_bounds(bc.attention_ratios(got, None, ref))
    assert torch.isfinite(dsum).all()
    # [40, 0, 50]: the middle entry is empty
    lens = [40, 0, 50]
    T = sum(lens)
    refs = []
    for lo, hi in ((0, 40), (40, 90)):
        refs.append(br.attention_bwd_ref(qkv[lo:hi], dctx[lo:hi], None, 1, hi - lo, heads, SCALE))
    c = dict(heads=heads, p=0.0, qkv=qkv[:T].contiguous(), dctx=dctx[:T].contiguous(),
             ctx=torch.cat([r.O.to(torch.bfloat16) for r in refs], 0),
             lse=torch.cat([r.lse[0].float() for r in refs], 1).contiguous(), bits=None, cu=_cu(lens), lens=lens)
    buf, dsum = _run_bwd(dev, c, None, 3, 64, want_dsum=True, l_pad=64)
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + T:].float()).all()
    assert torch.isnan(dsum[1]).all() and torch.isfinite(dsum[[0, 2]]).all()
    for r, (lo, hi) in zip(refs, ((0, 40), (40, 90))):
        assert not bc.over_bounds(bc.attention_ratios(buf[GUARD + lo:GUARD + hi], None, r))
    # the forward does the same
    cf = dict(c, p=0.0)
    ctxf, lsef, _ = _run_fwd(dev, cf, [(None, 3, 64)], 0.0)
    assert torch.isnan(ctxf[:GUARD].float()).all() and torch.isnan(ctxf[GUARD + T:].float()).all()
    assert torch.isfinite(ctxf[GUARD:GUARD + T].float()).all() and torch.isfinite(lsef).all()


@pytest.mark.parametrize("H", [8, 768, 1000])
def test_pack_rows_inverts_unpack_rows(dev, H):
    """pack_rows(unpack_rows(x)) == x bit for bit; the rows up to out_rows behind T are zeros and
    nothing further is written; the pad rows of the padded matrix are never read (they hold NaN)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    s = _native.stream_ptr(dev)
    lens, L = [9, 37, 1, 37, 20], 37
    B, T = len(lens), sum(lens)
    rows = (T + 31) // 32 * 32
    x = torch.randn(T, H, generator=bc.gen("pack-rows", H)).to(torch.bfloat16)
    xd = x.to(dev)
    cud = torch.tensor(_cu(lens), dtype=torch.int32, device=dev)
    padded = torch.full((B * L, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_unpack_rows_bf16(xd.data_ptr(), cud.data_ptr(), B, L, H, padded.data_ptr(), s), "unpack")
    out = torch.full((rows + 3, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_pack_rows_bf16(padded.data_ptr(), cud.data_ptr(), B, L, H, out.data_ptr(), rows, s), "pack")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out[:T].view(torch.int16), x.view(torch.int16))
    assert (out[T:rows].view(torch.int16) == 0).all() and torch.isnan(out[rows:].float()).all()
    # NaN at the pad positions of the input: none of it reaches the packed rows
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).reshape(B * L).to(dev)
    poisoned = torch.where(mask[:, None], padded, torch.full_like(padded, float("nan")))
    out2 = torch.full((T, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_pack_rows_bf16(poisoned.data_ptr(), cud.data_ptr(), B, L, H, out2.data_ptr(), T, s), "pack")
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu().view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("with_types", [False, True])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_embed_ln_pre_packed_has_the_padded_rows(dev, H, with_types):
    """out and pre rows bit-equal to drt_embed_ln_pre's rows of the same tokens; out bit-equal to
    drt_embed_ln_packed; nothing written past row T."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    s = _native.stream_ptr(dev)
    lens, L, vocab = [1, 40, 7, 33, 18], 40, 1000          # T = 99: a ragged last block
    B, T = len(lens), sum(lens)
    g = bc.gen("packed-emb-pre", H, with_types)
    word = 0.02 * torch.randn(vocab, H, generator=g)
    pos = 0.02 * torch.randn(512, H, generator=g)
    typ = 0.02 * torch.randn(2, H, generator=g)
    gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
    ids = torch.randint(0, vocab, (B, L), generator=g)
    tt = torch.randint(0, 2, (B, L), generator=g).to(dev) if with_types else None
    ttp = None if tt is None else tt.data_ptr()
    d = [x.to(dev) for x in (ids, word, pos, typ, gamma, beta)]
    cu = _cu(lens)
    cud = torch.tensor(cu, dtype=torch.int32, device=dev)
    nan = lambda r: torch.full((r, H), float("nan"), dtype=torch.bfloat16, device=dev)   # noqa: E731
    out, pre, out_inf, p_out, p_pre = nan(T + 4), nan(T + 4), nan(T), nan(B * L), nan(B * L)
    tail = [x.data_ptr() for x in d[1:]]
    _native.check(lib.drt_embed_ln_pre_packed(d[0].data_ptr(), ttp, cud.data_ptr(), B, L, T, *tail, 1e-12, H,
                                              out.data_ptr(), pre.data_ptr(), s), "embed_ln_pre_packed")
    _native.check(lib.drt_embed_ln_packed(d[0].data_ptr(), ttp, cud.data_ptr(), B, L, T, *tail, 1e-12, H,
                                          out_inf.data_ptr(), s), "embed_ln_packed")
    _native.check(lib.drt_embed_ln_pre(d[0].data_ptr(), ttp, B, L, *tail, 1e-12, H, p_out.data_ptr(), p_pre.data_ptr(), s),
                  "embed_ln_pre")
    torch.cuda.synchronize()
    out, pre, out_inf = out.cpu(), pre.cpu(), out_inf.cpu()
    p_out, p_pre = p_out.cpu().reshape(B, L, H), p_pre.cpu().reshape(B, L, H)
    assert torch.isnan(out[T:].float()).all() and torch.isnan(pre[T:].float()).all(), "rows past T written"
    assert torch.equal(out[:T].view(torch.int16), out_inf.view(torch.int16))
    for b, n in enumerate(lens):
        rows = slice(cu[b], cu[b + 1])
        assert torch.equal(out[rows].view(torch.int16), p_out[b, :n].contiguous().view(torch.int16)), f"out, sequence {b}"
        assert torch.equal(pre[rows].view(torch.int16), p_pre[b, :n].contiguous().view(torch.int16)), f"pre, sequence {b}"

"""The kernels of padding-free training above 160 tokens through their native entries
(include/drt.h, "Padding-free BERT training"): the streamed varlen backward over a tile table and the
varlen training forward up to 512 tokens, on one shuffled packed batch with a length on both sides of
every 128-row tile edge and 32-row block edge above 160, against the fp64 references of
tests/encoder_bwd_refs.py per sequence with the bounds of tests/encoder_bwd_cases.py, and bit for bit
against the padded kernels where the contract says so.

Bounds (the streamed kernels' own, u = 2^-8): dV <= 2.5 u A_V, dQ / dK <= 3.5 u A on ctx = bf16(O_ref)
and lse = fp32(lse_ref); 5 u A for dQ / dK on the varlen forward's own ctx, lse and keep bits.
"""
import random

import pytest

import attention_abi as abi
import encoder_bwd_cases as bc
import encoder_bwd_refs as br
import test_packed_train_kernels_gpu as pk   # _cu, _pad_words, _unpack_words, _colsum, GUARD

pytestmark = pytest.mark.gpu

LENS = (33, 128, 161, 192, 193, 256, 257, 384, 385, 511, 512)
L_PAD, W, GUARD = 512, 16, pk.GUARD
VARIANT_P = {"plain": 0.0, "keep01": 0.1}
SEED, SITE, SCALE = 4321, 9, 0.125
LONG_CLASS_MAX = (192, 288, 512)     # the forward's launch classes (model/packing.py)

_CASES = {}


def _case(heads, data, variant, keeps=None):
    """The packed batch of (heads, data, variant), built once and left unchanged: per-sequence fp64
    references, packed qkv / dctx / ctx = bf16(O_ref) / lse = fp32(lse_ref) / keep words.  ``keeps``
    (bool [heads, n, n] per sequence) replaces the drawn keep masks (not cached)."""
    import torch
    key = (heads, data, variant)
    if keeps is None and key in _CASES:
        return _CASES[key]
    lens = list(LENS)
    random.Random(5 + heads).shuffle(lens)
    p = VARIANT_P[variant]
    seqs = []
    for b, n in enumerate(lens):
        qkv_b, dctx_b = bc.make_qkv_dctx(data, 1, n, heads, None, bc.gen("packed-long", heads, data, b, n))
        keep = None
        if p > 0:
            keep = bc.make_keep(1, n, heads, p, None, bc.gen("packed-long", "keep", heads, b, n))
            if keeps is not None:
                keep = keeps[b][None]
        ref = br.attention_bwd_ref(qkv_b, dctx_b, None, 1, n, heads, SCALE, keep=keep, p=p)
        seqs.append(dict(n=n, qkv=qkv_b, dctx=dctx_b, keep=keep, ref=ref))
    c = dict(heads=heads, p=p, lens=lens, cu=pk._cu(lens), seqs=seqs,
             qkv=torch.cat([s["qkv"] for s in seqs], 0), dctx=torch.cat([s["dctx"] for s in seqs], 0),
             ctx=torch.cat([s["ref"].O.to(torch.bfloat16) for s in seqs], 0),
             lse=torch.cat([s["ref"].lse[0].float() for s in seqs], 1).contiguous(),
             bits=None if p == 0 else torch.cat([pk._pad_words(bc.pack_bits(s["keep"])[0], W) for s in seqs], 1).contiguous())
    if keeps is None:
        _CASES[key] = c
    return c


def _tiles(lens, ids):
    return [(b, g) for b in ids for g in range((lens[b] + 127) // 128)]


def _run_bwd(dev, c, tiles, max_len, *, want_dsum=False, ctx=None, lse=None, bits="case", cu=None, l_pad=L_PAD):
    """drt_attention_varlen_long_backward_bf16 over ``tiles``; outputs start as NaN.  Returns CPU (dqkv
    with its guard rows, dsum [n_tiles, 3H] or None)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads = c["heads"]
    T = c["qkv"].shape[0]
    to = lambda t: None if t is None else t.to(dev)   # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    qd, dod = to(c["qkv"]), to(c["dctx"])
    ctxd = to(c["ctx"]) if ctx is None else ctx
    lsed = to(c["lse"]) if lse is None else lse
    bitsd = to(c["bits"]) if isinstance(bits, str) else bits
    cud = torch.tensor(c["cu"] if cu is None else cu, dtype=torch.int32, device=dev)
    td = torch.tensor(tiles, dtype=torch.int32, device=dev).reshape(-1, 2)
    buf = torch.full((GUARD + T + GUARD, 3 * heads * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    dsum = torch.full((len(tiles), 3 * heads * 64), float("nan"), device=dev) if want_dsum else None
    _native.check(lib.drt_attention_varlen_long_backward_bf16(
        qd.data_ptr(), ctxd.data_ptr(), dod.data_ptr(), lsed.data_ptr(), cud.data_ptr(), td.data_ptr(), len(tiles),
        max_len, l_pad, T, W, ptr(bitsd), buf[GUARD:].data_ptr(), ptr(dsum), heads, 64, SCALE, c["p"], SEED, SITE,
        _native.stream_ptr(dev)), "varlen long attention backward")
    torch.cuda.synchronize()
    return buf.cpu(), None if dsum is None else dsum.cpu()


def _check_rows(buf, c, listed, tag, dqk=bc.BOUND_DQK):
    """Listed sequences within the bounds of their own fp64 reference, every other row (guards
    included) still NaN.  Returns the worst ratios."""
    import torch
    cu, T = c["cu"], c["qkv"].shape[0]
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + T:].float()).all(), f"{tag}: guard rows"
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


@pytest.mark.parametrize("data", bc.DATA_KINDS)
@pytest.mark.parametrize("variant", ["plain", "keep01"])
@pytest.mark.parametrize("heads", [4, 12])
def test_long_bwd_vs_fp64(dev, heads, variant, data):
    """Every sequence's dQ, dK, dV within the bounds of the fp64 reference of that sequence alone, in
    one launch over every tile and in a launch over three sequences (the others stay NaN); dqkv
    bit-equal between two runs and with or without the partial sums; each tile's partial row and
    drt_colsum_f32 of them by the existing dbias rule.

    Measured on an MI355X: see DESIGN.md section 5, "Padding-free training above 160 tokens"."""
    import torch
    c = _case(heads, data, variant)
    lens, cu, B, T = c["lens"], c["cu"], len(c["lens"]), c["qkv"].shape[0]
    tag = f"heads={heads} {variant} {data}"
    tiles = _tiles(lens, range(B))
    buf, _ = _run_bwd(dev, c, tiles, 512)
    worst = _check_rows(buf, c, set(range(B)), tag)
    print(f"varlen long bwd {tag}: worst u A " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    buf2, dsum = _run_bwd(dev, c, tiles, 512, want_dsum=True)
    assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16)), f"{tag}: dqkv differs with dsum / between runs"
    d = buf[GUARD:GUARD + T].double()
    for t, (b, g) in enumerate(tiles):   # row t: the column sums of the tile's stored rows
        rows = d[cu[b] + 128 * g:min(cu[b] + 128 * (g + 1), cu[b + 1])]
        assert ((dsum[t].double() - rows.sum(0)).abs() <= 1e-5 * rows.abs().sum(0) + 1e-6).all(), f"{tag}: tile {b, g}"
    dbias = pk._colsum(dev, dsum)
    assert ((dbias.double() - d.sum(0)).abs() <= 1e-5 * d.abs().sum(0) + 1e-6).all(), f"{tag}: dbias"
    ids = [b for b, n in enumerate(lens) if n in (161, 257, 385)]
    bufs, _ = _run_bwd(dev, c, _tiles(lens, ids), 385)
    _check_rows(bufs, c, set(ids), f"{tag} subset max_len 385")


@pytest.mark.parametrize("n", [161, 257, 512])
@pytest.mark.parametrize("variant", ["plain", "keep01"])
def test_sequence_alone_has_the_padded_streamed_kernels_bits(dev, variant, n):
    """A sequence run alone (max_len = len) gives the dqkv bits of drt_attention_backward_bf16 with
    B = 1, L = len, no mask, on the same lse and keep bits."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads = 4
    c = _case(heads, "gauss", variant)
    b = c["lens"].index(n)
    s, cu = c["seqs"][b], c["cu"]
    buf, _ = _run_bwd(dev, c, _tiles(c["lens"], [b]), n)
    got = buf[GUARD + cu[b]:GUARD + cu[b + 1]]
    assert torch.isnan(buf[:GUARD + cu[b]].float()).all() and torch.isnan(buf[GUARD + cu[b + 1]:].float()).all()
    dqkv = torch.full((n, 3 * heads * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    pb = None if s["keep"] is None else bc.pack_bits(s["keep"]).to(dev)
    _native.check(abi.backward(lib, s["qkv"].to(dev), s["ref"].O.to(torch.bfloat16).to(dev), s["dctx"].to(dev),
                               s["ref"].lse.float().to(dev), dqkv, 1, n, heads, bits=pb, scale=SCALE,
                               drop=(c["p"], SEED, SITE)), "padded backward")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), dqkv.cpu().view(torch.int16))


def _run_fwd(dev, c, launches, p, *, want_lse=True, inference=False):
    """The long varlen training forward (or the inference entry) over ``launches`` = [(seq_ids, n, max_len)].
    Returns device (ctx with guard rows, lse [heads, T], bits [heads, T, W])."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads, T = c["heads"], c["qkv"].shape[0]
    qd = c["qkv"].to(dev)
    cud = torch.tensor(c["cu"], dtype=torch.int32, device=dev)
    ctx = torch.full((GUARD + T + GUARD, heads * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((heads, T), float("nan"), device=dev) if want_lse else None
    bits = torch.zeros((heads, T, W), dtype=torch.int32, device=dev) if p > 0 else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    s = _native.stream_ptr(dev)
    for ids, n, ml in launches:
        sd = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev)
        if inference:
            rc = lib.drt_attention_varlen_forward_bf16(qd.data_ptr(), cud.data_ptr(), ptr(sd), n, ml,
                                                       ctx[GUARD:].data_ptr(), heads, 64, SCALE, s)
        else:
            rc = lib.drt_attention_varlen_long_train_forward_bf16(
                qd.data_ptr(), cud.data_ptr(), ptr(sd), n, ml, L_PAD, T, W, ctx[GUARD:].data_ptr(), ptr(lse), ptr(bits),
                heads, 64, SCALE, p, SEED, SITE, s)
        _native.check(rc, "varlen long attention forward")
        torch.cuda.synchronize()
    return ctx, lse, bits


def _policies(lens):
    """One launch at max_len 512, and one launch per LDS-image class of the forward."""
    groups = {}
    for b, n in enumerate(lens):
        groups.setdefault(next(m for m in LONG_CLASS_MAX if n <= m), []).append(b)
    return {"one launch": [(None, len(lens), 512)],
            "per class": [(ids, len(ids), max(lens[b] for b in ids)) for _, ids in sorted(groups.items(), reverse=True)]}


@pytest.mark.parametrize("policy", ["one launch", "per class"])
@pytest.mark.parametrize("heads", [4, 12])
def test_long_train_forward(dev, heads, policy):
    """lse within atol 1e-3, rtol 1e-4 of the reference; at p = 0 the ctx bits of
    drt_attention_varlen_forward_bf16, with and without lse; at p = 0.1 the keeps of every real
    (q, key) equal those of drt_attention_forward_bf16 on the padded [B, 512] batch with the same
    (p, seed, site), and the drop rate lies in (0.08, 0.12)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    c = _case(heads, "gauss", "plain")
    lens, cu, B = c["lens"], c["cu"], len(c["lens"])
    T, H = c["qkv"].shape[0], heads * 64
    launches = _policies(lens)[policy]
    want, _, _ = _run_fwd(dev, c, [(None, B, 512)], 0.0, inference=True)
    ctx, lse, _ = _run_fwd(dev, c, launches, 0.0)
    ctx0, _, _ = _run_fwd(dev, c, launches, 0.0, want_lse=False)
    assert torch.equal(ctx.view(torch.int16), want.view(torch.int16)), "ctx bits differ from the inference entry"
    assert torch.equal(ctx.view(torch.int16), ctx0.view(torch.int16)), "ctx differs without lse"
    assert torch.isnan(ctx[:GUARD].float()).all() and torch.isnan(ctx[GUARD + T:].float()).all()
    torch.testing.assert_close(lse.cpu(), c["lse"], atol=1e-3, rtol=1e-4)
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
    ctx, _, bits = _run_fwd(dev, c, launches, p)
    pbits, bits, ctx = pbits.cpu(), bits.cpu(), ctx.cpu()[GUARD:GUARD + T]
    dropped = 0
    for b, n in enumerate(lens):
        got = pk._unpack_words(bits[:, cu[b]:cu[b + 1]], n)
        assert torch.equal(got, pk._unpack_words(pbits[b, :, :n], n)), f"keeps of sequence {b} (len {n})"
        dropped += int((~got).sum())
    assert torch.isfinite(ctx.float()).all()
    total = heads * sum(n * n for n in lens)
    assert 0.08 < dropped / total < 0.12, f"drop rate {dropped / total:.4f}"


def test_long_bwd_on_the_long_forwards_outputs(dev):
    """The backward on the forward's own ctx, lse and keep bits at p = 0.1: dQ, dK <= 5 u A, dV <= 2.5 u A;
    with drop_bits = NULL the same keeps are drawn again: the same dqkv bits."""
    import torch
    heads, p = 4, 0.1
    base = _case(heads, "gauss", "keep01")
    lens, cu, B, T = base["lens"], base["cu"], len(base["lens"]), base["qkv"].shape[0]
    ctx, lse, bits = _run_fwd(dev, base, [(None, B, 512)], p)
    words = bits.cpu()
    c = _case(heads, "gauss", "keep01", keeps=[pk._unpack_words(words[:, cu[b]:cu[b + 1]], n) for b, n in enumerate(lens)])
    ctxd = ctx[GUARD:GUARD + T].contiguous()
    tiles = _tiles(lens, range(B))
    buf, _ = _run_bwd(dev, c, tiles, 512, ctx=ctxd, lse=lse, bits=bits)
    worst = _check_rows(buf, c, set(range(B)), "on the forward's outputs", dqk=bc.BOUND_DQK_FWD)
    print("varlen long bwd on the long forward's outputs: worst u A " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    again, _ = _run_bwd(dev, c, tiles, 512, ctx=ctxd, lse=lse, bits=None)
    assert torch.equal(buf.view(torch.int16), again.view(torch.int16)), "dqkv differs when the keeps are drawn again"


def test_clamped_and_empty_entries(dev):
    """A table entry longer than max_len is clamped: its first max_len tokens are differentiated as a
    sequence of that length, rows past it stay NaN.  A zero-length entry, and a tile past a sequence's
    end, write nothing, in dqkv or in the partial sums."""
    import torch
    heads, n, ml = 4, 300, 200
    g = bc.gen("packed-long-clamp")
    qkv, dctx = bc.make_qkv_dctx("gauss", 1, n, heads, None, g)
    ref = br.attention_bwd_ref(qkv[:ml], dctx[:ml], None, 1, ml, heads, SCALE)
    lse = torch.full((heads, n), float("nan"))
    lse[:, :ml] = ref.lse[0].float()
    ctx = torch.full((n, heads * 64), float("nan"), dtype=torch.bfloat16)
    ctx[:ml] = ref.O.to(torch.bfloat16)
    c = dict(heads=heads, p=0.0, qkv=qkv, dctx=dctx, ctx=ctx, lse=lse, bits=None, cu=[0, n], lens=[n])
    # tiles 0 and 1 hold the clamped sequence; tile 2 starts at row 256 >= 200: nothing
    buf, dsum = _run_bwd(dev, c, [(0, 0), (0, 1), (0, 2)], ml, want_dsum=True, l_pad=n)
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + ml:].float()).all()
    assert not bc.over_bounds(bc.attention_ratios(buf[GUARD:GUARD + ml], None, ref))
    assert torch.isfinite(dsum[:2]).all() and torch.isnan(dsum[2]).all()
    # [170, 0, 130]: the middle entry is empty
    lens, spans = [170, 0, 130], ((0, 170), (170, 300))
    refs = [br.attention_bwd_ref(qkv[lo:hi], dctx[lo:hi], None, 1, hi - lo, heads, SCALE) for lo, hi in spans]
    c = dict(heads=heads, p=0.0, qkv=qkv, dctx=dctx, ctx=torch.cat([r.O.to(torch.bfloat16) for r in refs], 0),
             lse=torch.cat([r.lse[0].float() for r in refs], 1).contiguous(), bits=None, cu=pk._cu(lens), lens=lens)
    buf, dsum = _run_bwd(dev, c, [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)], 170, want_dsum=True, l_pad=170)
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + n:].float()).all()
    assert torch.isnan(dsum[2]).all() and torch.isfinite(dsum[[0, 1, 3, 4]]).all()
    for r, (lo, hi) in zip(refs, spans):
        assert not bc.over_bounds(bc.attention_ratios(buf[GUARD + lo:GUARD + hi], None, r))

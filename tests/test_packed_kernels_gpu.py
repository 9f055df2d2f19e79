"""The kernels of the padding-free inference path through their native entry points, against the
plain fp64 references of tests/encoder_refs.py with the bounds of tests/test_encoder_fwd_fp64_gpu.py:
the varlen attention over one packed batch that mixes every length class, the packed embedding
(also bit for bit against the padded kernel's rows), the packed pooling and the unpack copy."""
import random

import pytest

import encoder_refs as er
import test_encoder_fwd_fp64_gpu as fwd

pytestmark = pytest.mark.gpu

U = fwd.U
ATT_LENS = (1, 31, 32, 33, 64, 100, 128, 129, 160, 161, 257, 512)
GUARD = 8          # NaN rows before row 0 and after row T of ctx

_ATT_CASES = {}


def _att_case(heads, data):
    """(lens, cu list, packed qkv bf16 [T, 3H], fp64 ref [T, H], A [T, H]) of the one packed batch,
    built once per (heads, data) and left unchanged."""
    import torch
    key = (heads, data)
    if key not in _ATT_CASES:
        lens = list(ATT_LENS)
        random.Random(7 + heads).shuffle(lens)
        H = heads * 64
        parts, refs, As = [], [], []
        for b, n in enumerate(lens):
            g = fwd._gen("packed-att", heads, data, b, n)
            qkv_b = fwd._qkv(data, 1, n, heads, None, g).float()
            qkv_b[:, 2 * H:] *= 4.0 ** (b % 6)      # exact in bf16: a neighbour's V is far off the bound
            qkv_b = qkv_b.to(torch.bfloat16)
            ref, A, _ = er.attention_ref(qkv_b, None, 1, n, heads, 0.125)
            parts.append(qkv_b)
            refs.append(ref)
            As.append(A)
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        _ATT_CASES[key] = (lens, cu, torch.cat(parts, 0), torch.cat(refs, 0), torch.cat(As, 0))
    return _ATT_CASES[key]


def _run_varlen(lib, dev, qkv, cu, heads, seq_ids, n_seqs, max_len):
    """ctx [GUARD + T + GUARD, H] on the CPU; everything starts as NaN."""
    import torch
    from denseretrievaltoolkits_amd import _native
    T, H = qkv.shape[0], heads * 64
    qd = qkv.to(dev)
    cud = torch.tensor(cu, dtype=torch.int32, device=dev)
    sd = None if seq_ids is None else torch.tensor(seq_ids, dtype=torch.int32, device=dev)
    buf = torch.full((GUARD + T + GUARD, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_attention_varlen_forward_bf16(qd.data_ptr(), cud.data_ptr(),
                                                        None if sd is None else sd.data_ptr(), n_seqs, max_len,
                                                        buf[GUARD:].data_ptr(), heads, 64, 0.125,
                                                        _native.stream_ptr(dev)), "varlen attention")
    torch.cuda.synchronize()
    return buf.cpu()


def _check_rows(buf, cu, lens, listed, ref, A, tag):
    """Listed sequences within 2.5 u A + 1e-7 of fp64, every other row (guards included) still NaN."""
    import torch
    T = cu[-1]
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + T:].float()).all(), \
        f"{tag}: guard rows written"
    ctx = buf[GUARD:GUARD + T]
    worst = 0.0
    for b, n in enumerate(lens):
        rows = slice(cu[b], cu[b + 1])
        if b not in listed:
            assert torch.isnan(ctx[rows].float()).all(), f"{tag}: unlisted sequence {b} (len {n}) written"
            continue
        assert torch.isfinite(ctx[rows].float()).all(), f"{tag}: sequence {b} (len {n}) not finite"
        ratio = fwd._ctx_ratio(ctx[rows], ref[rows], A[rows])
        worst = max(worst, ratio)
        assert ratio <= 2.5, f"{tag}: sequence {b} (len {n}) ctx error {ratio:.3f} u A > 2.5 u A"
    return worst


@pytest.mark.parametrize("data", ["gauss", "ramp"])
@pytest.mark.parametrize("heads", [12, 4])
def test_varlen_attention_vs_fp64(dev, heads, data):
    """One packed batch of lengths 1 .. 512 in shuffled order: every sequence within 2.5 u A + 1e-7
    of the fp64 reference of that sequence alone, with the whole batch in one launch (max_len 512:
    the streamed kernel), and with one launch per length class as the encoder issues them
    (ceil(len / 32) = 1 .. 5 and the streamed rest); a launch over a subset with a smaller max_len
    leaves every other row untouched."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    lens, cu, qkv, ref, A = _att_case(heads, data)
    B = len(lens)
    buf = _run_varlen(lib, dev, qkv, cu, heads, None, B, max(lens))
    worst = _check_rows(buf, cu, lens, set(range(B)), ref, A, f"heads={heads} {data} one launch")
    print(f"varlen attention heads={heads} {data} one launch: worst ctx error {worst:.3f} u A")
    classes = {}
    for b, n in enumerate(lens):
        nb = (n + 31) // 32
        classes.setdefault(nb if nb <= 5 else 0, []).append(b)
    for c, ids in sorted(classes.items()):
        ml = max(lens[b] for b in ids)
        buf = _run_varlen(lib, dev, qkv, cu, heads, ids, len(ids), ml)
        worst = _check_rows(buf, cu, lens, set(ids), ref, A, f"heads={heads} {data} class {c} max_len {ml}")
        print(f"varlen attention heads={heads} {data} class {c} (lens {[lens[b] for b in ids]}): "
              f"worst ctx error {worst:.3f} u A")
    # short sequences in a wider class (what one launch per batch does): whole query blocks and key
    # tiles without a token, with 4 waves (max_len 128) and with 5 (max_len 160)
    for ml, pick in ((128, (1, 33, 100)), (160, (1, 31, 64, 100, 129, 160))):
        ids = [b for b, n in enumerate(lens) if n in pick]
        buf = _run_varlen(lib, dev, qkv, cu, heads, ids, len(ids), ml)
        _check_rows(buf, cu, lens, set(ids), ref, A, f"heads={heads} {data} subset max_len {ml}")


def test_varlen_attention_clamps_length_to_max_len(dev):
    """A table whose sequence is longer than max_len: the kernel attends over its first max_len
    tokens only and writes those rows only (never past the launch's LDS image)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    heads, n, ml = 4, 100, 64
    g = fwd._gen("packed-clamp")
    qkv = fwd._qkv("gauss", 1, n, heads, None, g)
    ref, A, _ = er.attention_ref(qkv[:ml], None, 1, ml, heads, 0.125)
    buf = _run_varlen(lib, dev, qkv, [0, n], heads, None, 1, ml)
    ctx = buf[GUARD:GUARD + n]
    assert torch.isnan(ctx[ml:].float()).all() and torch.isnan(buf[:GUARD].float()).all()
    assert fwd._ctx_ratio(ctx[:ml], ref, A) <= 2.5


# ---------------------------------------------------------------------------------------------
# drt_embed_ln_packed
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_types", [False, True])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_embed_ln_packed_vs_fp64_and_padded_rows(dev, H, with_types):
    """Each packed row within one bf16 rounding of the fp64 LayerNorm of its sequence alone
    (positions restart at 0), bit-equal to the padded kernel's row of the same token, and nothing
    written past row T (T % 4 = 3: a ragged last block)."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    s = _native.stream_ptr(dev)
    lens, L = [1, 40, 7, 33, 18], 40                      # T = 99
    B, T = len(lens), sum(lens)
    g = fwd._gen("packed-emb", H, with_types)
    word = 0.02 * torch.randn(fwd.VOCAB, H, generator=g)
    pos = 0.02 * torch.randn(512, H, generator=g)
    typ = 0.02 * torch.randn(2, H, generator=g)
    gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
    ids = torch.randint(0, fwd.VOCAB, (B, L), generator=g)
    ids[0, 0], ids[1, L - 1] = 0, fwd.VOCAB - 1
    tt = torch.randint(0, 2, (B, L), generator=g) if with_types else None
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    eps = 1e-12
    d = [x.to(dev) for x in (ids, word, pos, typ, gamma, beta)]
    ttd = None if tt is None else tt.to(dev)
    ttp = None if ttd is None else ttd.data_ptr()
    cud = torch.tensor(cu, dtype=torch.int32, device=dev)
    out = torch.full((T + 4, H), float("nan"), dtype=torch.bfloat16, device=dev)
    padded = torch.full((B * L, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_embed_ln_packed(d[0].data_ptr(), ttp, cud.data_ptr(), B, L, T, d[1].data_ptr(),
                                          d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), eps, H,
                                          out.data_ptr(), s), "embed_ln_packed")
    _native.check(lib.drt_embed_ln(d[0].data_ptr(), ttp, B, L, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                   d[4].data_ptr(), d[5].data_ptr(), eps, H, padded.data_ptr(), s), "embed_ln")
    torch.cuda.synchronize()
    out, padded = out.cpu(), padded.cpu().reshape(B, L, H)
    assert torch.isnan(out[T:].float()).all(), "rows past T written"
    assert torch.isfinite(out[:T].float()).all()
    for b, n in enumerate(lens):
        rows = out[cu[b]:cu[b + 1]]
        ref = er.embed_ln_ref(ids[b, :n], None if tt is None else tt[b, :n], n, word, pos, typ, gamma, beta, eps)
        err = (rows.double() - ref).abs()
        bound = U * ref.abs() + U * beta.double().abs()[None, :] + 1e-6
        assert (err <= bound).all(), f"H={H} sequence {b}: err / bound {float((err / bound).max()):.3f}"
        assert torch.equal(rows.view(torch.int16), padded[b, :n].contiguous().view(torch.int16)), \
            f"H={H} sequence {b}: packed rows differ from the padded kernel's"


# ---------------------------------------------------------------------------------------------
# drt_pool_packed_bf16 / drt_unpack_rows_bf16
# ---------------------------------------------------------------------------------------------
def _packed_hidden(H, lens, L, g):
    """(packed bf16 [T, H], padded bf16 [B, L, H] with zeros at the pads, mask [B, L], cu)."""
    import torch
    B = len(lens)
    h = torch.randn(B, L, H, generator=g)
    h[0] = -h[0].abs() - 0.1                  # all negative, len < L: max pooling gives 0
    h[1] = -h[1].abs() - 0.1                  # all negative, len == L: the negative maximum
    h = h.to(torch.bfloat16)
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)
    h = torch.where(mask[:, :, None].bool(), h, torch.zeros_like(h))
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    packed = torch.cat([h[b, :n] for b, n in enumerate(lens)], 0).contiguous()
    return packed, h, mask, cu


@pytest.mark.parametrize("H", [64, 768, 1000])
def test_pool_packed_vs_fp64(dev, H):
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    s = _native.stream_ptr(dev)
    lens, L = [9, 37, 1, 37, 20], 37
    B = len(lens)
    assert lens[0] < L and lens[1] == L
    packed, h, mask, cu = _packed_hidden(H, lens, L, fwd._gen("packed-pool", H))
    pd = packed.to(dev)
    cud = torch.tensor(cu, dtype=torch.int32, device=dev)
    for mode in (0, 1, 2):
        out = torch.full((B + 1, H), float("nan"), device=dev)
        ob = torch.full((B + 1, H), float("nan"), dtype=torch.bfloat16, device=dev)
        _native.check(lib.drt_pool_packed_bf16(pd.data_ptr(), cud.data_ptr(), B, L, H, mode, out.data_ptr(),
                                               ob.data_ptr(), s), "pool_packed")
        torch.cuda.synchronize()
        out, ob = out.cpu(), ob.cpu()
        tag = f"H={H} mode={mode}"
        assert torch.isnan(out[B:]).all() and torch.isnan(ob[B:].float()).all(), f"{tag}: rows past B written"
        out, ob = out[:B], ob[:B]
        ref = er.pool_ref(h, mask, mode)
        if mode == 1:
            m = mask.double()
            sabs = (h.double().abs() * m[:, :, None]).sum(1)
            n = m.sum(1, keepdim=True)
            bound = n * 2.0 ** -24 * sabs / n + 1e-7
            err = (out.double() - ref).abs()
            assert (err <= bound).all(), f"{tag}: err / bound {float((err / bound).max()):.3f}"
        else:
            assert torch.equal(out.double(), ref), tag
        if mode == 2:
            assert (out[0] == 0).all(), f"{tag}: all-negative sequence with len < L"
            assert torch.equal(out[1].double(), h[1].double().max(0)[0]) and (out[1] < 0).all(), tag
        assert torch.equal(ob.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), tag
        # and the padded kernel's reps for the same batch
        want = torch.empty((B, H), device=dev)
        hd, md = h.to(dev), mask.to(dev)
        _native.check(lib.drt_pool_bf16(hd.data_ptr(), md.data_ptr(), B, L, H, mode, want.data_ptr(), None, s), "pool")
        torch.cuda.synchronize()
        assert torch.equal(out, want.cpu()), f"{tag}: differs from drt_pool_bf16"


@pytest.mark.parametrize("H", [8, 768, 1000])
def test_unpack_rows(dev, H):
    """Real rows bit-equal to the packed rows, pad rows exactly 0, nothing past B * L."""
    import torch
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    lens, L = [9, 37, 1, 37, 20], 37
    B = len(lens)
    packed, h, mask, cu = _packed_hidden(H, lens, L, fwd._gen("packed-unpack", H))
    pd = packed.to(dev)
    cud = torch.tensor(cu, dtype=torch.int32, device=dev)
    out = torch.full((B * L + 3, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(lib.drt_unpack_rows_bf16(pd.data_ptr(), cud.data_ptr(), B, L, H, out.data_ptr(),
                                           _native.stream_ptr(dev)), "unpack")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[B * L:].float()).all()
    got = out[:B * L].reshape(B, L, H)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n].contiguous().view(torch.int16),
                           packed[cu[b]:cu[b + 1]].view(torch.int16)), f"sequence {b}"
        assert (got[b, n:].view(torch.int16) == 0).all(), f"sequence {b}: pad rows not +0"

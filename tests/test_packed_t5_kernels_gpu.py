"""drt_attention_varlen_relbias_forward_bf16 (the packed T5 attention) through its native entry.

Bound: the project's attention bound, 2.5 u A + 1e-7 (tests/test_encoder_fwd_fp64_gpu.py); the bias is
one fp32 add in the score chain, inside that bound's slack (tests/test_t5_kernels_gpu.py).  Each
sequence's V is scaled by 4 ** (b % 6), so a neighbour's rows are far off the bound; the tables are
N(0, 1.5^2) per entry, not symmetric in k - q; queries are softened (Q / 8) as in the padded test."""
import pytest
import torch

import attention_abi as abi
import t5_refs as tr
import test_encoder_fwd_fp64_gpu as fwd

HEADS = 3
H = HEADS * 64
GUARD = 8          # NaN rows before row 0 and after row T of ctx
BATCHES = {"short": [1, 31, 32, 33, 64, 65, 96, 128, 129, 160], "long": [161, 200, 512, 17]}
_CASES = {}
P = 1              # a non-NULL pointer for the refusals


def _case(batch, span):
    """(lens, cu, qkv bf16 [T, 3H], table fp32 [HEADS, 2S-1], S, fp64 ref [T, H], A [T, H]); built once."""
    if (batch, span) not in _CASES:
        lens = BATCHES[batch]
        S = 512 if span == "512" else max(lens)
        g = fwd._gen("packed-t5-att", batch, span)
        table = 1.5 * torch.randn(HEADS, 2 * S - 1, generator=g)
        parts, refs, As = [], [], []
        for b, n in enumerate(lens):
            q = fwd._qkv("gauss", 1, n, HEADS, None, g).float()
            q[:, :H] *= 0.125
            q[:, 2 * H:] *= 4.0 ** (b % 6)
            q = q.to(torch.bfloat16)
            ref, A = tr.attention_relbias_ref(q, None, table[:, S - n:S + n - 1], 1, n, HEADS, 1.0)
            parts.append(q), refs.append(ref), As.append(A)
        cu = [0] + torch.tensor(lens).cumsum(0).tolist()
        _CASES[batch, span] = (lens, cu, torch.cat(parts), table, S, torch.cat(refs), torch.cat(As))
    return _CASES[batch, span]


def _run(dev, qkv, cu, table, S, seq_ids, max_len, entry="drt_attention_varlen_relbias_forward_bf16"):
    """ctx [T, H] on the CPU from one launch; unwritten rows are NaN, the guard rows are checked here."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    T = cu[-1]
    qd, cud = qkv.to(dev), torch.tensor(cu, dtype=torch.int32, device=dev)
    sd = None if seq_ids is None else torch.tensor(seq_ids, dtype=torch.int32, device=dev)
    n = len(cu) - 1 if seq_ids is None else len(seq_ids)
    buf = torch.full((GUARD + T + GUARD, H), float("nan"), dtype=torch.bfloat16, device=dev)
    head = (qd.data_ptr(), cud.data_ptr(), None if sd is None else sd.data_ptr(), n, max_len)
    tail = (buf[GUARD:].data_ptr(), HEADS, 64, 1.0, _native.stream_ptr(dev))
    bias = () if table is None else (table.to(dev).contiguous().data_ptr(), S)
    _native.check(getattr(lib, entry)(*head, *bias, *tail), entry)
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[GUARD + T:].float()).all(), "guard rows written"
    return buf[GUARD:GUARD + T]


def _launches(lens):
    """{length class: sequence ids}: ceil(len / 32) = 1 .. 5, the streamed rest as class 0."""
    out = {}
    for b, n in enumerate(lens):
        out.setdefault((n + 31) // 32 if n <= 160 else 0, []).append(b)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("span", ["512", "longest"])
@pytest.mark.parametrize("batch", ["short", "long"])
def test_varlen_relbias_vs_fp64(dev, batch, span):
    """short: one launch per class NB = 1 .. 5 over a subset list; long: one launch at max_len 512.  Listed
    sequences within the bound of their own fp64 reference; unlisted rows keep the sentinel."""
    lens, cu, qkv, table, S, ref, A = _case(batch, span)
    groups = _launches(lens) if batch == "short" else {0: list(range(len(lens)))}
    assert sorted(groups) == ([1, 2, 3, 4, 5] if batch == "short" else [0])
    for c, ids in groups.items():
        ctx = _run(dev, qkv, cu, table, S, ids if batch == "short" else None, max(lens[b] for b in ids))
        for b, n in enumerate(lens):
            rows = slice(cu[b], cu[b + 1])
            if b not in ids:
                assert torch.isnan(ctx[rows].float()).all(), f"class {c}: unlisted sequence {b} (len {n}) written"
                continue
            assert torch.isfinite(ctx[rows].float()).all(), f"class {c}: sequence {b} (len {n}) not finite"
            ratio = fwd._ctx_ratio(ctx[rows], ref[rows], A[rows])
            print(f"varlen relbias {batch} span {S} class {c} len {n}: ctx error {ratio:.3f} u A")
            assert ratio <= 2.5, f"class {c}: sequence {b} (len {n}) ctx error {ratio:.3f} u A > 2.5 u A"


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", [("short", 33), ("short", 160), ("long", 200)])
def test_varlen_relbias_bits_of_the_padded_kernel(dev, batch, n):
    """The packed rows of n tokens are the ctx bits of drt_attention_forward_bf16 at B = 1, L = n, L = n table."""
    from denseretrievaltoolkits_amd import _native
    lens, cu, qkv, table, S, _, _ = _case(batch, "512")
    b = lens.index(n)
    ids = _launches(lens)[(n + 31) // 32] if n <= 160 else None     # its class, as the tower launches it
    got = _run(dev, qkv, cu, table, S, ids, max(lens[i] for i in ids) if ids else max(lens))[cu[b]:cu[b + 1]]
    qd = qkv[cu[b]:cu[b + 1]].to(dev)
    td = table[:, S - n:S + n - 1].contiguous().to(dev)
    want = torch.full((n, H), float("nan"), dtype=torch.bfloat16, device=dev)
    _native.check(abi.forward(_native.load(), qd, want, 1, n, HEADS, relbias=td, scale=1.0), "attention_relbias")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.cpu().view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["short", "long"])
def test_varlen_relbias_zero_table_bits_of_the_varlen_kernel(dev, batch):
    lens, cu, qkv, table, S, _, _ = _case(batch, "512")
    got = _run(dev, qkv, cu, torch.zeros_like(table), S, None, max(lens))
    want = _run(dev, qkv, cu, None, S, None, max(lens), entry="drt_attention_varlen_forward_bf16")
    assert torch.isfinite(got.float()).all() and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
def test_varlen_relbias_clamps_length_to_max_len(dev):
    """A sequence longer than max_len attends over its first max_len tokens and writes those rows only."""
    lens, cu, qkv, table, S, _, _ = _case("short", "512")
    b, ml = lens.index(96), 64
    rows = qkv[cu[b]:cu[b + 1]]
    ctx = _run(dev, rows, [0, 96], table, S, None, ml)
    ref, A = tr.attention_relbias_ref(rows[:ml], None, table[:, S - ml:S + ml - 1], 1, ml, HEADS, 1.0)
    assert torch.isnan(ctx[ml:].float()).all()
    assert fwd._ctx_ratio(ctx[:ml], ref, A) <= 2.5


def test_entry_refuses_bad_arguments_before_any_device_work():
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()

    def call(n=3, max_len=64, relbias=P, bias_len=512, hd=64):
        return lib.drt_attention_varlen_relbias_forward_bf16(P, P, None, n, max_len, relbias, bias_len, P, 12, hd, 1.0,
                                                             None)

    E = _native.DRT_EINVAL
    assert call(max_len=64, bias_len=63) == E and call(bias_len=513) == E
    assert call(relbias=None) == E and call(hd=32) == E
    assert call(max_len=513, bias_len=513) == E and call(max_len=513) == E and call(n=0) == _native.DRT_OK

"""The inputs of the attention backward tests, shared by the CPU test of the bounds
(test_encoder_bwd_refs_cpu.py, on a torch emulation of the kernels' roundings) and the GPU test of the
kernels (test_encoder_bwd_fp64_gpu.py): masks and poisoned masked keys as in the forward test
(test_encoder_fwd_fp64_gpu.py), dO, keep masks and their packing into the kernels' drop_bits.
"""
import zlib

MASK_KINDS = ("null", "prefix", "left", "holes", "single")
DATA_KINDS = ("gauss", "peaked", "small")


# Elementwise bounds against tests/encoder_bwd_refs.py, in units of u A (u = 2^-8, A the output's error
# scale).  dV: P rounded to bf16 (u A_V) + the output rounding (u A_V) + the project's 0.5 u slack for the
# fp32 chain and the hardware exp2.  dQ, dK: dS rounded to bf16 (u A_S carried through the product) + D
# taken from the bf16 ctx (u P D_abs <= u A_S) + the output rounding + 0.5 u.  dtable is summed from the
# fp32 dS: the D term + 0.5 u for the fp32 sum.  With the forward kernel's own ctx D carries the forward's
# bound 2.5 u instead of u: 5 u for dQ, dK and 3 u for dtable.
BOUND_DV, BOUND_DQK, BOUND_DT, BOUND_DQK_FWD, BOUND_DT_FWD = 2.5, 3.5, 1.5, 5.0, 3.0
ATOL, ATOL_DT = 1e-7, 1e-6


def attention_ratios(dqkv, dtable, ref):
    """{"dQ", "dK", "dV"[, "dtable"]: worst (|err| - atol) / (u A)} of a backward's outputs against
    attention_bwd_ref's namespace; inf for a non-finite output or a non-zero where A = 0."""
    import encoder_bwd_refs as br
    H = ref.O.shape[1]
    out = {}
    for i, name in enumerate(("dQ", "dK", "dV")):
        sl = slice(i * H, (i + 1) * H)
        out[name] = br.bound_ratio(dqkv[:, sl], ref.dqkv[:, sl], ref.A[:, sl], ATOL)
    if dtable is not None:
        out["dtable"] = br.bound_ratio(dtable, ref.dtable, ref.A_T, ATOL_DT)
    return out


def over_bounds(ratios, dqk=BOUND_DQK, dt=BOUND_DT):
    """The entries of attention_ratios over their bound, as text."""
    lim = {"dQ": dqk, "dK": dqk, "dV": BOUND_DV, "dtable": dt}
    return [f"{n} error {r:.3f} u A > {lim[n]} u A" for n, r in ratios.items() if not r <= lim[n]]


def gen(*key):
    import torch
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def make_mask(kind, B, L, g):
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


def make_qkv_dctx(kind, B, L, heads, mask, g, keep_v=(), qk_scale=1.0):
    """(qkv [B*L, 3H], dctx [B*L, H]) in bf16.  Masked keys are poisoned (K x 50, V = 1e4, finite): a
    masked key leaking at any weight moves every gradient by orders of magnitude; sequences listed in
    keep_v keep their V.  A masked query row keeps its Q and its dO: its dQ is checked like any other.
    peaked: q, k x 3.  small: dO x 1e-2 on the last sequence, which a per-tensor norm would hide.
    qk_scale: a further factor on q and k (the relative-bias cases run scale = 1 with q, k x 0.35)."""
    import torch
    shape = (B, L, heads, 64)

    def bf(x):
        return x.to(torch.bfloat16).float()

    q, k, v, do = (torch.randn(shape, generator=g) for _ in range(4))
    if kind == "peaked":
        q, k = q * 3, k * 3
    elif kind == "small":
        do[B - 1] *= 1e-2
    elif kind != "gauss":
        raise ValueError(kind)
    q, k, v = bf(q * qk_scale), bf(k * qk_scale), bf(v)
    if mask is not None:
        dead = (mask == 0)[:, :, None, None]
        k = torch.where(dead, bf(k * 50), k)
        vdead = dead.clone()
        vdead[list(keep_v)] = False
        v = torch.where(vdead, torch.full_like(v, 1e4), v)
    H = heads * 64
    qkv = torch.cat([x.reshape(B * L, H) for x in (q, k, v)], 1).to(torch.bfloat16)
    return qkv, do.reshape(B * L, H).to(torch.bfloat16)


def make_keep(B, L, heads, p, mask, g, starve=False):
    """bool [B, heads, L, L], kept with probability 1 - p.  starve: query row L // 2 of every
    (sequence, head) has every live key dropped (its O is 0 and its dS = P (0 - 0))."""
    import torch
    keep = torch.rand(B, heads, L, L, generator=g) >= p
    if starve:
        live = torch.ones(B, L, dtype=torch.bool) if mask is None else mask != 0
        keep[:, :, L // 2, :] &= ~live[:, None, :]
    return keep


def pack_bits(keep):
    """drop_bits of include/drt.h from a bool [B, heads, L, L]: int32 [B, heads, L, ceil(L / 32)], bit
    key & 31 of word (query, key >> 5), bits of keys >= L zero."""
    import torch
    B, heads, L, _ = keep.shape
    nw = (L + 31) // 32
    kp = torch.zeros(B, heads, L, nw * 32, dtype=torch.int64)
    kp[..., :L] = keep.to(torch.int64)
    words = (kp.reshape(B, heads, L, nw, 32) << torch.arange(32)).sum(-1)      # < 2^32
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def emulate_attention_bwd(qkv_bf16, dctx_bf16, mask, B, L, heads, scale, ref, relbias=None, keep=None, p=0.0):
    """The backward kernels' roundings on top of fp64 arithmetic, from ctx = bf16(ref.O) and
    lse = fp32(ref.lse): P = exp(S - lse), D from the bf16 ctx, P and dS rounded to bf16 before the
    second products, one bf16 rounding of each output; dtable summed from the unrounded dS.  A
    sequence with every key masked: P = 1 / L over zeroed Qs and K.  Returns (dqkv bf16 [B*L, 3H],
    dtable fp64 or None)."""
    import torch
    qkv = qkv_bf16.detach().cpu()
    H = qkv.shape[1] // 3
    dh = H // heads

    def split(x):
        return x.reshape(B, L, heads, dh).transpose(1, 2)

    def merge(x):
        return x.transpose(1, 2).reshape(B * L, H)

    def bf(x):
        return x.to(torch.bfloat16).double()

    qs = split((qkv[:, :H].float() * scale).to(torch.bfloat16).double())
    k = split(qkv[:, H:2 * H].double())
    v = split(qkv[:, 2 * H:].double())
    do = split(dctx_bf16.detach().cpu().double())
    ctx = split(ref.O.to(torch.bfloat16).double())
    lse = ref.lse.float().double()
    live = torch.ones(B, L, dtype=torch.bool) if mask is None else mask != 0
    dead = ~live.any(1)
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
    inv = 1.0 / (1.0 - p) if keep is not None else 1.0
    dq, dk, dv = (torch.zeros(B, heads, L, dh, dtype=torch.float64) for _ in range(3))
    dts = torch.zeros(heads, L, L, dtype=torch.float64)
    for b in range(B):
        kp = torch.ones(heads, L, L, dtype=torch.float64) if keep is None else keep[b].double()
        if bool(dead[b]):
            pr = torch.full((heads, L, L), 1.0 / L, dtype=torch.float64)
            qb, kb = torch.zeros_like(qs[b]), torch.zeros_like(k[b])
        else:
            s = qs[b] @ k[b].transpose(-1, -2)
            if relbias is not None:
                s = s + relbias.double()[:, idx]
            s = s.masked_fill(~live[b][None, None, :], -float("inf"))
            pr = torch.exp(s - lse[b][:, :, None])
            qb, kb = qs[b], k[b]
        d = (do[b] * ctx[b]).sum(-1, keepdim=True)
        ds = pr * ((do[b] @ v[b].transpose(-1, -2)) * kp * inv - d)
        pa, sa = bf(pr * kp), bf(ds)
        dv[b] = (pa.transpose(-1, -2) @ do[b]) * inv
        dk[b] = sa.transpose(-1, -2) @ qb
        dq[b] = scale * (sa @ kb)
        if not bool(dead[b]):
            dts += ds
    dtable = None
    if relbias is not None:
        dtable = torch.zeros(heads, 2 * L - 1, dtype=torch.float64).index_add_(1, idx.reshape(-1), dts.reshape(heads, L * L))
    return torch.cat([merge(dq), merge(dk), merge(dv)], 1).to(torch.bfloat16), dtable

"""Plain fp64 references of the encoder backward kernels (torch CPU, no project kernels).

Every function takes the kernel's own inputs (bf16 / fp32 values, exactly representable in fp64),
computes the mathematical gradient in fp64 and returns CPU fp64 tensors together with the error
scales A the elementwise bounds are stated in.  tests/test_encoder_bwd_refs_cpu.py checks them
against torch.autograd in float64; tests/test_encoder_bwd_fp64_gpu.py checks the kernels against them.
"""
import math
from types import SimpleNamespace

FLT_MAX = 3.402823466e+38
U = 2.0 ** -8          # bf16's unit roundoff


def attention_bwd_ref(qkv_bf16, dctx_bf16, mask, B, L, heads, scale, relbias=None, keep=None, p=0.0):
    """The gradient of O = (softmax(Qs K^T + relbias + key mask) keep / (1 - p)) V by dO = dctx, per
    (sequence, head) of a packed [B*L, 3*H] bf16 QKV tensor (Q | K | V, head-major, head_dim = H / heads).

      Qs = bf16(Q scale) (as the kernels form it)      S = Qs K^T + relbias[h][k - q + L - 1], masked keys -inf
      P = softmax(S)     Pd = P keep / (1 - p)         O = Pd V
      dP = (dO V^T) keep / (1 - p)    D = sum_j dO_j O_j      dS = P (dP - D)
      dV = Pd^T dO       dQ = scale dS K       dK = dS^T Qs
      dtable[h][d + L - 1] = sum over (b, q, k with k - q = d) of dS

    keep: bool [B, heads, L, L] or None (all kept; p is then ignored).  A sequence with every key
    masked follows the contract of include/drt.h: P is uniform over its L keys whatever Q, K and
    relbias hold, so dQ, dK and its share of dtable are zero and dV = sum_q keep dO_q / (L (1 - p)).

    Returns a namespace of fp64 tensors: dqkv [B*L, 3H] (dQ | dK | dV), O [B*L, H], lse [B, heads, L]
    (dead sequences: ln L - FLT_MAX ln 2, as the forward reference), dtable [heads, 2L-1] (None without
    relbias), and the error scales A [B*L, 3H] (A_Q | A_K | A_V) and A_T [heads, 2L-1]:
      A_O = Pd |V|    D_abs = sum_j |dO_j| A_O,j    A_S = P (|dP| + D_abs)
      A_V = Pd^T |dO|    A_Q = scale A_S |K|    A_K = A_S^T |Qs|    A_T = diagonal sums of A_S.
    """
    import torch
    qkv = qkv_bf16.detach().cpu()
    H = qkv.shape[1] // 3
    dh = H // heads
    assert qkv.shape == (B * L, 3 * H) and dh * heads == H and dctx_bf16.shape == (B * L, H)

    def split(x):   # [B*L, H] -> [B, heads, L, dh]
        return x.reshape(B, L, heads, dh).transpose(1, 2)

    def merge(x):   # [B, heads, L, dh] -> [B*L, H]
        return x.transpose(1, 2).reshape(B * L, H)

    qs = split((qkv[:, :H].float() * scale).to(torch.bfloat16).double())
    k = split(qkv[:, H:2 * H].double())
    v = split(qkv[:, 2 * H:].double())
    do = split(dctx_bf16.detach().cpu().double())
    live = torch.ones(B, L, dtype=torch.bool) if mask is None else mask.detach().cpu() != 0
    dead = ~live.any(1)
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1          # [q, k] -> k - q + L - 1
    rb = None if relbias is None else relbias.detach().cpu().double()[:, idx]   # [heads, L, L]
    kf_all = None if keep is None else keep.detach().cpu().double() / (1.0 - p)

    out = {n: torch.zeros(B, heads, L, dh, dtype=torch.float64) for n in ("dq", "dk", "dv", "o", "aq", "ak", "av")}
    lse = torch.zeros(B, heads, L, dtype=torch.float64)
    dts = torch.zeros(heads, L, L, dtype=torch.float64)
    ats = torch.zeros(heads, L, L, dtype=torch.float64)
    for b in range(B):                                   # one sequence at a time: [heads, L, L] temporaries
        if bool(dead[b]):
            s = torch.zeros(heads, L, L, dtype=torch.float64)
            lse[b] = math.log(L) - FLT_MAX * math.log(2.0)
        else:
            s = qs[b] @ k[b].transpose(-1, -2)
            if rb is not None:
                s = s + rb
            s = s.masked_fill(~live[b][None, None, :], -math.inf)
            lse[b] = torch.logsumexp(s, -1)
        pr = torch.softmax(s, -1)
        kf = 1.0 if kf_all is None else kf_all[b]
        pd = pr * kf
        o = pd @ v[b]
        a_o = pd @ v[b].abs()
        dp = (do[b] @ v[b].transpose(-1, -2)) * kf
        d = (do[b] * o).sum(-1, keepdim=True)
        d_abs = (do[b].abs() * a_o).sum(-1, keepdim=True)
        ds = pr * (dp - d)
        a_s = pr * (dp.abs() + d_abs)
        out["o"][b] = o
        out["dv"][b] = pd.transpose(-1, -2) @ do[b]
        out["av"][b] = pd.transpose(-1, -2) @ do[b].abs()
        if not bool(dead[b]):
            out["dq"][b] = scale * (ds @ k[b])
            out["aq"][b] = scale * (a_s @ k[b].abs())
            out["dk"][b] = ds.transpose(-1, -2) @ qs[b]
            out["ak"][b] = a_s.transpose(-1, -2) @ qs[b].abs()
            dts += ds
            ats += a_s

    def diag_sums(x):   # [heads, L, L] -> [heads, 2L-1]
        return torch.zeros(heads, 2 * L - 1, dtype=torch.float64).index_add_(1, idx.reshape(-1), x.reshape(heads, L * L))

    return SimpleNamespace(
        dqkv=torch.cat([merge(out["dq"]), merge(out["dk"]), merge(out["dv"])], 1),
        O=merge(out["o"]), lse=lse,
        dtable=None if relbias is None else diag_sums(dts),
        A=torch.cat([merge(out["aq"]), merge(out["ak"]), merge(out["av"])], 1),
        A_T=diag_sums(ats))


def layernorm_bwd_ref(dy, x, gamma, eps, dres=None):
    """The gradient of y = LayerNorm(x) gamma + beta by dy, plus a residual gradient, in fp64:
      g = gamma dy    xhat = (x - mean) rstd
      dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres     dgamma = sum_rows dy xhat     dbeta = sum_rows dy.
    Returns a namespace: dx [M, H], dgamma, dbeta [H], their sums of absolute terms dgamma_abs, dbeta_abs
    (the scale of a summation error) and A_LN = rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |dres|."""
    dy = dy.detach().cpu().double()
    x = x.detach().cpu().double()
    gm = gamma.detach().cpu().double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)             # biased, as nn.LayerNorm
    rstd = 1.0 / (var + eps).sqrt()
    xhat = (x - mean) * rstd
    g = dy * gm
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    a = rstd * (g.abs() + g.abs().mean(1, keepdim=True) + xhat.abs() * (g * xhat).abs().mean(1, keepdim=True))
    if dres is not None:
        r = dres.detach().cpu().double()
        dx = dx + r
        a = a + r.abs()
    return SimpleNamespace(dx=dx, dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0), dgamma_abs=(dy * xhat).abs().sum(0),
                           dbeta_abs=dy.abs().sum(0), A_LN=a)


def bound_ratio(got, ref, A, atol):
    """max over elements of (|got - ref| - atol) / (u A), the figure an "err <= c u A + atol" bound is
    asserted on (ratio <= c).  Where A is exactly 0 nothing may round: got must be exactly 0 there,
    else the ratio is inf.  NaN in got gives inf."""
    import torch
    got = got.detach().cpu().double()
    if not torch.isfinite(got).all():
        return math.inf
    zero = A == 0
    if bool((got[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    err = ((got - ref).abs() - atol).clamp(min=0)[~zero]
    return float((err / (U * A[~zero])).max())

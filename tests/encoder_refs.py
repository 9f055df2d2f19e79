"""Plain fp64 references of the encoder forward kernels (torch CPU, no project kernels).

Every function takes the kernel's own inputs (bf16 / fp32 values, exactly representable in fp64),
computes the mathematical result in fp64 and returns CPU fp64 tensors.  tests/test_encoder_refs_cpu.py
checks them against HF BERT in .double(); tests/test_encoder_fwd_fp64_gpu.py checks the kernels
against them.
"""
import math

FLT_MAX = 3.402823466e+38


def attention_ref(qkv_bf16, mask, B, L, heads, scale):
    """softmax(Q K^T scale + key mask) V per (sequence, head) of a packed [B*L, 3*H] bf16 QKV tensor
    (Q | K | V, head-major inside each, head_dim = H / heads).

    Returns (ctx [B*L, H], A [B*L, H], lse [B, heads, L]) in fp64.  Q is scaled and rounded to bf16
    first, as the kernel does (exact for scale = 1/8); everything after is fp64 with masked keys at
    -inf.  A = P |V| is the scale of the kernel's rounding errors.  A row whose every key is masked is
    defined as the uniform mean over its L keys (HF's softmax of L equal finfo.min scores); its lse is
    ln L - FLT_MAX ln 2, finite and otherwise meaningless.
    """
    import torch
    qkv = qkv_bf16.detach().cpu()
    H = qkv.shape[1] // 3
    dh = H // heads
    assert qkv.shape == (B * L, 3 * H) and dh * heads == H

    def split(x):   # [B*L, H] -> [B, heads, L, dh]
        return x.reshape(B, L, heads, dh).transpose(1, 2)

    q = split((qkv[:, :H].float() * scale).to(torch.bfloat16).double())
    k = split(qkv[:, H:2 * H].double())
    v = split(qkv[:, 2 * H:].double())
    s = q @ k.transpose(-1, -2)                                   # [B, heads, L, L]
    keep = torch.ones(B, L, dtype=torch.bool) if mask is None else mask.detach().cpu() != 0
    dead = ~keep.any(1)                                           # sequences with every key masked
    keep_eff = keep | dead[:, None]
    s = s.masked_fill(~keep_eff[:, None, None, :], -math.inf)
    if dead.any():
        s[dead] = 0.0                                             # uniform over the L keys
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    if dead.any():
        lse[dead] = math.log(L) - FLT_MAX * math.log(2.0)

    def merge(x):   # [B, heads, L, dh] -> [B*L, H]
        return x.transpose(1, 2).reshape(B * L, H)

    return merge(p @ v), merge(p @ v.abs()), lse


def embed_sum(ids, type_ids, L, word, pos, typ, dtype):
    """(word[id] + type[tt]) + pos[t % L] in ``dtype``, HF's order of the two additions; [T, H]."""
    import torch
    ids = ids.detach().cpu().reshape(-1)
    T = ids.numel()
    tt = torch.zeros(T, dtype=torch.int64) if type_ids is None else type_ids.detach().cpu().reshape(-1)
    p = torch.arange(T) % L
    w, po, ty = (x.detach().cpu().to(dtype) for x in (word, pos, typ))
    return (w[ids] + ty[tt]) + po[p]


def embed_ln_ref(ids, type_ids, L, word, pos, typ, gamma, beta, eps):
    """BertEmbeddings: LayerNorm((word[id] + type[tt]) + pos[t % L]) in fp64; [T, H].
    type_ids None = token type 0 everywhere."""
    import torch
    x = embed_sum(ids, type_ids, L, word, pos, typ, torch.float64)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)                 # biased, as nn.LayerNorm
    return (x - mean) / torch.sqrt(var + eps) * gamma.detach().cpu().double() + beta.detach().cpu().double()


def pool_ref(hidden, mask, mode):
    """Pooling of hidden [B, L, H] under mask [B, L] (None = all ones), fp64 [B, H]:
    mode 0 = first token, 1 = sum(h m) / max(sum m, 1e-9), 2 = max over l of h m (HF's max of
    hidden * mask: a masked token contributes 0)."""
    import torch
    h = hidden.detach().cpu().double()
    B, L, _ = h.shape
    m = torch.ones(B, L, dtype=torch.float64) if mask is None else mask.detach().cpu().double()
    if mode == 0:
        return h[:, 0, :].clone()
    hm = h * m[:, :, None]
    if mode == 1:
        return hm.sum(1) / m.sum(1, keepdim=True).clamp(min=1e-9)
    if mode == 2:
        return hm.max(1)[0]
    raise ValueError(mode)


def l2_ref(x):
    """F.normalize(x, dim=1): x / max(||x||, 1e-12), fp64."""
    x = x.detach().cpu().double()
    return x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)

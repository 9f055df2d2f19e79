"""Plain fp64 references of the T5 encoder kernels (torch CPU, no project kernels), and the small
T5EncoderModel configurations the T5 tests share.

As tests/encoder_refs.py: every function takes the kernel's own inputs (bf16 / fp32 values, exactly
representable in fp64), computes the mathematical result in fp64 and returns CPU fp64 tensors.
"""
import math

# (d_model, layers, heads, d_ff, feed_forward_proj, B, L): vocab 1024, d_kv 64; heads * 64 differs
# from d_model in the second one (T5 v1.1-small has 6 heads at d_model 512)
T5_CASES = [
    (256, 2, 4, 512, "relu", 3, 300),
    (256, 2, 2, 512, "gated-gelu", 3, 160),
    (512, 2, 8, 1024, "gated-gelu", 5, 17),
    (768, 12, 12, 3072, "relu", 4, 128),
]
VOCAB = 1024


def t5_config(d_model, layers, heads, d_ff, act, d_kv=64):
    from transformers import T5Config
    return T5Config(vocab_size=VOCAB, d_model=d_model, d_kv=d_kv, d_ff=d_ff, num_layers=layers, num_heads=heads,
                    feed_forward_proj=act, dropout_rate=0.0, pad_token_id=0)


def t5_model(cfg, seed=0):
    """T5EncoderModel in eval mode with HF's seeded init; block 0's relative-attention bias is redrawn
    as N(0, 1.5^2) (HF's init has std ~ 0.06: a kernel that ignored the bias could still pass)."""
    import torch
    from transformers import T5EncoderModel
    torch.manual_seed(seed)
    m = T5EncoderModel(cfg).eval()
    w = m.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        w.copy_(1.5 * torch.randn(w.shape, generator=g))
    return m


def t5_batch(B, L, seed):
    """ids int64 [B, L] in [1, VOCAB) and the mask: sequence 0 full, 1 a prefix of L / 2, 2 a prefix
    of 5 (the rest full); pad id 0 under masked positions."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, VOCAB, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.int64)
    if B > 1:
        mask[1, max(1, L // 2):] = 0
    if B > 2:
        mask[2, min(5, L):] = 0
    return ids * mask, mask


def rmsnorm_ref(x, weight, eps):
    """T5LayerNorm: x / sqrt(mean(x^2) + eps) * weight in fp64; [M, H]."""
    x = x.detach().cpu().double()
    return x / (x.pow(2).mean(1, keepdim=True) + eps).sqrt() * weight.detach().cpu().double()


def gelu_new_ref(a):
    """transformers NewGELUActivation in fp64."""
    import torch
    a = a.detach().cpu().double()
    return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a.pow(3))))


def expand_bias(table, L):
    """[heads, 2L-1] over k - q  ->  [heads, L(q), L(k)]."""
    import torch
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
    return table[:, idx]


def attention_relbias_ref(qkv_bf16, mask, table, B, L, heads, scale):
    """softmax(Q K^T scale + table[h][k - q + L - 1] + key mask) V per (sequence, head) of a packed
    [B*L, 3*heads*64] bf16 QKV tensor; table fp32 [heads, 2L-1].  Returns (ctx, A = P |V|), fp64
    [B*L, heads*64].  As encoder_refs.attention_ref: Q is scaled and rounded to bf16 first (exact for a
    power of two), masked keys are at -inf, and a sequence whose every key is masked gets the uniform
    mean over its L keys (finfo.min absorbs scores and biases in HF's fp32 sum)."""
    import torch
    qkv = qkv_bf16.detach().cpu()
    H = qkv.shape[1] // 3
    dh = H // heads
    assert qkv.shape == (B * L, 3 * H) and dh * heads == H and table.shape == (heads, 2 * L - 1)

    def split(x):   # [B*L, H] -> [B, heads, L, dh]
        return x.reshape(B, L, heads, dh).transpose(1, 2)

    q = split((qkv[:, :H].float() * scale).to(torch.bfloat16).double())
    k = split(qkv[:, H:2 * H].double())
    v = split(qkv[:, 2 * H:].double())
    s = q @ k.transpose(-1, -2) + expand_bias(table.detach().cpu().double(), L)[None]
    keep = torch.ones(B, L, dtype=torch.bool) if mask is None else mask.detach().cpu() != 0
    dead = ~keep.any(1)
    s = s.masked_fill(~(keep | dead[:, None])[:, None, None, :], -math.inf)
    if dead.any():
        s[dead] = 0.0
    p = torch.softmax(s, -1)

    def merge(x):   # [B, heads, L, dh] -> [B*L, H]
        return x.transpose(1, 2).reshape(B * L, H)

    return merge(p @ v), merge(p @ v.abs())

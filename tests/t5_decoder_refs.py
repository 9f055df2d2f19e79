"""Plain fp64 references of the one-step T5 decoder (torch CPU, no project kernels), and the small
T5ForConditionalGeneration configurations the decoder tests share.

As tests/t5_refs.py: every kernel reference takes the kernel's own bf16 inputs (exactly representable
in fp64) and returns CPU fp64 tensors.  ``decoder_step_ref`` is the absorbed formula of
model/t5_decoder.py over an HF module's own fp32 weights.
"""
import math

import t5_refs as tr

# (d_model, encoder layers, decoder layers, heads, d_ff, feed_forward_proj, B, L)
S2S_CASES = [
    (256, 2, 2, 4, 512, "relu", 4, 70),
    (512, 2, 3, 6, 1024, "gated-gelu", 4, 37),
    (768, 12, 12, 12, 3072, "relu", 4, 128),
]
CROSS_Q_GAIN = 4.0


def s2s_config(d_model, enc_layers, dec_layers, heads, d_ff, act, d_kv=64, scale_outputs=True):
    from transformers import T5Config
    kw = {} if scale_outputs else {"tie_word_embeddings": False}     # how T5Config spells "no output scale"
    return T5Config(vocab_size=tr.VOCAB, d_model=d_model, d_kv=d_kv, d_ff=d_ff, num_layers=enc_layers,
                    num_decoder_layers=dec_layers, num_heads=heads, feed_forward_proj=act, dropout_rate=0.0,
                    pad_token_id=0, decoder_start_token_id=0, attn_implementation="eager", **kw)


def s2s_model(cfg, seed=0, untie=False):
    """T5ForConditionalGeneration in eval mode with HF's seeded init; block 0's encoder bias redrawn as
    in t5_refs.t5_model; every EncDecAttention.q.weight times 4 (HF's init leaves the cross-attention
    near uniform: a scorer that ignored the scores could still pass).  untie: lm_head gets its own
    N(0, 1) weight instead of shared.weight."""
    import torch
    from transformers import T5ForConditionalGeneration
    torch.manual_seed(seed)
    m = T5ForConditionalGeneration(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        w = m.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        w.copy_(1.5 * torch.randn(w.shape, generator=g))
        for blk in m.decoder.block:
            blk.layer[1].EncDecAttention.q.weight.mul_(CROSS_Q_GAIN)
        if untie:
            m.lm_head.weight = torch.nn.Parameter(torch.randn(m.lm_head.weight.shape, generator=g))
    return m


def output_scale(cfg):
    scaled = cfg.scale_decoder_outputs if hasattr(cfg, "scale_decoder_outputs") else cfg.tie_word_embeddings
    return float(cfg.d_model) ** -0.5 if scaled else 1.0


def hf_step(model, ids, mask, attentions=False):
    """The HF module's own one-step forward: (logits[:, 0, :], decoder_hidden_states[-1][:, 0],
    encoder last_hidden_state, cross attentions or None)."""
    import torch
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, decoder_input_ids=torch.zeros((ids.shape[0], 1), dtype=torch.long),
                    output_hidden_states=True, output_attentions=attentions, return_dict=True)
    return (out.logits[:, 0], out.decoder_hidden_states[-1][:, 0], out.encoder_last_hidden_state,
            out.cross_attentions if attentions else None)


def cross_entropy_fraction(cross_attentions, L):
    """Per decoder layer: the mean over heads of the softmax entropy of sequence 0 (unmasked) over
    ln L."""
    out = []
    for a in cross_attentions:          # [B, heads, 1, L]
        p = a[0, :, 0, :].double()
        ent = -(p * p.clamp(min=1e-300).log()).sum(-1)
        out.append(float(ent.mean()) / math.log(L))
    return out


# ---------------------------------------------------------------------------------------------
# kernel references
# ---------------------------------------------------------------------------------------------
def head_expand_ref(q, Wk, heads):
    """qt[b, h, :] = sum_j q[b, 64h+j] Wk[64h+j, :]; q [B, heads*64], Wk [heads*64, D] -> [B, heads, D]."""
    import torch
    q = q.detach().cpu().double()
    w = Wk.detach().cpu().double()
    B, D = q.shape[0], w.shape[1]
    return torch.einsum("bhj,hjd->bhd", q.reshape(B, heads, 64), w.reshape(heads, 64, D))


def head_reduce_ref(pooled, Wv, heads):
    """ctx[b, 64h+j] = Wv[64h+j, :] . pooled[b, h, :]; pooled [B, heads, D] -> [B, heads*64]."""
    import torch
    p = pooled.detach().cpu().double()
    w = Wv.detach().cpu().double()
    B, D = p.shape[0], w.shape[1]
    return torch.einsum("bhd,hjd->bhj", p.reshape(B, heads, D), w.reshape(heads, 64, D)).reshape(B, heads * 64)


def cross_pool_ref(qt, enc, mask, uniform=False):
    """p = softmax_l(qt[b, h] . enc[b, l] + key mask), pooled = p enc.  qt [B, heads, D], enc [B, L, D],
    mask int64 [B, L] or None.  Returns (pooled, A = p |enc|), fp64 [B, heads, D].  Masked keys are at
    -inf (their enc rows never enter, whatever they hold); a sequence whose every key is masked gets
    the uniform mean over its L keys.  uniform: every live key gets the same weight (the negative
    control of the reranker tests)."""
    import torch
    q = qt.detach().cpu().double()
    e = enc.detach().cpu().double()
    B, L, _ = e.shape
    keep = torch.ones(B, L, dtype=torch.bool) if mask is None else mask.detach().cpu() != 0
    dead = ~keep.any(1)
    live = keep | dead[:, None]
    e = torch.where(live[:, :, None], e, torch.zeros_like(e))      # p = 0 there: keep 0 * poison out of fp64 too
    s = torch.einsum("bhd,bld->bhl", q, e)
    if uniform:
        s = torch.zeros_like(s)
    s = s.masked_fill(~live[:, None, :], -math.inf)
    if dead.any():
        s[dead] = 0.0
    p = torch.softmax(s, -1)
    return torch.einsum("bhl,bld->bhd", p, e), torch.einsum("bhl,bld->bhd", p, e.abs())


# ---------------------------------------------------------------------------------------------
# the absorbed decoder step over an HF module's weights
# ---------------------------------------------------------------------------------------------
def decoder_step_ref(model, enc, mask, uniform=False):
    """(y [B, D], logits [B, vocab]) in fp64: the one-token decoder step in absorbed form over
    enc = the module's encoder last_hidden_state [B, L, D], from the module's own weights."""
    import torch
    cfg = model.config
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    heads, eps = cfg.num_heads, cfg.layer_norm_epsilon
    gated = cfg.feed_forward_proj == "gated-gelu"
    enc = enc.detach().double()
    B = enc.shape[0]

    def rms(x, w):
        return x / (x.pow(2).mean(-1, keepdim=True) + eps).sqrt() * w

    h = sd["shared.weight"][0][None, :].expand(B, -1).clone()
    for i in range(cfg.num_decoder_layers):
        p = f"decoder.block.{i}.layer."
        x = rms(h, sd[p + "0.layer_norm.weight"])
        h = h + (x @ sd[p + "0.SelfAttention.v.weight"].T) @ sd[p + "0.SelfAttention.o.weight"].T
        x = rms(h, sd[p + "1.layer_norm.weight"])
        q = x @ sd[p + "1.EncDecAttention.q.weight"].T
        qt = head_expand_ref(q, sd[p + "1.EncDecAttention.k.weight"], heads)
        pooled, _ = cross_pool_ref(qt, enc, mask, uniform=uniform)
        c = head_reduce_ref(pooled, sd[p + "1.EncDecAttention.v.weight"], heads)
        h = h + c @ sd[p + "1.EncDecAttention.o.weight"].T
        x = rms(h, sd[p + "2.layer_norm.weight"])
        if gated:
            f = tr.gelu_new_ref(x @ sd[p + "2.DenseReluDense.wi_0.weight"].T) * (x @ sd[p + "2.DenseReluDense.wi_1.weight"].T)
        else:
            f = torch.relu(x @ sd[p + "2.DenseReluDense.wi.weight"].T)
        h = h + f @ sd[p + "2.DenseReluDense.wo.weight"].T
    y = rms(h, sd["decoder.final_layer_norm.weight"])
    return y, output_scale(cfg) * y @ sd["lm_head.weight"].T

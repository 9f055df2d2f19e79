"""Host side of the T5 tower (no GPU): the relative-position bias table against HF's own
compute_bias, the supported-configuration check, and the new C entries' shape validation."""
import ctypes

import pytest

import t5_refs as tr


@pytest.mark.parametrize("buckets,max_distance", [(32, 128), (8, 20)])
@pytest.mark.parametrize("L", [1, 2, 9, 17, 129, 300, 512])
def test_relative_bias_table_equals_hf_compute_bias(L, buckets, max_distance):
    """table[h, k - q + L - 1] == T5Attention.compute_bias(L, L)[0, h, q, k], bit for bit in fp32."""
    import torch
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention
    from denseretrievaltoolkits_amd.model.t5_encoder import relative_bias_table
    heads = 3
    cfg = T5Config(d_model=64 * heads, d_kv=64, num_heads=heads, relative_attention_num_buckets=buckets,
                   relative_attention_max_distance=max_distance)
    att = T5Attention(cfg, has_relative_attention_bias=True)
    g = torch.Generator().manual_seed(1000 * buckets + L)
    with torch.no_grad():
        att.relative_attention_bias.weight.copy_(1.5 * torch.randn(buckets, heads, generator=g))
        want = att.compute_bias(L, L)[0]
    table = relative_bias_table(att.relative_attention_bias.weight, L, buckets, max_distance)
    assert table.shape == (heads, 2 * L - 1) and table.dtype == torch.float32
    got = tr.expand_bias(table, L)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_t5_supported():
    from transformers import BertConfig, BertModel, T5EncoderModel
    from denseretrievaltoolkits_amd.model.t5_encoder import t5_supported
    for d_model, layers, heads, d_ff, act, _, _ in tr.T5_CASES:
        assert t5_supported(T5EncoderModel(tr.t5_config(d_model, 1, heads, d_ff, act))) is None
    why = t5_supported(T5EncoderModel(tr.t5_config(256, 1, 4, 512, "relu", d_kv=32)))
    assert why is not None and "d_kv" in why
    why = t5_supported(T5EncoderModel(tr.t5_config(320, 1, 5, 512, "relu")))
    assert why is not None and "d_model" in why
    why = t5_supported(T5EncoderModel(tr.t5_config(256, 1, 4, 512, "gated-silu")))
    assert why is not None and "gated-silu" in why
    bert = BertModel(BertConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64,
                                vocab_size=100), add_pooling_layer=False)
    why = t5_supported(bert)
    assert why is not None and "BertModel" in why


def test_new_entries_reject_bad_shapes_without_gpu():
    """DRT_EINVAL before any HIP call (null pointers: a launch would have faulted, not returned)."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    E = _native.DRT_EINVAL
    att = lib.drt_attention_forward_bf16
    assert att(None, None, None, None, None, None, 2, 16, 4, 32, 1.0, 0.0, 0, 0, None) == E    # head_dim != 64
    assert att(None, None, None, None, None, None, 2, 0, 4, 64, 1.0, 0.0, 0, 0, None) == E     # L = 0
    assert att(None, None, None, None, None, None, 2, 513, 4, 64, 1.0, 0.0, 0, 0, None) == E   # L > 512
    att = lib.drt_attention_relbias_bf16                                    # the earlier name forwards
    assert att(None, None, None, None, 2, 16, 4, 32, 1.0, None) == E        # head_dim != 64
    assert att(None, None, None, None, 2, 0, 4, 64, 1.0, None) == E         # L = 0
    assert att(None, None, None, None, 2, 513, 4, 64, 1.0, None) == E       # L > 512
    assert lib.drt_rmsnorm_bf16(None, 4, 320, None, 1e-6, None, None) == E  # H % 256
    assert lib.drt_rmsnorm_bf16(None, 4, 1280, None, 1e-6, None, None) == E
    assert lib.drt_t5_embed_bf16(None, 2, 0, None, 256, None, None) == E
    assert lib.drt_t5_embed_bf16(None, 2, 8, None, 258, None, None) == E
    assert lib.drt_gated_gelu_new_bf16(None, 4, 12, None, None) == E
    # ReLU (8) with GELU (1), and ReLU with fp32 output (2): with null pointers, and with non-null
    # ones (never dereferenced on the host), so that it is the flags that are refused
    assert lib.drt_linear_bf16(None, None, None, None, None, 4, 64, 64, 8 | 1, None) == E
    assert lib.drt_linear_bf16_ws(None, None, None, None, None, 4, 64, 64, 8 | 1, None, 0, None) == E
    buf = ctypes.create_string_buffer(64 * 64 * 2)
    p = ctypes.addressof(buf)
    assert lib.drt_linear_bf16(p, p, None, None, p, 4, 64, 64, 8 | 1, None) == E
    assert lib.drt_linear_bf16(p, p, None, None, p, 4, 64, 64, 8 | 2, None) == E

"""Host side of the T5 reranker (no GPU): the supported-configuration check, the new C entries'
shape validation, and the absorbed one-step decoder formula against the HF module itself."""
import pytest

import t5_decoder_refs as dr
import t5_refs as tr


def test_t5_seq2seq_supported():
    from transformers import BertConfig, BertModel, T5EncoderModel, T5ForConditionalGeneration
    from denseretrievaltoolkits_amd.model.t5_decoder import t5_seq2seq_supported
    for d_model, _, dec_layers, heads, d_ff, act, _, _ in dr.S2S_CASES:
        # one encoder layer, the case's decoder depth capped at 2: the check reads the config only
        cfg = dr.s2s_config(d_model, 1, min(dec_layers, 2), heads, d_ff, act)
        assert t5_seq2seq_supported(T5ForConditionalGeneration(cfg)) is None
    why = t5_seq2seq_supported(T5ForConditionalGeneration(dr.s2s_config(256, 1, 1, 4, 512, "relu", d_kv=32)))
    assert why is not None and "d_kv" in why
    why = t5_seq2seq_supported(T5ForConditionalGeneration(dr.s2s_config(256, 1, 1, 20, 512, "relu")))
    assert why is not None and "heads" in why
    why = t5_seq2seq_supported(T5ForConditionalGeneration(dr.s2s_config(256, 1, 1, 4, 512, "gated-silu")))
    assert why is not None and "gated-silu" in why
    why = t5_seq2seq_supported(T5EncoderModel(tr.t5_config(256, 1, 4, 512, "relu")))
    assert why is not None and "T5EncoderModel" in why
    bert = BertModel(BertConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64,
                                vocab_size=100), add_pooling_layer=False)
    why = t5_seq2seq_supported(bert)
    assert why is not None and "BertModel" in why


def test_decoder_entries_reject_bad_shapes_without_gpu():
    """DRT_EINVAL before any HIP call (null pointers: a launch would have faulted, not returned)."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    E = _native.DRT_EINVAL
    pool = lib.drt_t5_cross_pool_bf16
    assert pool(None, None, None, None, 2, 0, 4, 256, None) == E        # L = 0
    assert pool(None, None, None, None, 2, 513, 4, 256, None) == E      # L > 512
    assert pool(None, None, None, None, 2, 16, 17, 256, None) == E      # heads > 16
    assert pool(None, None, None, None, 2, 16, 4, 320, None) == E       # D % 256
    assert pool(None, None, None, None, 2, 16, 4, 256, None) == E       # null pointers with a good shape
    for fn in (lib.drt_t5_head_expand_bf16, lib.drt_t5_head_reduce_bf16):
        assert fn(None, None, None, 2, 17, 256, None) == E
        assert fn(None, None, None, 2, 0, 256, None) == E
        assert fn(None, None, None, 2, 4, 320, None) == E
        assert fn(None, None, None, 2, 4, 1280, None) == E
        assert fn(None, None, None, 2, 4, 256, None) == E


@pytest.mark.parametrize("case", dr.S2S_CASES[:2], ids=lambda c: f"d{c[0]}-{c[5]}")
def test_absorbed_formula_equals_hf_fp32(case):
    """The fp64 absorbed step over the HF module's own fp32 weights and encoder output reproduces
    HF fp32 logits[:, 0, :] and the final decoder state to 1e-4 (the remainder is HF's fp32
    arithmetic): self-attention over one key is the v/o product, T5 scales no score, the
    cross-attention bias is zero, and the output scale is the config's."""
    import torch
    d_model, enc_layers, dec_layers, heads, d_ff, act, B, L = case
    model = dr.s2s_model(dr.s2s_config(d_model, enc_layers, dec_layers, heads, d_ff, act))
    ids, mask = tr.t5_batch(B, L, seed=11)
    logits, hidden, enc, _ = dr.hf_step(model, ids, mask)
    y, ref = dr.decoder_step_ref(model, enc, mask)
    print(f"d_model {d_model} {act}: logits rms {float(logits.pow(2).mean().sqrt()):.3f}, worst |ref - HF| "
          f"{float((ref - logits.double()).abs().max()):.2e}, hidden {float((y - hidden.double()).abs().max()):.2e}")
    torch.testing.assert_close(ref, logits.double(), atol=1e-4, rtol=0)
    torch.testing.assert_close(y, hidden.double(), atol=1e-4, rtol=0)

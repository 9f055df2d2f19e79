"""Host side of the T5 training tower (no GPU): the support check's reasons, the differentiable
relative-position bias table against autograd through HF's own compute_bias, DRModel's opt-in
flag, and the new C entries' shape validation."""
import ctypes
from types import SimpleNamespace

import pytest

import t5_refs as tr


def test_t5_tower_supported_reasons():
    from transformers import BertConfig, BertModel, T5EncoderModel
    from denseretrievaltoolkits_amd.model.t5_train_tower import t5_tower_supported
    ok = T5EncoderModel(tr.t5_config(256, 1, 4, 512, "relu"))
    assert t5_tower_supported(ok) is None and t5_tower_supported(ok, 512) is None
    why = t5_tower_supported(ok, 513)
    assert why is not None and "513" in why
    why = t5_tower_supported(T5EncoderModel(tr.t5_config(256, 1, 4, 512, "relu", d_kv=32)))
    assert why is not None and "d_kv 32" in why
    why = t5_tower_supported(T5EncoderModel(tr.t5_config(384, 1, 6, 512, "gated-gelu")), 16)
    assert why is not None and "d_model 384" in why
    bert = BertModel(BertConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64,
                                vocab_size=100), add_pooling_layer=False)
    assert "BertModel" in t5_tower_supported(bert)


@pytest.mark.parametrize("L", [5, 32, 200])
def test_differentiable_table_folds_into_the_bucket_weights(L):
    """For a random upstream dtable [heads, 2L-1], the gradient that reaches
    relative_attention_bias.weight through relative_bias_table_grad equals autograd through HF's
    T5Attention.compute_bias(L, L) under the upstream expanded over (q, k): every (q, k) of a diagonal
    shares one table entry, so the expanded upstream of entry d is dtable[d] / (entries on d)."""
    import torch
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention
    from denseretrievaltoolkits_amd.model.t5_encoder import relative_bias_table
    from denseretrievaltoolkits_amd.model.t5_train_tower import relative_bias_table_grad
    heads, buckets, maxd = 3, 32, 128
    cfg = T5Config(d_model=64 * heads, d_kv=64, num_heads=heads, relative_attention_num_buckets=buckets,
                   relative_attention_max_distance=maxd)
    att = T5Attention(cfg, has_relative_attention_bias=True).double()
    w = att.relative_attention_bias.weight
    g = torch.Generator().manual_seed(L)
    with torch.no_grad():
        w.copy_(1.5 * torch.randn(buckets, heads, generator=g, dtype=torch.float64))
    up = torch.randn(heads, 2 * L - 1, generator=g, dtype=torch.float64)
    # HF side: the per-(q, k) upstream whose diagonal sums are `up`
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1          # [q, k] -> table entry
    count = torch.bincount(idx.flatten(), minlength=2 * L - 1).double()
    up_qk = (up / count)[:, idx]                                               # [heads, L, L]
    (att.compute_bias(L, L)[0] * up_qk).sum().backward()
    want = w.grad.clone()
    w.grad = None
    table = relative_bias_table_grad(w, L, buckets, maxd)
    assert table.shape == (heads, 2 * L - 1) and table.requires_grad
    # the same values as the inference table (fp32 of the weights)
    assert torch.equal(table.detach(), relative_bias_table(w, L, buckets, maxd))
    (table.double() * up).sum().backward()
    torch.testing.assert_close(w.grad, want, atol=1e-5, rtol=1e-5)   # the table is fp32: one cast per entry
    # relative_bias_table itself stays detached
    assert not relative_bias_table(w, L, buckets, maxd).requires_grad


def test_drmodel_hip_train_t5_flag():
    from transformers import T5EncoderModel
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    lm = T5EncoderModel(tr.t5_config(256, 1, 4, 512, "relu"))
    assert DRModel(lm, lm).hip_train_t5 is False
    assert DRModel(lm, lm, model_args=SimpleNamespace(encoder_only=True)).hip_train_t5 is False
    assert DRModel(lm, lm, model_args=SimpleNamespace(encoder_only=True, hip_train_t5=True)).hip_train_t5 is True


def test_cpu_t5_tower_with_the_flag_takes_hf_and_logs(caplog):
    """With the flag on, a tower on the CPU cannot take the HIP tower: reason logged, HF module."""
    import logging
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    lm = tr.t5_model(tr.t5_config(256, 1, 4, 512, "relu"))
    model = biencoder.DRModel(lm, lm, pooling="mean",
                              model_args=SimpleNamespace(encoder_only=True, hip_train_t5=True)).eval()
    ids, mask = tr.t5_batch(2, 8, seed=1)
    biencoder._FALLBACK_LOGGED.clear()
    with caplog.at_level(logging.WARNING, logger=biencoder.logger.name):
        hidden, reps = model.encode_passage({"input_ids": ids, "attention_mask": mask})
    assert reps.requires_grad and hidden.dtype == torch.float32
    assert any("tower on the CPU" in r.getMessage() for r in caplog.records)


def test_new_entries_reject_bad_shapes_without_gpu():
    """DRT_EINVAL before any HIP call (null pointers: a launch would have faulted, not returned)."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    E = _native.DRT_EINVAL
    fwd = lib.drt_attention_forward_bf16
    assert fwd(None, None, None, None, None, None, 2, 16, 4, 32, 1.0, 0.0, 0, 0, None) == E     # head_dim
    assert fwd(None, None, None, None, None, None, 2, 513, 4, 64, 1.0, 0.0, 0, 0, None) == E    # L > 512
    assert fwd(None, None, None, None, None, None, 2, 16, 4, 64, 1.0, 1.0, 0, 0, None) == E     # p = 1
    # non-null arguments are the address of a host buffer: nothing is dereferenced before the check
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    bwd = lib.drt_attention_backward_bf16
    wsq = lib.drt_attention_backward_workspace

    def bwd_rc(relbias=None, dbias=None, dtable=None, ws=None, ws_bytes=0):
        return bwd(None, None, None, None, None, relbias, None, None, 2, 50, 4, 64, 1.0, 0.0, 0, 0, dbias, dtable,
                   ws, ws_bytes, None)
    assert bwd_rc(relbias=p) == E                                                                # no table
    assert bwd_rc(dtable=p, ws=p, ws_bytes=wsq(2, 50, 4, 64, 1)) == E                            # table, no relbias
    assert bwd_rc(relbias=p, dbias=p, dtable=p, ws=p, ws_bytes=1 << 30) == E                     # both share ws
    assert bwd_rc(dbias=p, ws=p, ws_bytes=wsq(2, 50, 4, 64, 0) - 1) == E                         # one byte short
    assert wsq(2, 513, 4, 64, 1) == 0
    assert wsq(2, 50, 4, 64, 1) >= 2 * 4 * 99 * 4
    assert wsq(2, 200, 4, 64, 1) >= 2 * 2 * 4 * 399 * 4                                          # two query groups
    assert wsq(2, 50, 4, 64, 0) == 2 * 4 * 3 * 256 * 4   # [B][4 groups][3H] fp32; 8 rows need no column-sum scratch
    # the earlier names forward to the pair: the same refusals and the same sizes
    fwd = lib.drt_attention_relbias_train_fwd_bits_bf16
    assert fwd(None, None, None, None, None, None, 2, 16, 4, 32, 1.0, 0.0, 0, 0, None) == E     # head_dim
    assert fwd(None, None, None, None, None, None, 2, 513, 4, 64, 1.0, 0.0, 0, 0, None) == E    # L > 512
    assert fwd(None, None, None, None, None, None, 2, 16, 4, 64, 1.0, 1.0, 0, 0, None) == E     # p = 1
    bwd = lib.drt_attention_relbias_train_bwd_bf16
    assert bwd(None, None, None, None, None, None, None, None, 2, 16, 4, 64, 1.0, 0.0, 0, 0, None, None, 0,
               None) == E                                                                        # no table
    assert lib.drt_attention_relbias_train_bwd_workspace(2, 513, 4) == 0
    assert lib.drt_attention_relbias_train_bwd_workspace(2, 50, 4) == wsq(2, 50, 4, 64, 1)
    assert lib.drt_attention_relbias_train_bwd_workspace(2, 200, 4) == wsq(2, 200, 4, 64, 1)
    assert lib.drt_attention_train_bwd_bias_workspace(2, 4, 64) == wsq(2, 50, 4, 64, 0)
    assert lib.drt_rmsnorm_bwd_bf16(None, None, None, 1e-6, 4, 320, None, None, None, None, 0, None) == E
    assert lib.drt_rmsnorm_bwd_bf16(None, None, None, 1e-6, 4, 1280, None, None, None, None, 0, None) == E
    assert lib.drt_rmsnorm_bwd_workspace(4, 256) >= 1024 * 256 * 4
    assert lib.drt_gated_gelu_new_bwd_bf16(None, None, 4, 12, 0.0, 0, 0, None, None) == E
    assert lib.drt_relu_bwd_bf16(None, None, 12, 0.0, 0, 0, None, None) == E
    assert lib.drt_t5_embedding_bwd(None, None, 2, 0, 256, 100, None, None) == E

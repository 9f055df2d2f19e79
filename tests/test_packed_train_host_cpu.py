"""Host side of padding-free training, no GPU: the argument checks of the new native entries (they
refuse with DRT_EINVAL before any HIP call and return DRT_OK for empty inputs), the
``hip_packed_train`` flag of DRModel / RRModel and its own threshold, and the fallback of a tower
on the CPU, which keeps the HF module and says why."""
import logging
from types import SimpleNamespace

from oracle import bert_weights as bw

P = 0x1000   # a non-null "device pointer": the checks under test return before anything reads it


def _lib():
    from denseretrievaltoolkits_amd import _native
    return _native.load(), _native


def _fwd(lib, n=3, max_len=64, L_pad=64, T=100, W=2, hd=64, p=0.0, ptr=None, heads=12):
    return lib.drt_attention_varlen_train_forward_bf16(ptr, ptr, None, n, max_len, L_pad, T, W, ptr, ptr, ptr, heads, hd,
                                                       0.125, p, 1, 2, None)


def _bwd(lib, n=3, max_len=64, L_pad=64, T=100, W=2, hd=64, p=0.0, ptr=None, heads=12):
    return lib.drt_attention_varlen_backward_bf16(ptr, ptr, ptr, ptr, ptr, None, n, max_len, L_pad, T, W, ptr, ptr, ptr,
                                                  heads, hd, 0.125, p, 1, 2, None)


def test_new_entries_are_exported():
    _, native = _lib()
    for name in ("drt_attention_varlen_train_forward_bf16", "drt_attention_varlen_backward_bf16",
                 "drt_pack_rows_bf16", "drt_embed_ln_pre_packed"):
        assert name in native.EXPORTED


def test_attention_entries_refuse_bad_arguments_with_null_pointers():
    lib, native = _lib()
    E = native.DRT_EINVAL
    for call in (_fwd, _bwd):
        assert call(lib, max_len=161, L_pad=161) == E
        assert call(lib, max_len=0) == E
        assert call(lib, hd=32) == E
        assert call(lib, p=1.0) == E
        assert call(lib, p=-0.1) == E
        assert call(lib, heads=0) == E
        assert call(lib, n=-1) == E
        assert call(lib) == E                      # null tensors with work to do
        assert call(lib, ptr=P, L_pad=63) == E     # the padded length is below max_len
        assert call(lib, ptr=P, p=0.1, W=1) == E   # keep words that cannot hold max_len keys


def test_attention_entries_accept_empty_inputs():
    lib, native = _lib()
    for call in (_fwd, _bwd):
        assert call(lib, n=0) == native.DRT_OK
        assert call(lib, T=0) == native.DRT_OK
        assert call(lib, n=0, max_len=161) == native.DRT_EINVAL   # the shape checks come first


def test_max_packed_train_len_is_the_bound_both_entries_enforce():
    """MAX_PACKED_TRAIN_LEN (Python) against kAbMaxSeq (csrc/drt_common.h), through the library's own
    refusal: the shape checks come before the empty-input return, so n = 0 probes them with no launch."""
    from denseretrievaltoolkits_amd.model.train_tower import MAX_PACKED_TRAIN_LEN as M
    lib, native = _lib()
    assert M == 160
    for call in (_fwd, _bwd):
        assert call(lib, n=0, max_len=M, L_pad=M, W=5) == native.DRT_OK
        assert call(lib, n=0, max_len=M + 1, L_pad=M + 1, W=6) == native.DRT_EINVAL


def test_copies_refuse_and_accept():
    lib, native = _lib()
    E, OK = native.DRT_EINVAL, native.DRT_OK
    pack = lambda padded=P, cu=P, B=2, L=8, H=768, out=P, rows=32: lib.drt_pack_rows_bf16(   # noqa: E731
        padded, cu, B, L, H, out, rows, None)
    assert pack(H=100) == E and pack(L=0) == E and pack(rows=-1) == E and pack(padded=None) == E
    assert pack(cu=None) == E and pack(out=None) == E and pack(padded=P + 2) == E
    assert pack(B=0) == OK and pack(rows=0) == OK
    emb = lambda B=2, L=8, T=10, H=768, ids=P: lib.drt_embed_ln_pre_packed(   # noqa: E731
        ids, None, P, B, L, T, P, P, P, P, P, 1e-12, H, P, P, None)
    assert emb(H=100) == E and emb(T=17) == E and emb(ids=None) == E and emb(L=0) == E
    assert emb(B=0, T=0) == OK and emb(T=0) == OK


def test_flag_defaults_off_and_threshold():
    from denseretrievaltoolkits_amd.model import packing
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    from transformers import BertModel
    lm = BertModel(bw.bert_config(layers=1), add_pooling_layer=False)
    dr = DRModel(lm, lm)
    rr = RRModel(lm, LinearHead(768, 1))
    assert dr.hip_packed_train is False and rr.hip_packed_train is False
    assert dr.hip_packed is False and rr.hip_packed is False
    args = SimpleNamespace(hip_packed_train=True)
    dr, rr = DRModel(lm, lm, model_args=args), RRModel(lm, LinearHead(768, 1), model_args=args)
    assert dr.hip_packed_train is True and rr.hip_packed_train is True
    assert dr.hip_packed is False and rr.hip_packed is False     # the inference flag is its own
    assert 0.0 < packing.hip_packed_train_min_saving <= 0.25


def test_cpu_tower_keeps_hf_and_logs_why(caplog):
    """A tower on the CPU has no HIP training pass, packed or padded: the HF module runs under
    autograd, the result is HF's, and the flag's fallback is logged."""
    import torch
    from denseretrievaltoolkits_amd.model import biencoder
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from transformers import BertModel
    lm = bw.init_model_(BertModel(bw.bert_config(layers=1), add_pooling_layer=False).eval(), 0)
    ids, mask = bw.token_batch(3, 16, seed=5)
    items = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}
    dr = DRModel(lm, lm)
    dr.hip_packed_train = True
    biencoder._FALLBACK_LOGGED.clear()
    with caplog.at_level(logging.WARNING):
        hidden, reps = dr.encode(items, lm, None)
    ref = lm(**items).last_hidden_state
    assert torch.equal(hidden, ref) and reps.requires_grad
    text = " ".join(r.getMessage() for r in caplog.records)
    assert "hip_packed_train" in text and "tower on the CPU" in text

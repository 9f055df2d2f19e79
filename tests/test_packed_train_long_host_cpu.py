"""Host side of padding-free training above 160 tokens, no GPU: the argument checks of the two long
entries (DRT_EINVAL before any HIP call, DRT_OK for empty inputs), the ``hip_packed_train_long`` flag,
and the short / long split and tile table of a PackingPlan."""
from types import SimpleNamespace

import pytest

from oracle import bert_weights as bw

P = 0x1000   # a non-null "device pointer": the checks under test return before anything reads it


def _lib():
    from denseretrievaltoolkits_amd import _native
    return _native.load(), _native


def _fwd(lib, n=3, max_len=300, L_pad=320, T=700, W=10, hd=64, p=0.0, ptr=None, heads=12, table=P):
    return lib.drt_attention_varlen_long_train_forward_bf16(ptr, ptr, None, n, max_len, L_pad, T, W, ptr, ptr, ptr,
                                                            heads, hd, 0.125, p, 1, 2, None)


def _bwd(lib, n=3, max_len=300, L_pad=320, T=700, W=10, hd=64, p=0.0, ptr=None, heads=12, table=P):
    return lib.drt_attention_varlen_long_backward_bf16(ptr, ptr, ptr, ptr, ptr, table, n, max_len, L_pad, T, W, ptr,
                                                       ptr, ptr, heads, hd, 0.125, p, 1, 2, None)


def test_long_entries_are_exported():
    _, native = _lib()
    assert "drt_attention_varlen_long_train_forward_bf16" in native.EXPORTED
    assert "drt_attention_varlen_long_backward_bf16" in native.EXPORTED


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_long_entries_refuse_and_accept(call):
    from denseretrievaltoolkits_amd.model.train_tower import MAX_PACKED_TRAIN_LEN, MAX_PACKED_TRAIN_LONG_LEN as M
    lib, native = _lib()
    E, OK = native.DRT_EINVAL, native.DRT_OK
    assert M == 512 and MAX_PACKED_TRAIN_LEN == 160
    for bad in (dict(max_len=0), dict(hd=32), dict(p=1.0), dict(p=-0.1), dict(heads=0), dict(n=-1),
                dict(),                                   # null tensors with work to do
                dict(ptr=P, L_pad=299),                   # the padded length is below max_len
                dict(ptr=P, p=0.1, W=9)):                 # keep words that cannot hold max_len keys
        assert call(lib, **bad) == E, bad
    assert _bwd(lib, ptr=P, table=None) == E              # a null tile table
    assert call(lib, n=0) == OK and call(lib, T=0) == OK
    # the bound, probed with no launch: the shape checks come before the empty-input return
    assert call(lib, n=0, max_len=M, L_pad=M, W=16) == OK
    assert call(lib, n=0, max_len=M + 1, L_pad=M + 1, W=17) == E


def test_both_flags_default_off():
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    from transformers import BertModel
    lm = BertModel(bw.bert_config(layers=1), add_pooling_layer=False)
    dr, rr = DRModel(lm, lm), RRModel(lm, LinearHead(768, 1))
    assert dr.hip_packed_train is False and dr.hip_packed_train_long is False
    assert rr.hip_packed_train is False and rr.hip_packed_train_long is False
    args = SimpleNamespace(hip_packed_train_long=True)
    dr, rr = DRModel(lm, lm, model_args=args), RRModel(lm, LinearHead(768, 1), model_args=args)
    assert dr.hip_packed_train_long is True and rr.hip_packed_train_long is True
    assert dr.hip_packed_train is False and rr.hip_packed_train is False   # the short flag is its own


def test_split_and_tile_table():
    from denseretrievaltoolkits_amd.model.packing import _plan_from_lens
    lens = [300, 40, 256, 161, 160, 257, 512, 128]       # 256 = 2 * 128, 257 = 2 * 128 + 1
    plan = _plan_from_lens(list(lens), 512, "cpu", 0.0, True)
    sp = plan.split()
    short = [b for b, n in enumerate(lens) if n <= 160]
    long_ = [b for b, n in enumerate(lens) if n > 160]
    tiles = [[b, g] for b in long_ for g in range(-(-lens[b] // 128))]
    assert sp["tiles"].tolist() == tiles and sp["n_tiles"] == len(tiles) == 3 + 2 + 2 + 3 + 4
    for part, ids in (("short", short), ("long", long_)):
        (one, n, ml), = sp[part][False]
        assert sorted(one.tolist()) == ids and n == len(ids) and ml == max(lens[b] for b in ids)
        per_class = sp[part][True]
        assert sorted(b for s, _, _ in per_class for b in s.tolist()) == ids
        assert all(n == len(s) and ml == max(lens[b] for b in s.tolist()) for s, n, ml in per_class)
        assert plan.launches(False, part) == [(one.data_ptr(), n, ml)]
    assert [ml for _, _, ml in sp["long"][True]] == [512, 257, 161]   # by LDS image, longest first
    assert plan.launches(False) == [(None, 8, 512)]                    # the whole-batch form is unchanged
    all_long = _plan_from_lens([200, 400], 512, "cpu", 0.0, True).split()
    assert all_long["long"][False] == [(None, 2, 400)] and all_long["short"] == {False: [], True: []}

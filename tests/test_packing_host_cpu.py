"""Host side of the padding-free inference path, no GPU: plan_packing on CPU masks, and the
argument checks of the four packed entry points, which refuse with DRT_EINVAL before any HIP call
and return DRT_OK for empty inputs."""
import pytest

P = 0x1000   # a non-null "device pointer": the checks under test return before anything reads it


def _prefix_mask(lens, L):
    import torch
    return (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)


def test_plan_of_prefix_masks():
    import torch
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    lens, L = [5, 1, 32, 17, 32], 32
    plan = plan_packing(_prefix_mask(lens, L), L)
    assert plan is not None
    assert plan.lens == lens and plan.T == sum(lens) and plan.max_len == 32 and (plan.B, plan.L) == (5, L)
    assert plan.cu_seqlens.dtype == torch.int32 and plan.cu_seqlens.device.type == "cpu"
    assert plan.cu_seqlens.tolist() == [0, 5, 6, 38, 55, 87]
    # bool and 0/1 float masks are the same prefixes
    assert plan_packing(_prefix_mask(lens, L).bool(), L).lens == lens


def test_plan_length_classes_and_halves():
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    lens, L = [5, 200, 33, 64, 161, 32, 1], 256
    plan = plan_packing(_prefix_mask(lens, L), L)
    got = sorted((sorted(ids.tolist()), n, ml) for ids, n, ml in plan.classes())
    # ceil(len / 32): 1 -> {0, 5, 6}, 2 -> {2, 3}, more than 5 blocks -> {1, 4}
    assert got == sorted([([0, 5, 6], 3, 32), ([2, 3], 2, 64), ([1, 4], 2, 200)])
    one = plan_packing(_prefix_mask([3, 30, 17], 32), 32)
    assert one.classes() == [(None, 3, 30)]
    (b0, first), (b1, second) = plan.halves()
    assert b0 == 0 and first.lens + second.lens == lens and b1 == len(first.lens)
    assert first.T + second.T == plan.T and 0 < first.T < plan.T
    # the boundary nearest T / 2 = 248: after [5, 200, 33] (238) rather than after [5, 200] (205)
    assert first.lens == [5, 200, 33]


def test_plan_launches():
    """PackingPlan.launches: what every varlen attention caller iterates over, (seq_ids pointer or None,
    n_seqs, max_len) per launch."""
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    lens, L = [5, 200, 33, 64, 161, 32, 1], 256
    plan = plan_packing(_prefix_mask(lens, L), L)
    assert plan.launches(per_class=False) == [(None, 7, 200)]
    got = plan.launches(per_class=True)
    classes = plan.classes()
    assert got == [(ids.data_ptr(), n, ml) for ids, n, ml in classes]
    # the three classes of test_plan_length_classes_and_halves, each pointer its class tensor's
    by_ptr = {ids.data_ptr(): sorted(ids.tolist()) for ids, _, _ in classes}
    assert sorted((by_ptr[p], n, ml) for p, n, ml in got) == sorted(
        [([0, 5, 6], 3, 32), ([2, 3], 2, 64), ([1, 4], 2, 200)])
    one = plan_packing(_prefix_mask([3, 30, 17], 32), 32)   # one class: no list either way
    assert one.launches(per_class=True) == one.launches(per_class=False) == [(None, 3, 30)]


@pytest.mark.parametrize("kind", ["holes", "left", "allzero_row", "none", "full"])
def test_no_plan(kind):
    import torch
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    L = 16
    mask = _prefix_mask([4, 16, 9], L)
    if kind == "holes":
        mask[2, 3] = 0
    elif kind == "left":
        mask[0] = torch.flip(mask[0], dims=(0,))
    elif kind == "allzero_row":
        mask[0] = 0
    elif kind == "none":
        mask = None
    else:
        mask = torch.ones(3, L, dtype=torch.int64)
    assert plan_packing(mask, L) is None
    if kind == "full":   # the control of the A/B tool
        assert plan_packing(mask, L, force=True).T == 3 * L


def test_min_saving_threshold():
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    mask = _prefix_mask([15, 16, 16, 16], 16)            # padding share 1 / 64
    assert plan_packing(mask, 16, min_saving=0.0) is not None
    assert plan_packing(mask, 16, min_saving=0.05) is None
    # the default is the measured threshold of model/packing.py
    from denseretrievaltoolkits_amd.model import packing
    assert 1 / 64 < packing.hip_packed_min_saving <= 0.25
    assert plan_packing(mask, 16) is None
    assert plan_packing(_prefix_mask([4, 16, 16, 16], 16), 16) is not None      # padding share 3 / 16


def _lib():
    from denseretrievaltoolkits_amd import _native
    return _native.load(), _native


def _varlen(lib, qkv=P, cu=P, seq=None, n=3, max_len=64, ctx=P, heads=12, hd=64):
    return lib.drt_attention_varlen_forward_bf16(qkv, cu, seq, n, max_len, ctx, heads, hd, 0.125, None)


def _embed(lib, ids=P, cu=P, B=2, L=8, T=9, H=768, out=P, word=P):
    return lib.drt_embed_ln_packed(ids, None, cu, B, L, T, word, P, P, P, P, 1e-12, H, out, None)


def _pool(lib, hidden=P, cu=P, B=2, L=8, H=768, mode=0, out=P):
    return lib.drt_pool_packed_bf16(hidden, cu, B, L, H, mode, out, None, None)


def _unpack(lib, packed=P, cu=P, B=2, L=8, H=768, out=P):
    return lib.drt_unpack_rows_bf16(packed, cu, B, L, H, out, None)


def test_entries_refuse_bad_arguments():
    lib, native = _lib()
    E = native.DRT_EINVAL
    assert _varlen(lib, max_len=0) == E
    assert _varlen(lib, max_len=513) == E
    assert _varlen(lib, hd=32) == E
    assert _varlen(lib, hd=128) == E
    assert _varlen(lib, heads=0) == E
    assert _varlen(lib, n=-1) == E
    assert _varlen(lib, qkv=None) == E
    assert _varlen(lib, cu=None) == E
    assert _varlen(lib, ctx=None) == E
    assert _embed(lib, H=700) == E
    assert _embed(lib, H=1280) == E
    assert _embed(lib, L=0) == E
    assert _embed(lib, T=17) == E          # more tokens than B * L
    assert _embed(lib, ids=None) == E
    assert _embed(lib, cu=None) == E
    assert _embed(lib, out=None) == E
    assert _embed(lib, word=None) == E
    assert _pool(lib, mode=3) == E
    assert _pool(lib, mode=-1) == E
    assert _pool(lib, hidden=None) == E
    assert _pool(lib, cu=None) == E
    assert _pool(lib, out=None) == E
    assert _unpack(lib, H=100) == E        # rows are copied in 16-byte pieces
    assert _unpack(lib, L=0) == E
    assert _unpack(lib, packed=None) == E
    assert _unpack(lib, cu=None) == E
    assert _unpack(lib, out=None) == E


def test_entries_accept_empty_inputs():
    lib, native = _lib()
    assert _varlen(lib, n=0, qkv=None, cu=None, ctx=None) == native.DRT_OK
    assert _embed(lib, B=0, T=0, ids=None, cu=None, out=None) == native.DRT_OK
    assert _embed(lib, T=0, ids=None, cu=None, out=None) == native.DRT_OK
    assert _pool(lib, B=0, hidden=None, cu=None, out=None) == native.DRT_OK
    assert _unpack(lib, B=0, packed=None, cu=None, out=None) == native.DRT_OK
    # the shape checks come first
    assert _varlen(lib, n=0, max_len=0) == native.DRT_EINVAL
    assert _pool(lib, B=0, mode=3) == native.DRT_EINVAL

"""CPU: the grouped (MaxP) search's depth plan and the two facts its exactness stands on (DESIGN.md "Grouped
search"), by brute force on small random instances; the host-only side of drt_topk_collapse.  No GPU compute."""
import numpy as np
import pytest


@pytest.mark.parametrize("k,p_max,ntotal,want", [
    (10, 1, 10 ** 7, (10, None)), (100, 20, 10 ** 7, (2000, None)), (100, 21, 10 ** 7, (2048, 2100)),
    (1000, 40, 10 ** 7, (2048, 32768)), (10, 2500, 6000, (2048, 6000)), (5, 3, 7, (7, None))])
def test_grouped_depths(k, p_max, ntotal, want):
    from denseretrievaltoolkits_amd import kernels
    assert kernels.grouped_depths(k, p_max, ntotal) == want


def test_grouped_depths_guards():
    from denseretrievaltoolkits_amd import kernels
    assert kernels.grouped_depths(3, 2, 0) == (1, None)          # an empty index is searched at depth 1
    assert kernels.grouped_depths(kernels.MAX_K, 1, 10 ** 7) == (kernels.MAX_K, None)
    assert kernels.grouped_depths(kernels.MAX_K + 1, 1, 10 ** 7) == (kernels.MAX_K, kernels.MAX_K + 1)
    for bad in ((0, 1, 10), (1, 0, 10), (1, 1, -1)):
        with pytest.raises(ValueError):
            kernels.grouped_depths(*bad)


def first_occurrences(groups_in_order):
    """The distinct values of a sequence in the order they first appear."""
    _, first = np.unique(groups_in_order, return_index=True)
    return groups_in_order[np.sort(first)]


def test_prefix_property_and_depth_bound_by_brute_force():
    """200 random instances (n <= 400 rows, group sizes 1..30, integer scores with many ties): the
    first-occurrence groups of EVERY prefix of the canonical row order are a prefix of the full grouped order,
    and the prefix of length min(k * P_max, n) shows min(k, #groups) groups."""
    rng = np.random.default_rng(20240)
    for _ in range(200):
        n = int(rng.integers(1, 401))
        sizes = []
        while sum(sizes) < n:
            sizes.append(min(int(rng.integers(1, 31)), n - sum(sizes)))
        group_of = rng.permutation(np.repeat(rng.permutation(10 * len(sizes))[: len(sizes)], sizes))
        p_max = max(sizes)
        scores = rng.integers(-3, 4, size=n)
        order = np.lexsort((np.arange(n), -scores))               # canonical: score desc, row id asc
        # the grouped order restated from the definition: per group its best row, groups by that row's rank
        rank = np.empty(n, np.int64)
        rank[order] = np.arange(n)
        gids = np.unique(group_of)
        best_rank = np.array([rank[group_of == g].min() for g in gids])
        full_order = gids[np.argsort(best_rank)]
        for depth in range(1, n + 1):
            seen = first_occurrences(group_of[order[:depth]])
            np.testing.assert_array_equal(seen, full_order[: seen.size])
        for k in (1, 2, int(rng.integers(1, 12)), len(sizes), len(sizes) + 3):
            depth = min(k * p_max, n)
            assert first_occurrences(group_of[order[:depth]]).size >= min(k, len(sizes))


def test_collapse_symbols_and_workspace_are_host_side():
    from denseretrievaltoolkits_amd import _native, kernels
    lib = _native.load()
    assert {"drt_topk_collapse", "drt_topk_collapse_workspace"} <= set(_native.EXPORTED)
    T = kernels.COLLAPSE_LDS_K
    # > 0 for supported shapes, 0 for rejected ones
    assert lib.drt_topk_collapse_workspace(0, 1) > 0 and lib.drt_topk_collapse_workspace(1, T) > 0
    for nq, k_in in ((1, 0), (1, kernels.MAX_K_LARGE + 1), (-1, 10)):
        assert lib.drt_topk_collapse_workspace(nq, k_in) == 0
    # beyond the LDS threshold: one table of the power of two >= 2 k_in 8-byte slots per region ...
    assert lib.drt_topk_collapse_workspace(1, T + 1) == 8 * 2 * 2 * T
    assert lib.drt_topk_collapse_workspace(3, kernels.MAX_K_LARGE) == 3 * 8 * 2 * kernels.MAX_K_LARGE
    # ... and bounded whatever nq is
    cap = lib.drt_topk_collapse_workspace(kernels.COLLAPSE_REGIONS, kernels.MAX_K_LARGE)
    assert cap == kernels.COLLAPSE_REGIONS * 8 * 2 * kernels.MAX_K_LARGE
    assert lib.drt_topk_collapse_workspace(10 ** 6, kernels.MAX_K_LARGE) == cap
    assert lib.drt_topk_collapse_workspace(10 ** 6, T) == lib.drt_topk_collapse_workspace(1, T)


@pytest.mark.parametrize("k_in,k_out", [(0, 1), (32769, 1), (8, 0)])
def test_collapse_rejects_bad_shapes_without_gpu(k_in, k_out):
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    rc = lib.drt_topk_collapse(None, None, 4, k_in, None, 0, k_out, None, None, None, None, None, 0, None)
    assert rc == _native.DRT_EINVAL


def test_op_schema_and_fake_kernel():
    import torch
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    assert str(drt.topk_collapse.default._schema) == (
        "drt::topk_collapse(Tensor scores, Tensor ids, Tensor groups, int k_out) -> (Tensor, Tensor, Tensor, Tensor)")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        s = torch.empty((7, 90), dtype=torch.float32, device="cuda")
        i = torch.empty((7, 90), dtype=torch.int64, device="cuda")
        g = torch.empty((500,), dtype=torch.int32, device="cuda")
        os_, og, oi, cnt = drt.topk_collapse(s, i, g, 20)
    assert (tuple(os_.shape), os_.dtype) == ((7, 20), torch.float32)
    assert (tuple(og.shape), og.dtype) == ((7, 20), torch.int32)
    assert (tuple(oi.shape), oi.dtype) == ((7, 20), torch.int64)
    assert (tuple(cnt.shape), cnt.dtype) == ((7,), torch.int32)


def test_index_classes_offer_the_grouped_surface():
    import inspect
    from denseretrievaltoolkits_amd import search
    from denseretrievaltoolkits_amd.evaluator.index import BaseFaissIPRetriever
    for cls in (search.FlatIPIndex, search.ShardedFlatIP):
        for name in ("set_groups", "search_grouped_batches_iter", "search_grouped_device", "search_grouped"):
            assert callable(getattr(cls, name)), (cls, name)
    for fn in (BaseFaissIPRetriever.search_grouped, BaseFaissIPRetriever.batch_search_grouped):
        assert inspect.signature(fn).parameters["groups"].default is None

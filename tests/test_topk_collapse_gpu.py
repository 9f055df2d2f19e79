"""GPU: drt_topk_collapse (csrc/collapse.hip) against a numpy restatement on synthetic canonical lists.

The kernel is a stable compaction of a canonical top-k list to the first entry of every group -- the device form
of the host-side dedup a document-level (MaxP) search otherwise needs.  It is called through the C ABI into output
buffers pre-filled with garbage (an unwritten slot shows) and through torch.ops.drt.topk_collapse; scores, group
ids, row ids and counts must equal the restatement exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD_S = np.float32(-3.402823466e+38)
LDS_K = 2048                                    # kernels.COLLAPSE_LDS_K, checked below
SHAPES = [(1, 1, 1), (3, 63, 10), (5, 64, 64), (5, 65, 20), (130, 257, 100), (2, 2049, 2048), (2, 5000, 300),
          (2, LDS_K, 64), (2, LDS_K + 1, 64), (1, 32768, 32768)]
MAPS = ["identity", "one_group", "consecutive", "shuffled", "strided_ids", "high_ids"]


def restate(scores, ids, groups, k_out):
    nq = scores.shape[0]
    os_ = np.full((nq, k_out), PAD_S, np.float32)
    og = np.full((nq, k_out), -1, np.int32)
    oi = np.full((nq, k_out), -1, np.int64)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        j = np.nonzero((ids[q] >= 0) & (ids[q] < groups.size))[0]
        _, first = np.unique(groups[ids[q, j]], return_index=True)
        j = j[np.sort(first)]
        cnt[q] = j.size
        j = j[:k_out]
        os_[q, : j.size] = scores[q, j]
        og[q, : j.size] = groups[ids[q, j]]
        oi[q, : j.size] = ids[q, j]
    return os_, og, oi, cnt


def make_lists(rng, nq, k_in, n_rows, n_pad=0):
    """[nq, k_in] lists over row ids [0, n_rows) in (score desc, id asc) order with many exact score ties; the
    last n_pad entries pads."""
    ids = np.stack([rng.choice(n_rows, size=k_in, replace=False) for _ in range(nq)]).astype(np.int64)
    scores = rng.integers(-40, 41, size=(nq, k_in)).astype(np.float32) / 4
    for q in range(nq):
        o = np.lexsort((ids[q], -scores[q]))
        ids[q], scores[q] = ids[q][o], scores[q][o]
    if n_pad:
        ids[:, k_in - n_pad:] = -1
        scores[:, k_in - n_pad:] = PAD_S
    return scores, ids


def make_groups(rng, kind, n_rows):
    """int32 [n_rows] row -> group maps."""
    if kind == "identity":
        return np.arange(n_rows, dtype=np.int32)
    if kind == "one_group":
        return np.full(n_rows, 7, np.int32)
    sizes = rng.integers(1, 41, size=n_rows)
    sizes = sizes[: np.searchsorted(np.cumsum(sizes), n_rows) + 1]
    dense = np.repeat(np.arange(sizes.size), sizes)[:n_rows].astype(np.int64)   # sizes 1..40, consecutive rows
    if kind == "consecutive":
        return dense.astype(np.int32)
    if kind == "shuffled":                                                      # the same sizes, rows scattered
        return rng.permutation(dense).astype(np.int32)
    if kind == "strided_ids":                                                   # multiples of 65536: probing
        assert dense.max() * 65536 < 2 ** 31
        return (rng.permutation(dense) * 65536).astype(np.int32)
    if kind == "high_ids":                                                      # ids up to 2^31 - 1
        return (2 ** 31 - 1 - rng.permutation(dense)).astype(np.int32)
    raise AssertionError(kind)


def run_both(dev, scores, ids, groups, k_out):
    """The C entry into garbage-filled buffers and the torch op; both must agree.  Host arrays back."""
    import torch
    from denseretrievaltoolkits_amd import _native, ops
    lib = _native.load()
    nq, k_in = scores.shape
    s_d, i_d, g_d = (torch.from_numpy(x).to(dev) for x in (scores, ids, groups))
    os_ = torch.full((nq, k_out), 12345.0, dtype=torch.float32, device=dev)
    og = torch.full((nq, k_out), 555, dtype=torch.int32, device=dev)
    oi = torch.full((nq, k_out), 777, dtype=torch.int64, device=dev)
    cnt = torch.full((nq,), -9, dtype=torch.int32, device=dev)
    wsb = int(lib.drt_topk_collapse_workspace(nq, k_in))
    assert wsb > 0
    ws = torch.full((wsb,), 0x5A, dtype=torch.uint8, device=dev)     # a dirty workspace: the kernel resets it
    rc = lib.drt_topk_collapse(s_d.data_ptr(), i_d.data_ptr(), nq, k_in, g_d.data_ptr() if groups.size else None,
                               groups.size, k_out, os_.data_ptr(), og.data_ptr(), oi.data_ptr(), cnt.data_ptr(),
                               ws.data_ptr(), wsb, _native.stream_ptr(dev))
    assert rc == 0
    ts, tg, ti, tc = ops.load().topk_collapse(s_d, i_d, g_d, k_out)
    torch.cuda.synchronize()
    assert torch.equal(ts, os_) and torch.equal(tg, og) and torch.equal(ti, oi) and torch.equal(tc, cnt)
    return os_.cpu().numpy(), og.cpu().numpy(), oi.cpu().numpy(), cnt.cpu().numpy()


def check(dev, scores, ids, groups, k_out):
    got = run_both(dev, scores, ids, groups, k_out)
    want = restate(scores, ids, groups, k_out)
    for g, w, name in zip(got, want, ("scores", "groups", "ids", "count")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return want


def test_threshold_constant_matches_the_library():
    """kernels.COLLAPSE_LDS_K is where the workspace query switches from the LDS form's token size to tables."""
    from denseretrievaltoolkits_amd import _native, kernels
    lib = _native.load()
    assert kernels.COLLAPSE_LDS_K == LDS_K
    assert lib.drt_topk_collapse_workspace(1, LDS_K) < 8 * 2 * LDS_K < lib.drt_topk_collapse_workspace(1, LDS_K + 1)


@pytest.mark.parametrize("nq,k_in,k_out", SHAPES)
def test_shapes_and_group_maps(dev, nq, k_in, k_out):
    """Every shape with every group map; the lists are shared by the maps."""
    rng = np.random.default_rng(1000 * nq + k_in)
    n_rows = k_in + k_in // 3 + 50
    scores, ids = make_lists(rng, nq, k_in, n_rows)
    for kind in MAPS:
        groups = make_groups(rng, kind, n_rows)
        os_, og, oi, cnt = check(dev, scores, ids, groups, k_out)
        if kind == "identity":
            np.testing.assert_array_equal(oi, ids[:, :k_out])
            np.testing.assert_array_equal(os_, scores[:, :k_out])
            assert (cnt == k_in).all()
        if kind == "one_group":
            assert (cnt == 1).all() and (oi[:, 0] == ids[:, 0]).all() and (og[:, 0] == 7).all()
            assert (oi[:, 1:] == -1).all()


@pytest.mark.parametrize("nq,k_in", [(1030, 70), (130, LDS_K + 1)])
def test_table_regions_are_reused_across_queries(dev, nq, k_in):
    """More queries than work-groups in flight (1024 in the LDS form, 128 table regions in the workspace form):
    a work-group's later queries find its table as the earlier one left it and must reset it -- a group seen by
    the region's previous query would otherwise look like a repeat."""
    from denseretrievaltoolkits_amd import kernels
    assert nq > (kernels.COLLAPSE_LDS_GROUPS if k_in <= LDS_K else kernels.COLLAPSE_REGIONS)
    rng = np.random.default_rng(k_in)
    n_rows = 2 * k_in
    scores, ids = make_lists(rng, nq, k_in, n_rows)
    for kind in ("shuffled", "high_ids"):
        _, _, _, cnt = check(dev, scores, ids, make_groups(rng, kind, n_rows), 64)
        assert (cnt > 1).all()


def test_pads_and_out_of_range_ids_are_dropped(dev):
    rng = np.random.default_rng(4)
    n_rows = 400
    scores, ids = make_lists(rng, 4, 300, n_rows, n_pad=37)
    groups = make_groups(rng, "shuffled", n_rows)
    _, og, oi, cnt = check(dev, scores, ids, groups, 300)
    assert (cnt <= 300 - 37).all() and (oi[:, -37:] == -1).all() and (og[:, -37:] == -1).all()
    # ids at and beyond n_rows (and far beyond 32 bits), and negative ones other than -1
    ids2 = ids.copy()
    ids2[:, 5] = n_rows
    ids2[:, 11] = n_rows + (1 << 33)
    ids2[:, 17] = -5
    ids2[0, 0] = 1 << 40
    _, _, oi, _ = check(dev, scores, ids2, groups, 300)
    assert not np.isin(oi, [n_rows, n_rows + (1 << 33), -5, 1 << 40]).any()
    # a map shorter than the ids the list holds: the rows beyond it are dropped; an empty map drops all
    check(dev, scores, ids, groups[:150], 50)
    _, _, oi, cnt = check(dev, scores, ids, groups[:0], 50)
    assert (cnt == 0).all() and (oi == -1).all()


def test_k_out_beyond_the_count_pads_the_tail(dev):
    rng = np.random.default_rng(7)
    n_rows = 3000
    scores, ids = make_lists(rng, 3, 2500, n_rows)
    groups = make_groups(rng, "consecutive", n_rows)
    os_, og, oi, cnt = check(dev, scores, ids, groups, 4000)       # k_out > k_in > count
    for q in range(3):
        assert 0 < cnt[q] < 2500
        assert (oi[q, : cnt[q]] >= 0).all() and (oi[q, cnt[q]:] == -1).all()
        assert (og[q, cnt[q]:] == -1).all() and (os_[q, cnt[q]:] == PAD_S).all()


def test_op_argument_checks(dev):
    import torch
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    s = torch.zeros(2, 8, device=dev)
    i = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    g = torch.zeros(20, dtype=torch.int32, device=dev)
    drt.topk_collapse(s, i, g, 4)
    with pytest.raises(ValueError):
        drt.topk_collapse(s, i.int(), g, 4)
    with pytest.raises(ValueError):
        drt.topk_collapse(s.double(), i, g, 4)
    with pytest.raises(ValueError):
        drt.topk_collapse(s, i, g.long(), 4)
    with pytest.raises(ValueError):
        drt.topk_collapse(s, i, g.view(4, 5), 4)
    with pytest.raises(ValueError):
        drt.topk_collapse(s, i[:, :7], g, 4)
    with pytest.raises(ValueError):
        drt.topk_collapse(s, i, g, 0)
    with pytest.raises(ValueError):
        drt.topk_collapse(torch.zeros(1, 32769, device=dev), torch.zeros(1, 32769, dtype=torch.int64, device=dev), g, 4)


def test_opcheck(dev):
    import torch
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic")
    rng = np.random.default_rng(8)
    scores, ids = make_lists(rng, 4, 90, 200)
    groups = make_groups(rng, "shuffled", 200)
    args = [torch.from_numpy(x).to(dev) for x in (scores, ids, groups)]
    torch.library.opcheck(drt.topk_collapse.default, (*args, 30), test_utils=utils)
    scores, ids = make_lists(rng, 2, LDS_K + 40, 3000)
    args = [torch.from_numpy(x).to(dev) for x in (scores, ids, make_groups(rng, "consecutive", 3000))]
    torch.library.opcheck(drt.topk_collapse.default, (*args, 100), test_utils=utils)

"""GPU: the grouped (document-level, MaxP) search end to end against a numpy fp64 brute force.

Integer bf16 fixtures (helpers.int_bf16), so every score is exact.  Expected: the full score matrix, per group its
max score and the smallest row id attaining it, groups sorted by (-score, row id).  Scores, group ids and row ids
must be equal element for element."""
import numpy as np
import pytest

from helpers import int_bf16, to_dev_bf16

pytestmark = pytest.mark.gpu

PAD_S = np.float32(-3.402823466e+38)


def brute_force(q, p, groups, k):
    """(scores fp32, group ids, best-row ids) [nq, k] of the grouped search, padded (-FLT_MAX, -1, -1)."""
    S = q.astype(np.float64) @ p.astype(np.float64).T
    gids, inv = np.unique(groups, return_inverse=True)
    nq = q.shape[0]
    es = np.full((nq, k), PAD_S, np.float32)
    eg = np.full((nq, k), -1, np.int64)
    er = np.full((nq, k), -1, np.int64)
    rows = np.arange(p.shape[0])
    for j in range(nq):
        o = np.lexsort((rows, -S[j]))                       # canonical row order
        _, first = np.unique(inv[o], return_index=True)     # per group the first position = max score, least row
        best = o[first]                                     # group g's best row
        go = np.lexsort((best, -S[j, best]))[:k]
        es[j, : go.size] = S[j, best[go]]
        eg[j, : go.size] = gids[go]
        er[j, : go.size] = best[go]
    return es, eg, er


def sized_groups(rng, n, lo, hi):
    """[n] group ids (arbitrary distinct numbers below 2^31) of random sizes lo..hi, rows shuffled."""
    sizes = rng.integers(lo, hi + 1, size=n)
    sizes = sizes[: np.searchsorted(np.cumsum(sizes), n) + 1]
    names = rng.choice(2 ** 31 - 1, size=sizes.size, replace=False)
    return rng.permutation(np.repeat(names, sizes)[:n]).astype(np.int64)


def assert_equal(got, want):
    for g, w, name in zip(got, want, ("scores", "groups", "rows")):
        np.testing.assert_array_equal(np.asarray(g), w, err_msg=name)


@pytest.fixture(scope="module")
def one_rung(dev):
    """n = 3000, d = 64, group sizes 1..8, 133 queries; the brute force at k = 100 (k = 10 is its head)."""
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    rng = np.random.default_rng(31)
    p = int_bf16(rng, (3000, 64), -3, 3)
    q = int_bf16(rng, (133, 64), -3, 3)
    groups = sized_groups(rng, 3000, 1, 8)
    idx = FlatIPIndex(64, device=dev)
    idx.add(to_dev_bf16(p, dev))
    idx.set_groups(groups)
    return dict(p=p, q=q, groups=groups, idx=idx, want=brute_force(q, p, groups, 100),
                ngroups=np.unique(groups).size)


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("batch", [5, 128])
def test_one_rung_batches(dev, one_rung, k, batch):
    f = one_rung
    from denseretrievaltoolkits_amd import kernels
    assert kernels.grouped_depths(k, f["idx"]._p_max, 3000)[1] is None and f["idx"]._p_max == 8
    qd = to_dev_bf16(f["q"], dev)
    res = list(f["idx"].search_grouped_batches_iter([qd[a: a + batch] for a in range(0, 133, batch)], k))
    assert [r[0].shape[0] for r in res] == [min(batch, 133 - a) for a in range(0, 133, batch)]
    import torch
    got = [torch.cat([r[j] for r in res]).cpu().numpy() for j in range(4)]
    assert_equal(got[:3], [w[:, :k] for w in f["want"]])
    assert (got[3] >= k).all()
    # numpy out of the iterator and out of search_grouped
    host = list(f["idx"].search_grouped_batches_iter([qd[:7]], k, to_host=True))[0]
    assert all(isinstance(x, np.ndarray) for x in host)
    assert_equal(host[:3], [w[:7, :k] for w in f["want"]])
    assert_equal(f["idx"].search_grouped(f["q"][:7], k)[:3], [w[:7, :k] for w in f["want"]])


def test_k_beyond_the_number_of_groups_pads(dev, one_rung):
    f = one_rung
    k = f["ngroups"] + 25
    s, g, r, cnt = f["idx"].search_grouped(f["q"][:6], k)
    assert_equal((s, g, r), brute_force(f["q"][:6], f["p"], f["groups"], k))
    assert (cnt == f["ngroups"]).all() and (g[:, f["ngroups"]:] == -1).all() and (r[:, f["ngroups"]:] == -1).all()


def dominated(rng, n, nbig, nq=6):
    """A corpus with one group of ``nbig`` rows that outscore every other row for query 0 only: those rows are
    2 u or 3 u for a fixed +-1 pattern u and query 0 is 3 u (scores 384 and 576), while every other row is
    random on 16 coordinates and zero elsewhere (at most 3 * 3 * 16 = 144 against query 0).  The other queries
    are random on those 16 coordinates and -2 u on the rest, which puts the big group's rows at the bottom
    (at most 2 * (48 - 96) < 0) and leaves the others' scores random."""
    d = 64
    u = rng.choice([-1.0, 1.0], size=d).astype(np.float32)
    p = int_bf16(rng, (n, d), -3, 3)
    p[nbig:, 16:] = 0
    p[:nbig] = u[None, :] * rng.integers(2, 4, size=(nbig, 1)).astype(np.float32)
    q = int_bf16(rng, (nq, d), -3, 3)
    q[1:, 16:] = -2 * u[16:]
    q[0] = 3 * u
    groups = np.empty(n, np.int64)
    groups[:nbig] = 123456789
    groups[nbig:] = sized_groups(rng, n - nbig, 1, 4)
    perm = rng.permutation(n)                               # scatter the big group's rows over the ids
    return q, p[perm], groups[perm]


def test_two_rungs(dev):
    """n = 6000, k = 10, one group of 2500 rows on top for query 0: its first 2048 rows show one group, so it --
    and only it -- is searched again at depth min(10 * 2500, 6000) = 6000."""
    from denseretrievaltoolkits_amd import kernels
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    rng = np.random.default_rng(32)
    q, p, groups = dominated(rng, 6000, 2500)
    S = q.astype(np.float64) @ p.astype(np.float64).T
    for j in range(q.shape[0]):                             # the precondition, in numpy
        shown = np.unique(groups[np.lexsort((np.arange(6000), -S[j]))[:2048]]).size
        assert shown < 10 if j == 0 else shown >= 10, (j, shown)
    idx = FlatIPIndex(64, device=dev)
    idx.add(to_dev_bf16(p, dev))
    idx.set_groups(groups)
    assert idx._p_max == 2500 and kernels.grouped_depths(10, 2500, 6000) == (2048, 6000)
    calls = []
    inner = idx.search_batches_iter

    def spy(batches, k, *a, **kw):
        batches = list(batches)
        calls.append((k, [int(b.shape[0]) for b in batches]))
        return inner(batches, k, *a, **kw)

    idx.search_batches_iter = spy
    got = idx.search_grouped(q, 10)
    assert calls == [(2048, [q.shape[0]]), (6000, [1])]
    assert_equal(got[:3], brute_force(q, p, groups, 10))
    assert got[3][0] >= 10 and got[0][0, 0] == 3 * 3 * 64 and got[1][0, 0] == 123456789


def test_refusal_when_no_depth_certifies(dev):
    """n = 40000, k = 2, one group of 33000 rows on top for query 0: even the deepest list (32768 rows) shows one
    group and is not the whole corpus, so there is no certified answer -- ValueError, not a guess."""
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    rng = np.random.default_rng(33)
    q, p, groups = dominated(rng, 40000, 33000)
    idx = FlatIPIndex(64, device=dev)
    idx.add(to_dev_bf16(p, dev))
    idx.set_groups(groups)
    with pytest.raises(ValueError, match=r"\b1 queries .*32768.* 40000"):
        idx.search_grouped(q, 2)
    assert_equal(idx.search_grouped(q[1:], 2)[:3], brute_force(q[1:], p, groups, 2))


def test_set_groups_handling(dev, one_rung):
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    f = one_rung
    idx = FlatIPIndex(64, device=dev)
    with pytest.raises(ValueError, match="set_groups"):
        idx.search_grouped(f["q"][:2], 5)
    idx.add(to_dev_bf16(f["p"][:1000], dev))
    for bad in (np.array([0, -1, 3]), np.array([0, 2 ** 31]), np.zeros((10, 2), np.int64), np.zeros(10, np.float32)):
        with pytest.raises(ValueError):
            idx.set_groups(bad)
    idx.set_groups(f["groups"][:1000])
    assert_equal(idx.search_grouped(f["q"][:3], 5)[:3], brute_force(f["q"][:3], f["p"][:1000], f["groups"][:1000], 5))
    idx.add(to_dev_bf16(f["p"][1000:1010], dev))
    with pytest.raises(ValueError, match="1000 .*1010"):
        idx.search_grouped(f["q"][:3], 5)
    idx.reset()
    assert idx._groups is None
    idx.add(to_dev_bf16(f["p"][:1000], dev))
    with pytest.raises(ValueError, match="set_groups"):
        idx.search_grouped(f["q"][:3], 5)


def test_sharded_single_process_equals_flat(dev, one_rung):
    from denseretrievaltoolkits_amd.search import ShardedFlatIP
    f = one_rung
    sh = ShardedFlatIP(64, device=dev)
    sh.add_shard(to_dev_bf16(f["p"], dev))
    sh.set_groups(f["groups"])
    qd = to_dev_bf16(f["q"], dev)
    for k in (10, 100):
        a = sh.search_grouped(qd, k)
        b = f["idx"].search_grouped(qd, k)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert_equal(a[:3], [w[:, :k] for w in f["want"]])
    res = list(sh.search_grouped_batches_iter([qd[:50], qd[50:]], 10))
    assert [tuple(r[1].shape) for r in res] == [(50, 10), (83, 10)]
    np.testing.assert_array_equal(sh.search_grouped_device(qd[:50], 10)[1].cpu().numpy(), f["want"][1][:50, :10])


def test_retriever(dev, one_rung):
    from denseretrievaltoolkits_amd.evaluator.index import BaseFaissIPRetriever
    f = one_rung
    ret = BaseFaissIPRetriever(64, device=dev)
    ret.add(to_dev_bf16(f["p"], dev))
    es, eg, er = (w[:, :10] for w in f["want"])
    g1 = ret.search_grouped(f["q"], 10, groups=f["groups"])
    np.testing.assert_array_equal(g1, eg)
    np.testing.assert_array_equal(ret.last_scores, es)
    np.testing.assert_array_equal(ret.last_rows, er)
    ret.last_scores = ret.last_rows = None
    g2 = ret.batch_search_grouped(f["q"], 10, 48)            # groups=None: what the first call stored
    np.testing.assert_array_equal(g2, g1)
    np.testing.assert_array_equal(ret.last_scores, es)
    np.testing.assert_array_equal(ret.last_rows, er)
    # consistent among themselves: each hit's row belongs to its group and scores what is reported
    np.testing.assert_array_equal(f["groups"][ret.last_rows], g2)
    S = f["q"].astype(np.float64) @ f["p"].astype(np.float64).T
    np.testing.assert_array_equal(np.take_along_axis(S, ret.last_rows, 1).astype(np.float32), ret.last_scores)

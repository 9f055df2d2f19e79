"""The one-GPU group filter as interleaved passes with a threshold tightened after the first pass
(kernels.filter_passes_into / drt_ip_topk_filter_passes, search.TIGHTEN_AFTER_FIRST_PASS).

Pass p of P scans the 16-row tiles t with t % P == p.  Pass 0 filters against the sample threshold
tau0; each query's threshold is then raised to tau1 = the score of the r-th best key pass 0 collected
(tau0 where it collected fewer than r) and the other passes filter against tau1 into the same lists.
The list then holds every row >= tau1 plus pass-0 rows in [tau0, tau1), so a tightened query is
certified only if r_eff + (hits of passes 1..) >= the list width, r_eff = pass-0 hits >= tau1.

The protocol is restated below in numpy on top of oracle.search_oracle; integer-valued inputs make
every score exact, so tau1, the counts, the packed lists and the flag word are compared bit for bit.
"""
import math

import numpy as np
import pytest

from helpers import int_bf16, gauss_bf16, to_dev_bf16
from oracle import search_oracle as orc

pytestmark = pytest.mark.gpu

TILE = 16


def tighten_rank(n, npasses, k):
    """drt_ip_topk_tighten_rank: smallest r with C r - 5 sqrt(C (C - 1) r + (C - 1) r) >= k, C = shard
    tiles / pass-0 tiles; 0 when there is nothing to tighten."""
    if n <= 0 or npasses <= 1:
        return 0
    tall = -(-n // TILE)
    t0 = -(-tall // npasses)
    if t0 >= tall:
        return 0
    c = tall / t0
    r = 1
    while c * r - 5.0 * math.sqrt(c * (c - 1.0) * r + (c - 1.0) * r) < k:
        r += 1
    return r


def restate(q, p, k, tau0, npasses, r=None):
    """The tightened protocol on the host: (tau1 [nq] f32, c0 [nq], r_eff [nq], tightened [nq] bool,
    packed [nq, k + 1] u64 with the flag word, failing [nq] bool = tightened and not certified)."""
    nq, n = q.shape[0], p.shape[0]
    cap = orc.dist_plan(n, n, k)["cap"]
    r = tighten_rank(n, npasses, k) if r is None else r
    s = orc._scores_f32(q, p)
    in0 = (np.arange(n) // TILE) % npasses == 0
    tau1 = np.array(tau0, dtype=np.float32)
    c0 = np.zeros(nq, np.int64)
    r_eff = np.zeros(nq, np.int64)
    tight = np.zeros(nq, bool)
    failing = np.zeros(nq, bool)
    packed = np.full((nq, k + 1), orc.PAD_KEY64, dtype=np.uint64)
    for i in range(nq):
        hit0 = in0 & (s[i] >= tau0[i])
        c0[i] = hit0.sum()
        r_eff[i] = c0[i]
        if r > 0 and r <= c0[i] <= cap and not np.isnan(tau0[i]):
            tau1[i] = -np.sort(-s[i, hit0])[r - 1]
            r_eff[i] = (s[i, hit0] >= tau1[i]).sum()
            tight[i] = tau1[i] > tau0[i]
        later = ~in0 & (s[i] >= tau1[i])
        sel = np.nonzero(hit0 | later)[0]
        failing[i] = tight[i] and r_eff[i] + later.sum() < k
        flags = (1 if (len(sel) > cap or failing[i]) else 0) | (2 if len(sel) > k else 0)
        keys = np.sort((orc.desc_key(s[i, sel]).astype(np.uint64) << np.uint64(32)) | sel.astype(np.uint64))[:k]
        packed[i, :len(keys)] = keys
        packed[i, k] = (np.uint64(len(keys)) << np.uint64(32)) | np.uint64(flags)
    return tau1, c0, r_eff, tight, packed, failing


def run_passes(dev, qt, pt, k, tau, npasses, r=-1):
    """(packed, tau1, pass0) of kernels.filter_passes_into, on the host."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    nq, n = qt.shape[0], pt.shape[0]
    packed = torch.full((nq, k + 1), -7, dtype=torch.int64, device=dev)
    tau1 = torch.full((nq,), 123.0, dtype=torch.float32, device=dev)
    pass0 = torch.full((nq, 4), -1, dtype=torch.int32, device=dev)
    kernels.filter_passes_into(qt, pt, n, k, 0, tau, npasses, packed, r=r, tau1=tau1, pass0=pass0)
    torch.cuda.synchronize()
    return packed, tau1.cpu().numpy(), pass0.cpu().numpy().astype(np.int64)


INT_SHAPES = [
    (300, 50011, 768, 100, 4),   # 32-query kernel, partial last tile, partial query block
    (33, 20000, 128, 10, 8),     # 16-query kernel
    (257, 5003, 64, 10, 8),      # d = 64: a tile is 2 DMA instructions for 8 waves
    (129, 100, 320, 10, 8),      # fewer tiles than passes: some passes are empty
    (64, 3, 128, 10, 8),         # fewer rows than k
]
_int_runs = {}


def int_run(dev, shape):
    """One run per shape, shared by the tests below: inputs, the whole-shard filter, the new entry's
    outputs and the host restatement."""
    if shape in _int_runs:
        return _int_runs[shape]
    import torch
    from denseretrievaltoolkits_amd import kernels
    nq, n, d, k, npasses = shape
    rng = np.random.default_rng(nq + n + d + k)
    q = int_bf16(rng, (nq, d), -4, 4)
    p = int_bf16(rng, (n, d), -4, 4)
    qt, pt = to_dev_bf16(q, dev), to_dev_bf16(p, dev)
    tau = kernels.dist_tau(kernels.dist_sample(qt, pt, n, k).unsqueeze(0), k)
    whole = torch.empty((nq, k + 1), dtype=torch.int64, device=dev)
    kernels.dist_filter_into(qt, pt, n, k, 0, tau, whole)
    packed, tau1, pass0 = run_passes(dev, qt, pt, k, tau, npasses)
    s, i, st = kernels.merge_packed(packed.unsqueeze(0), k, n)
    out = dict(q=q, p=p, tau0=tau.cpu().numpy(), whole=whole, packed=packed, tau1=tau1, pass0=pass0,
               merged=(s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()),
               restated=restate(q, p, k, tau.cpu().numpy(), npasses), rank=kernels.tighten_rank(n, npasses, k))
    _int_runs[shape] = out
    return out


@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_passes_integer_bit_exact(dev, shape):
    """Heavy ties (integers in -4..4: rows equal to tau1 are common).  The packed lists equal
    dist_filter_into's over the whole shard entry for entry, flag word included, and the merged result
    is the oracle's."""
    import torch
    nq, n, d, k, npasses = shape
    run = int_run(dev, shape)
    assert torch.equal(run["packed"], run["whole"])
    np.testing.assert_array_equal(run["packed"].cpu().numpy().view(np.uint64), run["restated"][4])
    s, i, st = run["merged"]
    es, ei = orc.ip_topk(run["q"], run["p"], k)
    assert (st == 0).all()
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(s, es)


@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_tightened_threshold_white_box(dev, shape):
    """tau1 = the score of the r-th best key among the pass-0 tiles' rows >= tau0 (tau0 where there are
    fewer than r), tau1 >= tau0, c0 and r_eff (ties count) equal the numpy counts."""
    nq, n, d, k, npasses = shape
    run = int_run(dev, shape)
    tau1, c0, r_eff, tight, _, failing = run["restated"]
    assert run["rank"] == tighten_rank(n, npasses, k)
    np.testing.assert_array_equal(run["tau1"], tau1)
    assert (run["tau1"] >= run["tau0"]).all()
    if run["rank"] > 0:
        np.testing.assert_array_equal(run["pass0"][:, 0], c0)
        np.testing.assert_array_equal(run["pass0"][:, 1], r_eff)
        np.testing.assert_array_equal(run["pass0"][:, 2], tight.astype(np.int64))
        np.testing.assert_array_equal(run["tau1"][c0 < run["rank"]], run["tau0"][c0 < run["rank"]])
    else:
        assert (run["pass0"] == 0).all()
    assert not failing.any()
    # the three larger shapes do tighten; the two tiny ones cannot
    assert tight.any() == (n >= 5003)


def test_inactive_query_keeps_nan(dev):
    """A NaN threshold (an inactive query) stays NaN and collects nothing."""
    import torch
    rng = np.random.default_rng(3)
    nq, n, d, k = 5, 20000, 128, 10
    qt = to_dev_bf16(int_bf16(rng, (nq, d), -4, 4), dev)
    pt = to_dev_bf16(int_bf16(rng, (n, d), -4, 4), dev)
    tau = torch.tensor([float("nan"), 150.0, float("nan"), 150.0, 150.0], device=dev)
    packed, tau1, pass0 = run_passes(dev, qt, pt, k, tau, 8)
    assert np.isnan(tau1[[0, 2]]).all() and (tau1[[1, 3, 4]] >= 150.0).all()
    assert (pass0[[0, 2], 0] == 0).all()
    assert (packed[[0, 2], k].cpu().numpy() >> 32 == 0).all()


@pytest.fixture
def grouped_small():
    """The grouped path at test sizes; both constants restored afterwards."""
    from denseretrievaltoolkits_amd import search as srch
    saved = (srch.GROUP_MIN_ROWS, srch.GROUP_CHUNK_ROWS, srch.TIGHTEN_AFTER_FIRST_PASS)
    srch.GROUP_MIN_ROWS = 0
    yield srch
    srch.GROUP_MIN_ROWS, srch.GROUP_CHUNK_ROWS, srch.TIGHTEN_AFTER_FIRST_PASS = saved


@pytest.mark.parametrize("nq,n,d,k,chunk_rows", [
    (300, 60000, 768, 100, 15000),   # 4 passes
    (513, 30000, 128, 200, 3750),    # 8 passes
])
def test_passes_gaussian(dev, grouped_small, nq, n, d, k, chunk_rows):
    """Gaussian data (same fp32 chains in every kernel): the lists equal the whole-shard filter's at the
    same tau0, and FlatIPIndex.search_batches returns the fp64 order with the switch on and off, the
    same tensors both ways."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    srch = grouped_small
    srch.GROUP_CHUNK_ROWS = chunk_rows
    npasses = len(srch.group_chunks(n))
    assert npasses == -(-n // chunk_rows) > 1
    rng = np.random.default_rng(nq + n + d)
    q = gauss_bf16(rng, (nq, d))
    p = gauss_bf16(rng, (n, d))
    qt, pt = to_dev_bf16(q, dev), to_dev_bf16(p, dev)
    kc = kernels.refine_width(k)
    tau = kernels.dist_tau(kernels.dist_sample(qt, pt, n, k).unsqueeze(0), k)
    whole = torch.empty((nq, kc + 1), dtype=torch.int64, device=dev)
    kernels.dist_filter_into(qt, pt, n, kc, 0, tau, whole)
    packed, tau1, pass0 = run_passes(dev, qt, pt, kc, tau, npasses)
    assert torch.equal(packed, whole)
    assert (pass0[:, 2] == 1).any() and (tau1 >= tau.cpu().numpy()).all()

    index = FlatIPIndex.from_rows(pt)
    assert index._use_groups(k)
    batches = [qt[a: a + 128] for a in range(0, nq, 128)]
    res = {}
    for on in (True, False):
        srch.TIGHTEN_AFTER_FIRST_PASS = on
        out = index.search_batches(batches, k)
        res[on] = (torch.cat([s for s, _ in out]), torch.cat([i for _, i in out]))
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert index.group_fallbacks == 0 and index.resolved == 0
    _, ei = orc.ip_topk(q.astype(np.float64), p.astype(np.float64), k, dtype=np.float64, out_dtype=np.float64)
    np.testing.assert_array_equal(res[True][1].cpu().numpy(), ei)


def test_unrepresentative_first_pass_is_flagged(dev, grouped_small):
    """A corpus whose pass-0 tiles hold ALL the high-scoring rows of half the queries: their tau1 lands
    above what the rest of the shard can supply, so the certification count fails -- the native status
    flags exactly the restatement's failing queries, no query is certified with fewer than kc rows >=
    tau1, and search_batches still returns the oracle's result (the flagged batches are redone exactly)."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    srch = grouped_small
    nq, n, d, k, npasses = 160, 40000, 128, 10, 8
    srch.GROUP_CHUNK_ROWS = n // npasses
    assert len(srch.group_chunks(n)) == npasses
    kc = kernels.refine_width(k)
    r = tighten_rank(n, npasses, kc)
    rng = np.random.default_rng(17)
    q = int_bf16(rng, (nq, d), -4, 4)
    p = int_bf16(rng, (n, d), -4, 4)
    v = rng.choice([-4, -3, 3, 4], size=d).astype(np.float32)   # v . v ~ 12 sigma of an i.i.d. score
    nrig = r + 20
    assert r < nrig < kc
    # the rigged rows sit in pass-0 tiles (tile % npasses == 0), the rigged queries are the even ones
    rig_rows = np.array([(j // TILE) * npasses * TILE + j % TILE for j in range(nrig)])
    assert ((rig_rows // TILE) % npasses == 0).all() and rig_rows.max() < n
    for j, row in enumerate(rig_rows):
        p[row] = v
        p[row, j % d] = 0
    for j in range(0, nq, 2):
        q[j] = v
        q[j, (7 * j) % d] = 0
    qt, pt = to_dev_bf16(q, dev), to_dev_bf16(p, dev)
    tau = kernels.dist_tau(kernels.dist_sample(qt, pt, n, k).unsqueeze(0), k)
    tau1, c0, r_eff, tight, e_packed, failing = restate(q, p, kc, tau.cpu().numpy(), npasses)
    # both outcomes, asserted on the host first: every rigged query fails the count; an i.i.d. query fails
    # only where it happens to score the ~100 near-identical rigged rows high (they then crowd its pass 0 too)
    assert failing[0::2].all() and failing[1::2].mean() < 0.2

    packed, g_tau1, pass0 = run_passes(dev, qt, pt, kc, tau, npasses)
    np.testing.assert_array_equal(g_tau1, tau1)
    np.testing.assert_array_equal(pass0[:, 1], r_eff)
    np.testing.assert_array_equal(packed.cpu().numpy().view(np.uint64), e_packed)
    _, _, st = kernels.merge_packed(packed.unsqueeze(0), kc, n, k_cert=k)
    st = st.cpu().numpy()
    np.testing.assert_array_equal(st != 0, failing)
    s = orc._scores_f32(q, p)
    at_or_above = (s >= g_tau1[:, None]).sum(axis=1)
    assert (at_or_above[(st == 0) & (pass0[:, 2] == 1)] >= kc).all()

    index = FlatIPIndex.from_rows(pt)
    batches = [qt[a: a + 32] for a in range(0, nq, 32)]
    out = index.search_batches(batches, k)
    assert index.group_fallbacks == len(batches)   # every batch holds a rigged query
    es, ei = orc.ip_topk(q, p, k)
    np.testing.assert_array_equal(torch.cat([i for _, i in out]).cpu().numpy(), ei)
    np.testing.assert_array_equal(torch.cat([s for s, _ in out]).cpu().numpy(), es)


def test_first_pass_overflow_keeps_tau0_and_is_flagged(dev):
    """A pass-0 count above the list capacity keeps tau0 and raises the overflow flag (status 1), like
    test_dist_overflow_and_short_lists_are_flagged for the whole-shard entry."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    rng = np.random.default_rng(5)
    nq, n, d, k, npasses = 3, 80000, 128, 50, 2
    qt = to_dev_bf16(int_bf16(rng, (nq, d), -4, 4), dev)
    pt = to_dev_bf16(int_bf16(rng, (n, d), -4, 4), dev)
    cap = orc.dist_plan(n, n, k)["cap"]
    assert n // npasses > cap
    tau = torch.full((nq,), float("-inf"), device=dev)
    packed, tau1, pass0 = run_passes(dev, qt, pt, k, tau, npasses)
    assert np.isneginf(tau1).all()
    assert (pass0[:, 0] > cap).all() and (pass0[:, 2] == 0).all()
    assert (packed[:, k].cpu().numpy() & 1).all()
    _, _, st = kernels.merge_packed(packed.unsqueeze(0), k, n)
    assert (st.cpu().numpy() == 1).all()

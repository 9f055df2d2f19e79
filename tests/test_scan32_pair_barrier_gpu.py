"""ip_scan32r_kernel (the grouped filter scan, more than 256 queries per launch) synchronises its
work-group once per PAIR of 16-row corpus tiles: waves drift by up to two tiles inside a 6-slot ring.
A ring hazard (a slot refilled while a wave still reads it, or read before every wave's share landed)
shows up as a wrong fragment -- a wrong score, a missing or a spurious hit -- not as a fault, so the
packed lists are compared with a host restatement entry for entry, flag word included, for every query.

Shapes: blocks with every short or odd trip count (1 .. 8 tiles, neighbouring blocks differing by one:
with 2048 queries the grid is 32 x 8, one tile per block below 8 tiles; with 300 queries 128 x 2),
partial last tiles, partial query blocks, d = 64 (a tile is 2 DMA pieces for 8 waves) and 320,
interleaved passes (empty passes, unequal tile counts), a long run with hits in almost every wave-tile,
and a repeat-equality run on Gaussian data.

Integer-valued bf16 inputs make every score exact in fp32, so oracle.search_oracle.dist_filter restates
kernels.dist_filter_into bit for bit; the interleaved passes with their tightened threshold are restated
below (as in test_group_tighten_gpu.py).  Gaussian scores are fp32 chains of 24 MFMA steps, which numpy
cannot repeat bit for bit: there the first 64 queries' lists are pinned by the exact fp64 scores and the
chain's error bound eps (refine.hip, "Error bound"): every listed score within eps of the exact one, the
keys ascending, and no unlisted row scoring above the last listed score + eps.
"""
import math

import numpy as np
import pytest

from helpers import int_bf16, to_dev_bf16
from oracle import search_oracle as orc

pytestmark = pytest.mark.gpu

TILE = 16
K = 1000
_queries = {}


def int_queries(dev, nq, d):
    """(host, device) integer-valued queries, one set per (nq, d) shared by the cases."""
    if (nq, d) not in _queries:
        q = int_bf16(np.random.default_rng(1000 * nq + d), (nq, d), -4, 4)
        _queries[(nq, d)] = (q, to_dev_bf16(q, dev))
    return _queries[(nq, d)]


def int_corpus(dev, n, d):
    p = int_bf16(np.random.default_rng(7 * n + d), (n, d), -4, 4)
    return p, to_dev_bf16(p, dev)


def sampled_tau(qt, pt, n, k):
    from denseretrievaltoolkits_amd import kernels
    return kernels.dist_tau(kernels.dist_sample(qt, pt, n, k).unsqueeze(0), k)


def filter_into(dev, qt, pt, k, tau):
    """kernels.dist_filter_into into a fresh buffer -> uint64 [nq, k + 1] on the host."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    nq, n = qt.shape[0], pt.shape[0]
    packed = torch.full((nq, k + 1), -7, dtype=torch.int64, device=dev)
    kernels.dist_filter_into(qt, pt, n, k, 0, tau, packed)
    torch.cuda.synchronize()
    return packed.cpu().numpy().view(np.uint64)


def check_whole(dev, nq, n, d, k=K, tau_value=None):
    import torch
    q, qt = int_queries(dev, nq, d)
    p, pt = int_corpus(dev, n, d)
    if tau_value is None:
        tau = sampled_tau(qt, pt, n, k)
    else:
        tau = torch.full((nq,), tau_value, dtype=torch.float32, device=dev)
    got = filter_into(dev, qt, pt, k, tau)
    want = orc.dist_filter(q, p, n, k, 0, tau.cpu().numpy())
    np.testing.assert_array_equal(got, want)
    return want


# per-block tile counts 1 .. 8 at a 32 x 8 grid; "- 5": the shard's last tile is short
@pytest.mark.parametrize("short", [0, 5], ids=["full", "partial"])
@pytest.mark.parametrize("tiles", [1, 7, 8, 31, 33, 64, 65, 97, 129, 161, 193, 225])
def test_trip_counts_2048_queries(dev, tiles, short):
    check_whole(dev, 2048, TILE * tiles - short, 768)


# a 128 x 2 grid with a partial query block: m and m + 1 tiles per block
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_trip_counts_300_queries(dev, m):
    check_whole(dev, 300, TILE * 128 * m + 11, 768)


@pytest.mark.parametrize("d", [64, 320])
def test_small_d(dev, d):
    check_whole(dev, 1030, 5003, d)


def test_long_drift_hits_everywhere(dev):
    """About one score in ten is a hit (integers in -4 .. 4 at d = 768: sigma = 184.8, tau = 1.28 sigma):
    nearly every wave-tile takes the append path and the wave segments flush constantly while the ring
    turns 41 or 42 times per block.  No list overflows (the most hits of a query stay far below cap)."""
    n = TILE * 128 * 41 + 5
    want = check_whole(dev, 300, n, 768, tau_value=237.0)
    # (fp32 BLAS is exact on these integers: |score| <= 768 * 16)
    hits = (int_queries(dev, 300, 768)[0] @ int_corpus(dev, n, 768)[0].T >= 237.0).sum(axis=1)
    assert 0.07 * n < hits.mean() < 0.13 * n and hits.max() <= orc.dist_plan(n, n, K)["cap"]
    assert (want[:, K] == ((np.uint64(K) << np.uint64(32)) | np.uint64(2))).all()


def tighten_rank(n, npasses, k):
    """drt_ip_topk_tighten_rank (include/drt.h)."""
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


def restate_passes(q, p, k, tau0, npasses):
    """kernels.filter_passes_into on the host: pass 0 (tiles t with t % npasses == 0) against tau0, the
    others against tau1 = the r-th best pass-0 score (tau0 where pass 0 collected fewer than r or
    overflowed) -> packed [nq, k + 1] u64 with the flag word."""
    nq, n = q.shape[0], p.shape[0]
    cap = orc.dist_plan(n, n, k)["cap"]
    r = tighten_rank(n, npasses, k)
    s = orc._scores_f32(q, p)
    in0 = (np.arange(n) // TILE) % npasses == 0
    packed = np.full((nq, k + 1), orc.PAD_KEY64, dtype=np.uint64)
    for i in range(nq):
        hit0 = in0 & (s[i] >= tau0[i])
        c0 = int(hit0.sum())
        tau1, r_eff, tight = tau0[i], c0, False
        if r > 0 and r <= c0 <= cap and not np.isnan(tau0[i]):
            tau1 = -np.sort(-s[i, hit0])[r - 1]
            r_eff = int((s[i, hit0] >= tau1).sum())
            tight = tau1 > tau0[i]
        later = ~in0 & (s[i] >= tau1)
        sel = np.nonzero(hit0 | later)[0]
        failing = tight and r_eff + int(later.sum()) < k
        flags = (1 if (len(sel) > cap or failing) else 0) | (2 if len(sel) > k else 0)
        keys = np.sort((orc.desc_key(s[i, sel]).astype(np.uint64) << np.uint64(32)) | sel.astype(np.uint64))[:k]
        packed[i, :len(keys)] = keys
        packed[i, k] = (np.uint64(len(keys)) << np.uint64(32)) | np.uint64(flags)
    return packed


# 8 interleaved passes at a 128 x 2 grid: a long shard; fewer tiles than passes (some passes are empty);
# 26 tiles = passes of 4 and 3 tiles (the odd / even pair boundary under the pass's tile stride)
@pytest.mark.parametrize("n", [50011, 100, TILE * 8 * 3 + TILE * 2])
def test_interleaved_passes(dev, n):
    import torch
    from denseretrievaltoolkits_amd import kernels
    nq, d, k, npasses = 300, 768, 100, 8
    q, qt = int_queries(dev, nq, d)
    p, pt = int_corpus(dev, n, d)
    tau = sampled_tau(qt, pt, n, k)
    packed = torch.full((nq, k + 1), -7, dtype=torch.int64, device=dev)
    kernels.filter_passes_into(qt, pt, n, k, 0, tau, npasses, packed)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(packed.cpu().numpy().view(np.uint64),
                                  restate_passes(q, p, k, tau.cpu().numpy(), npasses))


def chain_eps(q64, pp):
    """refine.hip's bound of the 24-step fp32 chain: 10 u (1 + 1e-3) (sum_{t<T} Qp_t Pp_t + ||q|| Pp_T),
    Qp_t = ||q[:32 t]||, Pp_t = max over rows of ||p[:32 t]|| (``pp`` [T], t = 1 .. T)."""
    T = q64.shape[1] // 32
    qp = np.sqrt(np.cumsum((q64 ** 2).reshape(q64.shape[0], T, 32).sum(axis=2), axis=1))   # [nq, T]
    return 10.0 * 2.0 ** -24 * (1.0 + 1e-3) * ((qp[:, :T - 1] * pp[None, :T - 1]).sum(axis=1) + qp[:, T - 1] * pp[T - 1])


def test_repeats_equal_gaussian(dev):
    """The same launch ten times into fresh buffers: ten equal outputs (an intermittent wrong fragment
    would differ between runs), and the first 64 queries' lists against the exact fp64 scores."""
    import torch
    nq, n, d, k, nchk = 2048, 200_000, 768, K, 64
    g = torch.Generator(device=dev).manual_seed(20)
    pt = torch.randn((n, d), generator=g, device=dev).to(torch.bfloat16)
    qt = torch.randn((nq, d), generator=g, device=dev).to(torch.bfloat16)
    tau = sampled_tau(qt, pt, n, k)
    runs = [filter_into(dev, qt, pt, k, tau) for _ in range(10)]
    for r in runs[1:]:
        np.testing.assert_array_equal(r, runs[0])

    q64 = qt[:nchk].double().cpu().numpy()
    exact = np.empty((nchk, n))
    for a in range(0, n, 50_000):
        exact[:, a: a + 50_000] = q64 @ pt[a: a + 50_000].double().cpu().numpy().T
    pp = pt.float().square().view(n, d // 32, 32).sum(dim=2).cumsum(dim=1).max(dim=0).values.sqrt().double().cpu().numpy()
    eps = chain_eps(q64, pp)
    tau_h = tau[:nchk].cpu().numpy().astype(np.float64)
    cap = orc.dist_plan(n, n, k)["cap"]
    got = runs[0][:nchk]
    for i in range(nchk):
        # the inputs: certainly more than k hits, certainly no overflow
        assert (exact[i] >= tau_h[i] + eps[i]).sum() > k and (exact[i] >= tau_h[i] - eps[i]).sum() <= cap
        assert got[i, k] == (np.uint64(k) << np.uint64(32)) | np.uint64(2)
        keys = got[i, :k]
        assert (keys[1:] > keys[:-1]).all()
        rows = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        score = orc.desc_key_to_score((keys >> np.uint64(32)).astype(np.uint32)).astype(np.float64)
        assert rows.max() < n and (np.abs(score - exact[i, rows]) <= eps[i]).all()
        assert (score >= tau_h[i]).all()
        rest = np.ones(n, bool)
        rest[rows] = False
        assert exact[i, rest].max() <= score[-1] + eps[i]

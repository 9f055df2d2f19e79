"""The hit path of ip_scan32r_kernel (the grouped filter scan, more than 128 queries per launch): the
per-set check that skips a tile without hits, the per-row test, the wave's LDS hit segment and its flush
to the per-query lists.  Contract pinned here: a query's count is the exact number of rows scoring >= its
tau, its list holds exactly those (desc_key | row) entries, and a list that outgrows cap is flagged.

The launches are driven as in test_scan32_pair_barrier_gpu.py (kernels.dist_filter_into, and
kernels.filter_passes_into for the interleaved passes); the packed result -- the sorted entries, the count
and the flag word of every query -- is compared with the host restatement oracle.search_oracle.dist_filter:
numpy fp32 scores of the same bf16 data, the threshold applied per query.  Integer-valued inputs make
every score exact in fp32.  With k = 2048 >= every query's hits the sorted list IS the hit set (compared
order-free) and the count word the exact count; the cases that must show more hits than a list carries
say so.

Shapes: d = 768 and 128 (tiles issued by the loader half) and d = 64 (every wave issues); 256 queries,
and 288 and 300 (a second, partly empty work-group: a wave with 32 valid queries next to none, and one with
12 -- lanes of invalid queries hold a NaN tau).  With these query counts the grid is 128 x 2 work-groups, so
16 * 37 + 5 and 16 * 4 + 1 rows (a short last tile: the row bound) give a block one tile -- the epilogue after
the loop, which tests the row bound; 16 * 200 rows give one or two, and 16 * 128 * 3 + 5 rows three or four
(and 3 tiles + the short one in the last block): the epilogue inside the loop, whose three-instruction
prefilter skips a set's tile when no score of it reaches tau.  Densities: none; one to three hits per QUERY
over the long shard (a set's tile then holds at most a single hit, in any of a lane's four rows, scoring
exactly tau: a prefilter that dropped an operand or compared > would lose it); one score in ten; 64, 65,
128, 129 hits in ONE wave (the wave's 128-entry segment exactly full and one over, which flushes it); about
half of all scores (every tile overflows the segment: a blocking flush per ballot); everything (tau = -inf)
within k, beyond k and beyond cap.  Passes: 8 interleaved passes with the hits confined to the tiles of
pass 0, 3 or 7, everywhere, and one pass.
"""
import numpy as np
import pytest

from helpers import int_bf16, to_dev_bf16
from oracle import search_oracle as orc

pytestmark = pytest.mark.gpu

TILE = 16
K = 2048          # widest list (cap = 32768); every case but the stated ones has <= K hits per query
N_TAIL = TILE * 37 + 5
N_TINY = TILE * 4 + 1
N_FLUSH = TILE * 200
N_LONG = TILE * 128 * 3 + 5   # 3 or 4 tiles per block at a 128 x 2 grid
DIMS = [768, 128, 64]
_data = {}


def sigma(d):
    """Standard deviation of a score: integers uniform in -4 .. 4 have variance 20 / 3."""
    return (20.0 / 3.0) * np.sqrt(d)


def data(dev, nq, n, d):
    """(host q, device q, host p, device p) shared by the cases of one shape."""
    key = (nq, n, d)
    if key not in _data:
        q = int_bf16(np.random.default_rng(31 * nq + d), (nq, d), -4, 4)
        p = int_bf16(np.random.default_rng(17 * n + d), (n, d), -4, 4)
        _data[key] = (q, to_dev_bf16(q, dev), p, to_dev_bf16(p, dev))
    return _data[key]


def launch(dev, qt, pt, k, tau, npasses=None):
    """packed uint64 [nq, k + 1] of one grouped filter launch (or of ``npasses`` interleaved ones, no
    tightening) into a fresh buffer."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    nq, n = qt.shape[0], pt.shape[0]
    packed = torch.full((nq, k + 1), -7, dtype=torch.int64, device=dev)
    taut = torch.from_numpy(np.array(tau, dtype=np.float32)).to(dev)
    if npasses is None:
        kernels.dist_filter_into(qt, pt, n, k, 0, taut, packed)
    else:
        kernels.filter_passes_into(qt, pt, n, k, 0, taut, npasses, packed, r=0)
    torch.cuda.synchronize()
    return packed.cpu().numpy().view(np.uint64)


def check(dev, q, qt, p, pt, tau, k=K, npasses=None, visible=True):
    """Launch and compare with the restatement; -> hits per query (restated).  ``visible``: the case is
    meant to show every hit (no query above k)."""
    n = p.shape[0]
    tau = np.broadcast_to(np.asarray(tau, np.float32), (q.shape[0],))
    hits = (orc._scores_f32(q, p) >= tau[:, None]).sum(axis=1)
    assert hits.max() <= orc.dist_plan(n, n, k)["cap"]
    assert (hits.max() <= k) == visible
    got = launch(dev, qt, pt, k, tau, npasses)
    want = orc.dist_filter(q, p, n, k, 0, tau)
    print(f"nq={q.shape[0]} n={n} d={q.shape[1]} hits/query min {hits.min()} mean {hits.mean():.1f} max {hits.max()}; "
          f"count words equal: {(got[:, k] == want[:, k]).all()}, entries equal: {(got[:, :k] == want[:, :k]).all()}")
    np.testing.assert_array_equal(got[:, k] >> np.uint64(32), np.minimum(hits, k).astype(np.uint64))
    np.testing.assert_array_equal(got, want)
    return hits


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", [N_TAIL, N_TINY, N_FLUSH])
def test_no_hits(dev, n, d):
    q, qt, p, pt = data(dev, 300, n, d)
    assert check(dev, q, qt, p, pt, 1e9).sum() == 0


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("nq", [256, 288, 300])
@pytest.mark.parametrize("n", [N_TAIL, N_FLUSH, N_LONG])
def test_rare_hits(dev, n, nq, d):
    """About one score in ten: most set-tiles hold a hit or two, a wave's segment takes a block's hits without
    a flush before the final one."""
    q, qt, p, pt = data(dev, nq, n, d)
    hits = check(dev, q, qt, p, pt, 1.28 * sigma(d))
    assert 0.05 * n < hits.mean() < 0.15 * n


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("nq", [256, 288, 300])
def test_half_of_all_scores(dev, nq, d):
    """Half of the scores are hits: ~256 per wave and tile against a segment of 128, so the wave flushes (and
    blocks) at every other ballot."""
    q, qt, p, pt = data(dev, nq, N_FLUSH, d)
    hits = check(dev, q, qt, p, pt, 0.5)
    assert 0.4 * N_FLUSH < hits.min()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("nq", [256, 300])
@pytest.mark.parametrize("n", [N_TAIL, N_TINY])
def test_every_row_is_a_hit(dev, n, nq, d):
    """tau = -inf, n <= k <= cap: every list holds every row."""
    q, qt, p, pt = data(dev, nq, n, d)
    assert (check(dev, q, qt, p, pt, -np.inf) == n).all()


@pytest.mark.parametrize("d", DIMS)
def test_every_row_beyond_k(dev, d):
    """tau = -inf, k < n <= cap: the best k of every row, the count k, flag bit 1 (truncated)."""
    q, qt, p, pt = data(dev, 300, N_FLUSH, d)
    assert (check(dev, q, qt, p, pt, -np.inf, visible=False) == N_FLUSH).all()


@pytest.mark.parametrize("d", DIMS)
def test_every_row_beyond_cap(dev, d):
    """tau = -inf with more rows than cap: the counters run past cap, entries past it are dropped and the
    list is flagged overflowed (bit 0) and truncated (bit 1) with k entries.  Which cap entries are kept
    depends on the order the waves arrive in -- on any build, the parent's included -- so the stored prefix
    is not compared entry for entry with another run's: the count and flag word must be the parent's (the
    restatement's), and the kept entries distinct real hits with their true scores."""
    k = 1000
    n = orc.dist_plan(1, 1, k)["cap"] + TILE * 3 + 5
    q, qt, p, pt = data(dev, 300, n, d)
    assert n > orc.dist_plan(n, n, k)["cap"]
    got = launch(dev, qt, pt, k, np.full(300, -np.inf, np.float32))
    np.testing.assert_array_equal(got[:, k], np.full(300, (k << 32) | 3, np.uint64))
    keys = got[:, :k]
    assert (keys[:, 1:] > keys[:, :-1]).all()
    rows = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert rows.max() < n
    s = orc._scores_f32(q, p)
    np.testing.assert_array_equal((keys >> np.uint64(32)).astype(np.uint32),
                                  orc.desc_key(np.take_along_axis(s, rows, axis=1)))


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("nq", [256, 300])
@pytest.mark.parametrize("rank", [1, 3])
def test_single_hits_in_long_blocks(dev, rank, nq, d):
    """tau = each query's own ``rank``-th best score over 3 to 4 tiles per block: a set's tile (16 queries x 16
    rows) holds a hit with probability 1 / 8 at most, so nearly every hit is the only score of its lane, set and
    tile to reach tau -- in whichever of the lane's four rows it lies -- and each query has one that equals
    tau."""
    q, qt, p, pt = data(dev, nq, N_LONG, d)
    s = orc._scores_f32(q, p)
    tau = -np.sort(-s, axis=1)[:, rank - 1]
    hits = check(dev, q, qt, p, pt, tau)
    assert (s == tau[:, None]).any(axis=1).all() and rank <= hits.min() and hits.mean() < rank + 1
    hit_rows = np.nonzero(s >= tau[:, None])[1]
    assert set(hit_rows % 4) == {0, 1, 2, 3}   # every accumulator element holds some query's hit


def taus_for_total(s, total):
    """Per-query thresholds (each one of the query's own scores, or +inf) that admit exactly ``total`` of the
    scores s [nq, rows] in all: queries take turns lowering their threshold to their next distinct score."""
    nq = s.shape[0]
    vals = [np.unique(s[i])[::-1] for i in range(nq)]
    step = np.zeros(nq, int)   # distinct values admitted
    count = lambda i, t: int((s[i] >= vals[i][t - 1]).sum()) if t else 0
    have = 0
    for _ in range(64):
        for i in range(nq):
            if step[i] < len(vals[i]):
                more = count(i, step[i] + 1) - count(i, step[i])
                if have + more <= total:
                    step[i] += 1
                    have += more
        if have == total:
            break
    assert have == total
    return np.array([vals[i][step[i] - 1] if step[i] else np.inf for i in range(nq)], np.float32)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("total", [64, 65, 128, 129])
def test_segment_exactly_full_and_one_over(dev, total, d):
    """``total`` hits in one wave: queries 0 .. 31 (a wave's) over rows 0 .. 15 (one tile, and with five
    tiles at most one per work-group); the segment is 128 entries: 129 hits flush it once before the final
    flush, 64 and 65 stay within it."""
    q, qt, p, pt = data(dev, 288, N_TINY, d)
    tau = np.full(288, np.inf, np.float32)
    tau[:32] = taus_for_total(orc._scores_f32(q[:32], p[:TILE]), total)
    hits = check(dev, q, qt, p, pt, tau)
    assert (orc._scores_f32(q[:32], p[:TILE]) >= tau[:32, None]).sum() == total and hits[32:].sum() == 0


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", [N_TAIL, N_TINY])
def test_hits_only_in_the_short_tile(dev, n, d):
    """Only the rows of the shard's short last tile can score: the others are zero and tau > 0.  The last
    row is a hit of every query (a clamped or repeated source row would be one too), and the rows that
    follow the shard in memory score far above tau."""
    q, qt, _, _ = data(dev, 300, n, d)
    rng = np.random.default_rng(n + d)
    first = n - n % TILE
    p = np.zeros((n + TILE, d), np.float32)
    p[first:n] = int_bf16(rng, (n - first, d), -4, 4)
    p[n - 1] = 1.0
    p[n:] = 8.0
    q = np.abs(q) + 1.0   # every query scores > 0 against rows n - 1 and n ..
    qt, pt = to_dev_bf16(q, dev), to_dev_bf16(p, dev)
    tau = np.full(300, 0.5, np.float32)
    assert (orc._scores_f32(q, p[n - 1:]) >= 1.0).all()
    hits = check(dev, q, qt, p[:n], pt[:n], tau)
    assert hits.min() >= 1 and hits.max() <= n - first


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("hot", [0, 3, 7, None])
@pytest.mark.parametrize("n", [N_TAIL, N_FLUSH])
def test_eight_passes(dev, n, hot, d):
    """8 interleaved passes (pass j: the tiles t with t % 8 == j) appending to the same lists; ``hot``: only
    that pass's tiles can score (the other rows are zero, tau > 0), about half of them do."""
    q, qt, p, pt = data(dev, 300, n, d)
    if hot is None:
        check(dev, q, qt, p, pt, 1.28 * sigma(d), npasses=8)
        return
    live = (np.arange(n) // TILE) % 8 == hot
    p = np.where(live[:, None], p, 0.0).astype(np.float32)
    hits = check(dev, q, qt, p, to_dev_bf16(p, dev), 0.5, npasses=8)
    assert 0.4 * live.sum() < hits.mean() < 0.6 * live.sum()


@pytest.mark.parametrize("d", DIMS)
def test_one_pass(dev, d):
    q, qt, p, pt = data(dev, 300, N_FLUSH, d)
    check(dev, q, qt, p, pt, 0.5, npasses=1)

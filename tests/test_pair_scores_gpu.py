"""GPU: drt_pair_scores_bf16 (csrc/exclude.hip) -- the exact score of chosen (query, row) pairs, in the
numerics of the canonical search: the fp64 sum of the bf16 products rounded once to fp32.  Expected values
are numpy's fp64 dot products of the bf16-valued inputs, rounded to fp32."""
import numpy as np
import pytest

from helpers import gauss_bf16, int_bf16, to_dev_bf16

pytestmark = pytest.mark.gpu

PAD_S = np.float32(-3.402823466e+38)


def restate(q, p, qidx, rows):
    out = np.full(len(rows), PAD_S, np.float32)
    for j, (a, r) in enumerate(zip(qidx, rows)):
        if 0 <= r < p.shape[0]:
            out[j] = np.float32(q[a].astype(np.float64) @ p[r].astype(np.float64))
    return out


def run(dev, q, p, qidx, rows):
    import torch
    from denseretrievaltoolkits_amd import kernels
    out = kernels.pair_scores(to_dev_bf16(q, dev), to_dev_bf16(p, dev),
                              torch.from_numpy(np.asarray(qidx, np.int32)).to(dev),
                              torch.from_numpy(np.asarray(rows, np.int64)).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("d", [8, 64, 768, 1024])
def test_integer_fixture_exact(dev, d):
    """Integer-valued rows: every sum is exact in fp64 and in fp32, so the result equals numpy's exactly.
    d = 8 is one chunk of one lane, 64 directly (no padding), 1024 the second chunk of every lane; 1003 pairs
    leave the last work-group (4 pairs) partly empty."""
    rng = np.random.default_rng(d)
    q, p = int_bf16(rng, (9, d)), int_bf16(rng, (333, d))
    qidx = rng.integers(0, 9, size=1003)
    rows = rng.integers(0, 333, size=1003)
    np.testing.assert_array_equal(run(dev, q, p, qidx, rows), restate(q, p, qidx, rows))


def test_gaussian_within_one_ulp(dev):
    """d = 768 Gaussian rows: the fp64 accumulation error (~768 x 2^-53 relative to the sum of |products|) is
    far below an fp32 ulp, so only a sum next to an fp32 rounding boundary can round the other way, by one
    ulp."""
    rng = np.random.default_rng(21)
    q, p = gauss_bf16(rng, (16, 768)), gauss_bf16(rng, (2000, 768))
    qidx = rng.integers(0, 16, size=4001)
    rows = rng.integers(0, 2000, size=4001)
    got, want = run(dev, q, p, qidx, rows), restate(q, p, qidx, rows)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert (got == want).mean() > 0.99


def test_rows_outside_the_shard(dev):
    rng = np.random.default_rng(22)
    q, p = int_bf16(rng, (3, 64)), int_bf16(rng, (50, 64))
    qidx, rows = [0, 1, 2, 0, 1], [-1, 50, 49, 0, 1 << 40]
    got = run(dev, q, p, qidx, rows)
    np.testing.assert_array_equal(got, restate(q, p, qidx, rows))
    assert got[0] == PAD_S and got[1] == PAD_S and got[4] == PAD_S and got[2] != PAD_S


def test_through_an_index_with_padded_rows(dev):
    """d = 100 through FlatIPIndex (stored zero-padded to 128): the padding adds nothing."""
    import torch
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    rng = np.random.default_rng(23)
    q, p = gauss_bf16(rng, (5, 100)), gauss_bf16(rng, (700, 100))
    idx = FlatIPIndex(100, device=dev)
    idx.add(torch.from_numpy(p))
    assert idx.rows.shape[1] == 128
    qidx = rng.integers(0, 5, size=300)
    rows = rng.integers(0, 700, size=300)
    got = idx.pair_scores(torch.from_numpy(q), qidx, rows).cpu().numpy()
    want = restate(q, p, qidx, rows)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert idx.pair_scores(torch.from_numpy(q), [0], [700]).item() == PAD_S


def test_agrees_with_the_scores_the_search_reports(dev):
    """A pair taken from a query's own top-k: within one fp32 ulp of the score the canonical search reported
    for it (the search rounds fp32 score + fp32 delta, this kernel the fp64 sum itself)."""
    import torch
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    rng = np.random.default_rng(24)
    q, p = gauss_bf16(rng, (8, 768)), gauss_bf16(rng, (30000, 768))
    idx = FlatIPIndex.from_rows(to_dev_bf16(p, dev))
    s, i = idx.search_device(to_dev_bf16(q, dev), 50)
    qidx = torch.arange(8, device=dev).repeat_interleave(50)
    got = idx.pair_scores(to_dev_bf16(q, dev), qidx, i.reshape(-1)).reshape(8, 50)
    torch.cuda.synchronize()
    s, got = s.cpu().numpy(), got.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - s.astype(np.float64)) <= np.spacing(np.abs(s))).all()

"""ip_scan32r_kernel (the grouped filter scan) has ONE wave of each SIMD issue the ring refill: every tile
of a block is brought in whole by waves 4-7 (a loader half; the form in which the halves take turns, tile
t by half t & 1, was measured beside it and must pass the same cases), for the widths whose tile is a
multiple of four 1-KiB DMA pieces (d = 128, 256, .. 768); the other widths keep the eight-wave issue.
What can go wrong is the bookkeeping: a half that waits for the wrong number of its own pieces, a lane
offset or LDS address of one of the 2 .. 24 pieces, a block whose prologue leaves a half with nothing
issued, a block that ends on either tile of a pair, the clamped rows of a short last tile.  All of
these give a wrong fragment -- a wrong score, a missing or a spurious hit -- so the packed lists are
compared with a host restatement entry for entry, flag word included, for every query.

Shapes (beside those of test_scan32_pair_barrier_gpu.py):
  every piece count: d = 64 (2 pieces), 128 (4), 192 (6), 320 (10), 448 (14), 704 (22), 768 (24), each on a
    128 x 2 grid (300 queries) with m + 1 tiles in block 0 and m in the others, m = 1 .. 5, last tile short;
    d = 256, 384, 512, 640 (2 .. 5 pieces per loader wave) the same way with m = 2, 3;
  blocks of exactly 1, 2 and 3 tiles at d = 768 on the 32 x 8 grid of 2048 queries, full and short last tile;
  interleaved passes (3 and 8) whose neighbouring blocks differ by one tile, on shards whose last tile is
    short and falls into a different pass each;
  two runs on Gaussian data whose lists must hold the same keys per query.

Integer-valued bf16 inputs make every score exact in fp32, so oracle.search_oracle.dist_filter restates
kernels.dist_filter_into bit for bit; the interleaved passes are restated by the pair-barrier test's
restate_passes.
"""
import numpy as np
import pytest

import test_scan32_pair_barrier_gpu as pb

pytestmark = pytest.mark.gpu

TILE = pb.TILE
K = pb.K


# 128 m + 1 tiles over 128 blocks: block 0 walks m + 1 tiles, the others m; the last tile has 11 rows
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("d", [64, 128, 192, 320, 448, 704, 768])
def test_piece_counts_300_queries(dev, d, m):
    pb.check_whole(dev, 300, TILE * 128 * m + 11, d)


# the other widths issued by loader halves (8, 12, 16, 20 pieces: 2 .. 5 per loader wave, each its own
# issue statement), blocks of both parities
@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("d", [256, 384, 512, 640])
def test_other_half_widths_300_queries(dev, d, m):
    pb.check_whole(dev, 300, TILE * 128 * m + 11, d)


# every block exactly 1, 2 or 3 tiles (32 x 8 grid): the prologue issues everything, one half nothing
# (1 tile) or a single tile (2), and no refill is ever issued
@pytest.mark.parametrize("short", [0, 5], ids=["full", "partial"])
@pytest.mark.parametrize("tiles", [1, 2, 3])
def test_short_blocks_2048_queries(dev, tiles, short):
    pb.check_whole(dev, 2048, TILE * 32 * tiles - short, 768)


# a pass of 128 m + 64 (+ 1) tiles on the 128 x 2 grid: blocks 0 .. 63 (64) walk m + 1 tiles, the rest m.
# 3 passes of 320 / 320 / 319 tiles (short last tile in pass 1) and 321 / 320 / 320 (in pass 0);
# 8 passes of 193 x 3 + 192 x 5 tiles (short last tile in pass 2) and 192 x 8 + 1 (in pass 0)
@pytest.mark.parametrize("npasses,tall,rows_last", [(3, 959, 5), (3, 961, 9), (8, 1539, 9), (8, 1537, 3)])
def test_interleaved_passes_uneven_blocks(dev, npasses, tall, rows_last):
    import torch
    from denseretrievaltoolkits_amd import kernels
    nq, d, k = 300, 768, 100
    n = TILE * (tall - 1) + rows_last
    q, qt = pb.int_queries(dev, nq, d)
    p, pt = pb.int_corpus(dev, n, d)
    tau = pb.sampled_tau(qt, pt, n, k)
    packed = torch.full((nq, k + 1), -7, dtype=torch.int64, device=dev)
    kernels.filter_passes_into(qt, pt, n, k, 0, tau, npasses, packed)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(packed.cpu().numpy().view(np.uint64),
                                  pb.restate_passes(q, p, k, tau.cpu().numpy(), npasses))


def test_two_runs_same_sets_gaussian(dev):
    """Two launches on Gaussian data into fresh buffers: per query the same keys (compared as sets: the
    lists are sorted on the host side here, so the order a work-group appended them in does not count) and
    the same flag word."""
    import torch
    nq, n, d = 2048, 100_003, 768
    g = torch.Generator(device=dev).manual_seed(12)
    pt = torch.randn((n, d), generator=g, device=dev).to(torch.bfloat16)
    qt = torch.randn((nq, d), generator=g, device=dev).to(torch.bfloat16)
    tau = pb.sampled_tau(qt, pt, n, K)
    a = pb.filter_into(dev, qt, pt, K, tau)
    b = pb.filter_into(dev, qt, pt, K, tau)
    np.testing.assert_array_equal(a[:, K], b[:, K])
    assert ((a[:, K] >> np.uint64(32)) > 0).all()
    np.testing.assert_array_equal(np.sort(a[:, :K], axis=1), np.sort(b[:, :K], axis=1))

"""Host arithmetic of the tightened group filter (no GPU): drt_ip_topk_tighten_rank and the workspace
query of drt_ip_topk_filter_passes."""
import math


def _rank(n, npasses, k):
    tall = -(-n // 16)
    t0 = -(-tall // npasses)
    if n <= 0 or npasses <= 1 or t0 >= tall:
        return 0
    c = tall / t0
    r = 1
    while c * r - 5.0 * math.sqrt(c * (c - 1.0) * r + (c - 1.0) * r) < k:
        r += 1
    return r


def test_tighten_rank_matches_its_formula():
    from denseretrievaltoolkits_amd import kernels
    # the bench's group: 8 passes over 10M rows, list width refine_width(1000) = 1256
    assert kernels.refine_width(1000) == 1256
    r = kernels.tighten_rank(10_000_000, 8, 1256)
    assert r == _rank(10_000_000, 8, 1256) == 233
    # the mean count of rows at or above the new threshold stays 5 sigma above the list width
    assert 8 * r - 5 * math.sqrt(63 * r) >= 1256 > 8 * (r - 1) - 5 * math.sqrt(63 * (r - 1))
    for n, p, k in [(50011, 4, 100), (20000, 8, 10), (5003, 8, 266), (100, 8, 10), (40000, 8, 266)]:
        assert kernels.tighten_rank(n, p, k) == _rank(n, p, k) > 0
    # nothing to tighten: one pass, or a first pass that holds every tile
    assert kernels.tighten_rank(10_000_000, 1, 1256) == 0
    assert kernels.tighten_rank(3, 8, 10) == 0
    assert kernels.tighten_rank(0, 8, 10) == 0


def test_filter_passes_workspace_and_argument_checks():
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    ws = lib.drt_ip_topk_filter_passes_workspace(2048, 10_000_000, 10_000_000, 768, 1256)
    base = lib.drt_ip_topk_dist_workspace(2048, 10_000_000, 10_000_000, 768, 1256)
    assert ws >= base + 2048 * 16
    assert lib.drt_ip_topk_filter_passes_workspace(128, 1000, 1000, 100, 10) == 0   # d % 64 != 0
    # rejected before any HIP call: d > 768, no passes
    rc = lib.drt_ip_topk_filter_passes(None, 4, None, 1000, 1000, 832, 10, 0, None, None, 8, -1, None, None, None, 0,
                                       None)
    assert rc == _native.DRT_EINVAL
    rc = lib.drt_ip_topk_filter_passes(None, 4, None, 1000, 1000, 128, 10, 0, None, None, 0, -1, None, None, None, 0,
                                       None)
    assert rc == _native.DRT_EINVAL

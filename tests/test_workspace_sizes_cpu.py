"""The search workspace queries return what they returned before the layouts were restated.

tests/golden/workspace_sizes.json was recorded by tools/gen_workspace_sizes.py from the library of the
commit before csrc/search_internal.h stated each workspace layout once; every offset and total must have
stayed what it was (a region added to a size and not to its carve is an out-of-bounds device write that no
CPU test would see).  Pure host arithmetic: no GPU.
"""
import itertools
import json
import os

import pytest

from conftest import REPO

with open(os.path.join(REPO, "tests", "golden", "workspace_sizes.json")) as _f:
    GOLDEN = json.load(_f)


def _flat(case):
    out = []
    for x in case:
        out.extend(x if isinstance(x, list) else [x])
    return out


@pytest.fixture(scope="module")
def lib():
    from denseretrievaltoolkits_amd import _native
    return _native.load()


def test_every_pinned_query_is_recorded():
    assert sorted(GOLDEN["grids"]) == sorted([
        "drt_ip_topk_workspace", "drt_ip_topk_dist_workspace", "drt_ip_topk_filter_passes_workspace",
        "drt_ip_topk_resolve_workspace", "drt_ip_topk_resolve_wide_workspace", "drt_ip_topk_large_workspace",
        "drt_refine_width", "drt_ip_topk_sample_rank", "drt_ip_topk_tighten_rank"])
    g = GOLDEN["grids"]["drt_ip_topk_workspace"]
    assert g["axes"] == [[0, 1, 128, 129, 2048], [0, 1000, 16384, 16385, 70000, 1250000, 10000000],
                         [64, 768, 1024], [1, 10, 1000, 2048]]
    assert GOLDEN["grids"]["drt_ip_topk_resolve_workspace"]["axes"][0] == [1, 5, 128, 1000]
    assert GOLDEN["grids"]["drt_ip_topk_large_workspace"]["axes"][1] == [2049, 4096, 32768]


@pytest.mark.parametrize("fn", sorted(GOLDEN["grids"]))
def test_grid_values_unchanged(lib, fn):
    g = GOLDEN["grids"][fn]
    cases = list(itertools.product(*g["axes"]))
    assert len(cases) == len(g["values"])
    got = [int(getattr(lib, fn)(*_flat(c))) for c in cases]
    wrong = [(fn, _flat(c), want, have) for c, want, have in zip(cases, g["values"], got) if want != have]
    assert not wrong, f"{len(wrong)} of {len(cases)} differ, first (query, args, recorded, now): {wrong[0]}"
    if fn.endswith("_workspace"):
        assert any(v > 0 for v in got)


def test_rejected_shapes_stay_rejected(lib):
    assert GOLDEN["rejected"]
    for fn, args, want in GOLDEN["rejected"]:
        assert want in (0, -1), (fn, args, want)
        assert int(getattr(lib, fn)(*args)) == want, (fn, args)

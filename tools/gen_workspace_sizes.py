#!/usr/bin/env python3
"""Record what the search workspace queries return, for tests/test_workspace_sizes_cpu.py.

    DRT_LIB=/path/to/libdrt_hip.so python tools/gen_workspace_sizes.py [tests/golden/workspace_sizes.json]

Pure host arithmetic: no GPU is needed.  Run it against the library of the commit BEFORE a change of the
workspace layouts; the test then holds the change to those sizes.  The file lists, per query, the axes of
its argument grid and the values in itertools.product order of those axes (an axis entry that is a list is
several arguments, e.g. an (n_local, n_global) pair), plus single rejecting cases that must return 0 / -1.
"""
from __future__ import annotations

import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NQ = [0, 1, 128, 129, 2048]
N = [0, 1000, 16384, 16385, 70000, 1_250_000, 10_000_000]
D = [64, 768, 1024]
K = [1, 10, 1000, 2048]
SHARDS = [[n, n] for n in N] + [[n // 8, n] for n in N]   # (n_local, n_global)

GRIDS = {
    "drt_ip_topk_workspace": [NQ, N, D, K],
    "drt_ip_topk_dist_workspace": [NQ, SHARDS, D, K],
    "drt_ip_topk_filter_passes_workspace": [NQ, SHARDS, D, K],
    "drt_ip_topk_resolve_workspace": [[1, 5, 128, 1000], N, D],
    "drt_ip_topk_resolve_wide_workspace": [N, D],
    "drt_ip_topk_large_workspace": [D, [2049, 4096, 32768]],
    "drt_refine_width": [K],
    "drt_ip_topk_sample_rank": [K],
    "drt_ip_topk_tighten_rank": [[n for n, _ in SHARDS], [1, 2, 4, 8], K],
}

# [query, arguments]: rejected shapes
REJECTED = [
    ["drt_ip_topk_workspace", [128, 1000, 100, 10]],
    ["drt_ip_topk_workspace", [128, 1000, 1088, 10]],
    ["drt_ip_topk_workspace", [128, 1000, 768, 0]],
    ["drt_ip_topk_workspace", [128, 1000, 768, 2049]],
    ["drt_ip_topk_dist_workspace", [128, 1000, 8000, 100, 10]],
    ["drt_ip_topk_dist_workspace", [128, 1000, 8000, 1088, 10]],
    ["drt_ip_topk_dist_workspace", [128, 1000, 8000, 768, 0]],
    ["drt_ip_topk_dist_workspace", [128, 1000, 8000, 768, 2049]],
    ["drt_ip_topk_dist_workspace", [128, 8000, 1000, 768, 10]],
    ["drt_ip_topk_filter_passes_workspace", [128, 1000, 8000, 100, 10]],
    ["drt_ip_topk_filter_passes_workspace", [128, 1000, 8000, 1088, 10]],
    ["drt_ip_topk_filter_passes_workspace", [128, 1000, 8000, 768, 0]],
    ["drt_ip_topk_filter_passes_workspace", [128, 1000, 8000, 768, 2049]],
    ["drt_ip_topk_resolve_workspace", [5, 1000, 100]],
    ["drt_ip_topk_resolve_workspace", [5, 1000, 1088]],
    ["drt_ip_topk_resolve_workspace", [0, 1000, 768]],
    ["drt_ip_topk_resolve_wide_workspace", [1000, 100]],
    ["drt_ip_topk_resolve_wide_workspace", [1000, 1088]],
    ["drt_ip_topk_large_workspace", [100, 4096]],
    ["drt_ip_topk_large_workspace", [1088, 4096]],
    ["drt_ip_topk_large_workspace", [768, 0]],
    ["drt_ip_topk_large_workspace", [768, 32769]],
    ["drt_refine_width", [0]],
    ["drt_refine_width", [2049]],
    ["drt_ip_topk_sample_rank", [0]],
    ["drt_ip_topk_sample_rank", [2049]],
]


def flat(case):
    out = []
    for x in case:
        out.extend(x if isinstance(x, list) else [x])
    return out


def main() -> None:
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    rec = {"library": lib.drt_version().decode(), "grids": {}, "rejected": []}
    for fn, axes in GRIDS.items():
        vals = [int(getattr(lib, fn)(*flat(c))) for c in itertools.product(*axes)]
        rec["grids"][fn] = {"axes": axes, "values": vals}
    for fn, args in REJECTED:
        rec["rejected"].append([fn, args, int(getattr(lib, fn)(*args))])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("tests", "golden", "workspace_sizes.json")
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(out, sum(len(g["values"]) for g in rec["grids"].values()), "grid values,", len(rec["rejected"]), "rejected")


if __name__ == "__main__":
    main()

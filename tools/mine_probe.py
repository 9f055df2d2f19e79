#!/usr/bin/env python3
"""What hard-negative mining costs on top of the search it rides on: the bench's 10M x 768 corpus, 4096
queries in batches of 128, m = 32 negatives, skip = 0, 1-4 random exclusions per query (depth K = 36).
HIP-event times of
  * the unfiltered FlatIPIndex.search_batches at depth K,
  * FlatIPIndex.search_filtered_batches_iter (the same search + kernels.topk_exclude per batch),
  * the topk_exclude launch alone on one batch's [128, K] lists,
  * FlatIPIndex.pair_scores over one positive per query,
alternated --reps times on one build; the filtered results are checked against a torch restatement of the
compaction on the unfiltered lists.  Writes JSON (also printed) to --out.
usage: python tools/mine_probe.py [--n 10000000] [--reps 3] [--out profiles/r08_mining/mine_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--qb", type=int, default=128)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r08_mining", "mine_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import gen_shard
    from denseretrievaltoolkits_amd import kernels
    from denseretrievaltoolkits_amd.search import FlatIPIndex, filtered_depth
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    dev = torch.device("cuda", 0)
    p, _, _ = gen_shard(a.n, 1, 0, 768, dev)
    idx = FlatIPIndex.from_rows(p)
    g = torch.Generator(device=dev).manual_seed(5678)
    q = torch.randn((a.queries, 768), generator=g, device=dev).to(torch.bfloat16)
    batches = [q[o: o + a.qb] for o in range(0, a.queries, a.qb)]
    rng = np.random.default_rng(9)
    lists = [rng.integers(0, a.n, size=int(rng.integers(1, 5))).tolist() for _ in range(a.queries)]
    excl, off = build_exclusions(lists, dev)
    K = filtered_depth(a.m, 0, off, idx.ntotal)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def plain():
        return idx.search_batches(batches, K)

    def filtered():
        return list(idx.search_filtered_batches_iter(batches, a.m, excl, off))

    plain()   # warm-up: allocator, row statistics, group reservation
    filtered()
    t_plain, t_filt, res, raw = [], [], None, None
    for _ in range(a.reps):
        t, raw = timed(plain)
        t_plain.append(t)
        t, res = timed(filtered)
        t_filt.append(t)

    # the filter launch alone, on one batch's lists
    s0, i0 = raw[0]
    reps = 200
    t_kernel, _ = timed(lambda: [kernels.topk_exclude(s0, i0, excl, off[: a.qb + 1], a.m) for _ in range(reps)])

    # one positive per query: here each query's own best row
    qidx = torch.arange(a.queries, dtype=torch.int32, device=dev)
    pos = torch.cat([r[1][:, 0] for r in raw])
    idx.pair_scores(q, qidx, pos)
    t_pair, ps = timed(lambda: idx.pair_scores(q, qidx, pos))
    top1 = torch.cat([r[0][:, 0] for r in raw])

    # restatement of the compaction on the unfiltered depth-K lists
    ok = True
    o = 0
    off_h = off.cpu().tolist()
    for (rs, ri), (fs, fi, fc) in zip(raw, res):
        for j in range(rs.shape[0]):
            seg = excl[off_h[o + j]: off_h[o + j + 1]]
            keep = ~torch.isin(ri[j], seg) & (ri[j] >= 0)
            ok &= bool(torch.equal(ri[j][keep][: a.m], fi[j])) and int(fc[j]) == int(keep.sum())
        o += rs.shape[0]

    # what crossing depth 2048 costs: the grouped path's last depth against the large-k path's first
    # (per batch and synchronous there), on one full group of 16 batches
    cross = {"batches": min(16, len(batches))}
    for depth in (kernels.MAX_K, kernels.MAX_K + 1):
        idx.search_batches(batches[:16], depth)
        cross[f"depth_{depth}_ms_per_batch"] = round(min(timed(lambda: idx.search_batches(batches[:16], depth))[0]
                                                         for _ in range(2)) / cross["batches"], 3)

    nb = len(batches)
    out = {
        "crossing_2048": cross,
        "workload": f"{a.n} x 768 bf16 corpus, {a.queries} queries in batches of {a.qb}, m = {a.m}, skip = 0, "
                    f"1-4 random exclusions per query, depth K = {K}",
        "n": a.n, "queries": a.queries, "query_batch": a.qb, "m": a.m, "depth": K, "reps": a.reps,
        "unfiltered_ms": [round(t, 3) for t in t_plain],
        "filtered_ms": [round(t, 3) for t in t_filt],
        "unfiltered_ms_per_batch": round(min(t_plain) / nb, 4),
        "filtered_ms_per_batch": round(min(t_filt) / nb, 4),
        "filter_share_of_search": round(min(t_filt) / min(t_plain) - 1.0, 5),
        "topk_exclude_us_per_launch": round(t_kernel / reps * 1e3, 2),
        "topk_exclude_bytes_per_launch": a.qb * K * 12,
        "pair_scores_ms": round(t_pair, 4), "pairs": a.queries,
        "pair_scores_within_one_ulp_of_search": bool(((ps.double() - top1.double()).abs()
                                                      <= torch.from_numpy(np.spacing(top1.abs().cpu().numpy())).to(dev)).all()),
        "filtered_equals_restatement": ok,
        "queries_per_s_unfiltered": round(a.queries / min(t_plain) * 1e3, 1),
        "queries_per_s_filtered": round(a.queries / min(t_filt) * 1e3, 1),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the grouped (document-level, MaxP) search costs on top of the row search it rides on.  HIP-event times of
  * the topk_collapse launch alone on [128, k_in] lists at k_in = 2048 (table in LDS), 2049 (the same work with
    the table in the workspace) and 32768, groups of 8 rows,
  * the plain row search of 128 queries at depths 2048 and 32768 over the bench's 10M x 768 corpus,
  * FlatIPIndex.search_grouped_device at k = 100 with groups of 8 consecutive rows (depth 800) beside the plain
    search at that depth, for one batch of 128 queries and for 16 batches through the iterators,
all in one process; the grouped result is checked against a torch restatement of the collapse on the plain
depth-800 lists.  Writes JSON (also printed) to --out.
usage: python tools/collapse_probe.py [--n 10000000] [--out profiles/collapse01/collapse_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--qb", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--group-size", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "collapse01", "collapse_probe.json"))
    a = ap.parse_args()
    import torch
    from bench import gen_shard
    from denseretrievaltoolkits_amd import kernels
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    dev = torch.device("cuda", 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    g = torch.Generator(device=dev).manual_seed(5678)

    # the launch alone: descending scores, distinct random row ids, groups of 8 consecutive rows
    alone = {}
    for k_in in (kernels.COLLAPSE_LDS_K, kernels.COLLAPSE_LDS_K + 1, kernels.MAX_K_LARGE):
        n_rows = 4 * k_in
        ids = torch.stack([torch.randperm(n_rows, generator=g, device=dev)[:k_in] for _ in range(a.qb)])
        scores = torch.sort(torch.randn((a.qb, k_in), generator=g, device=dev), dim=1, descending=True)[0]
        grp = (torch.arange(n_rows, device=dev) // a.group_size).to(torch.int32)
        launches = 200 if k_in <= 4096 else 50
        kernels.topk_collapse(scores, ids, grp, a.k)
        t = min(timed(lambda: [kernels.topk_collapse(scores, ids, grp, a.k) for _ in range(launches)])[0]
                for _ in range(a.reps))
        cnt = kernels.topk_collapse(scores, ids, grp, a.k)[3]
        alone[str(k_in)] = {"us_per_launch": round(t / launches * 1e3, 2), "launches": launches,
                            "table": "lds" if k_in <= kernels.COLLAPSE_LDS_K else "workspace",
                            "bytes_read": a.qb * k_in * 16, "mean_groups_shown": round(float(cnt.float().mean()), 1)}

    p, _, _ = gen_shard(a.n, 1, 0, 768, dev)
    idx = FlatIPIndex.from_rows(p)
    idx.set_groups(torch.arange(a.n, device=dev) // a.group_size)
    nb = 16
    q = torch.randn((nb * a.qb, 768), generator=g, device=dev).to(torch.bfloat16)
    batches = [q[o: o + a.qb] for o in range(0, nb * a.qb, a.qb)]
    d1, d2 = kernels.grouped_depths(a.k, idx._p_max, idx.ntotal)

    # the row search one batch at the depths the launch was timed at
    rows = {}
    for depth in (kernels.MAX_K, kernels.MAX_K_LARGE):
        idx.search_device(batches[0], depth)
        rows[str(depth)] = round(min(timed(lambda: idx.search_device(batches[0], depth))[0] for _ in range(a.reps)), 3)

    # grouped against plain at the grouped search's own depth
    idx.search_device(batches[0], d1)
    idx.search_grouped_device(batches[0], a.k)
    list(idx.search_batches_iter(batches, d1))
    list(idx.search_grouped_batches_iter(batches, a.k))
    t_p1, t_g1, t_pn, t_gn, raw, res = [], [], [], [], None, None
    for _ in range(a.reps):
        t_p1.append(timed(lambda: idx.search_device(batches[0], d1))[0])
        t_g1.append(timed(lambda: idx.search_grouped_device(batches[0], a.k))[0])
        t, raw = timed(lambda: list(idx.search_batches_iter(batches, d1)))
        t_pn.append(t)
        t, res = timed(lambda: list(idx.search_grouped_batches_iter(batches, a.k)))
        t_gn.append(t)

    # restatement of the collapse on the plain depth-d1 lists: a row is kept iff no earlier row shares its group
    ok = True
    for (rs, ri), (gs, gg, gi, gc) in zip(raw, res):
        grp = ri // a.group_size
        first = torch.ones_like(ri, dtype=torch.bool)
        o = torch.argsort(grp, dim=1, stable=True)
        sg = torch.gather(grp, 1, o)
        dup = torch.zeros_like(first)
        dup[:, 1:] = sg[:, 1:] == sg[:, :-1]
        first.scatter_(1, o, ~dup)
        for j in range(ri.shape[0]):
            keep = first[j] & (ri[j] >= 0)
            ok &= bool(torch.equal(ri[j][keep][: a.k], gi[j])) and bool(torch.equal(rs[j][keep][: a.k], gs[j]))
            ok &= bool(torch.equal(grp[j][keep][: a.k].to(torch.int32), gg[j])) and int(gc[j]) == int(keep.sum())

    us_lds = alone[str(kernels.COLLAPSE_LDS_K)]["us_per_launch"]
    us_big = alone[str(kernels.MAX_K_LARGE)]["us_per_launch"]
    out = {
        "workload": f"{a.n} x 768 bf16 corpus, batches of {a.qb} queries, k = {a.k} groups, groups of "
                    f"{a.group_size} consecutive rows, depth plan {d1}, {d2}",
        "n": a.n, "query_batch": a.qb, "k": a.k, "group_size": a.group_size, "depth": d1, "reps": a.reps,
        "collapse_alone": alone,
        "row_search_ms_one_batch": rows,
        "collapse_share_of_row_search_2048": round(us_lds / 1e3 / rows[str(kernels.MAX_K)], 5),
        "collapse_share_of_row_search_32768": round(us_big / 1e3 / rows[str(kernels.MAX_K_LARGE)], 5),
        "plain_ms_one_batch": [round(t, 3) for t in t_p1],
        "grouped_ms_one_batch": [round(t, 3) for t in t_g1],
        "plain_ms_16_batches": [round(t, 3) for t in t_pn],
        "grouped_ms_16_batches": [round(t, 3) for t in t_gn],
        "grouped_over_plain_one_batch": round(min(t_g1) / min(t_p1), 4),
        "grouped_over_plain_16_batches": round(min(t_gn) / min(t_pn), 4),
        "grouped_equals_restatement": ok,
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

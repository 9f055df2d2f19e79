"""Per-launch-shape durations of the filter scan from a rocprofv3 kernel trace (csv): every
ip_scan32r_kernel launch grouped by its grid (the launch shape), in issue order, with the per-shape
average -- the figure bench.py's roofline.per_shape reports from HIP events.  With --passes P the
launches are also grouped by their pass index within a group (issue order modulo P: a one-GPU group
is P interleaved passes, the first against the sample threshold, the others against the tightened
one), and the group's other launches -- the final select, the threshold-tightening launch -- are
averaged beside them.
usage: python tools/scan_shape_stats.py <run_kernel_trace.csv> <out.json> [--passes P] [--last N]"""
import csv
import json
import sys


def _avg(v):
    return round(sum(v) / len(v), 1) if v else None


def main(path, out, passes=0, last=0):
    allrows = list(csv.DictReader(open(path)))
    rows = [r for r in allrows if "ip_scan32r_kernel" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    gk = [k for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Grid_Size") if k in (rows[0] if rows else {})]
    shapes = {}
    seq = []
    for r in rows:
        g = "x".join(r[k] for k in gk)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        shapes.setdefault(g, []).append(us)
        seq.append([g, round(us, 1)])
    res = {"kernel": "ip_scan32r_kernel<768>", "launches": len(rows), "grid_fields": gk,
           "per_grid": {g: {"launches": len(v), "avg_us": round(sum(v) / len(v), 1),
                            "last8_avg_us": round(sum(v[-8:]) / len(v[-8:]), 1)} for g, v in shapes.items()},
           "sequence": seq}
    if passes > 1:
        us = [s[1] for s in seq]
        if last:   # the timed steps' launches only (the warm-up's come first)
            us = us[-last:]
        by_pass = [[u for j, u in enumerate(us) if j % passes == p] for p in range(passes)]
        later = [u for p in range(1, passes) for u in by_pass[p]]
        res["per_pass"] = {"passes": passes, "launches_used": len(us), "avg_us": [_avg(v) for v in by_pass],
                           "pass0_avg_us": _avg(by_pass[0]), "later_passes_avg_us": _avg(later)}
        other = {}
        for name in ("select_kernel<0, 0>", "tighten_kernel"):
            v = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                 for r in allrows if name in r.get("Kernel_Name", "")]
            other[name] = {"launches": len(v), "avg_us": _avg(v)}
        res["group_other"] = other
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("per_grid", "per_pass", "group_other") if k in res}))


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {"--passes": 0, "--last": 0}
    for name in list(opt):
        if name in args:
            j = args.index(name)
            opt[name] = int(args[j + 1])
            del args[j: j + 2]
    main(args[0], args[1], opt["--passes"], opt["--last"])

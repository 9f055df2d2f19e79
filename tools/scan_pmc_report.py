#!/usr/bin/env python3
"""Summarise a counters-only rocprofv3 --pmc run of tools/scan_group_pmc.py: the ip_scan32r_kernel
dispatches' counters (mean per dispatch), the share of wave-cycles spent waiting (SQ_WAIT_ANY /
SQ_WAVE_CYCLES: waves parked at s_waitcnt or s_barrier), issuing (SQ_ACTIVE_INST_ANY / SQ_WAVE_CYCLES)
and the effective clock GRBM_GUI_ACTIVE / 8 XCDs / launch wall time (the dispatches' own timestamps in the
csv; without them the time scan_group_pmc.py printed, HIP events around its timed launches, passed as --ms).
usage: python tools/scan_pmc_report.py <dir of the run> <out.json> --ms <ms per launch>"""
import csv
import glob
import json
import os
import sys


def main(d, out, ms):
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    per = {}
    dur = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            if "ip_scan32r_kernel" not in r.get("Kernel_Name", ""):
                continue
            if r.get("Start_Timestamp") and r.get("End_Timestamp"):
                dur[r["Dispatch_Id"]] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
            per.setdefault(r["Counter_Name"], {}).setdefault(r["Dispatch_Id"], 0.0)
            per[r["Counter_Name"]][r["Dispatch_Id"]] += float(r["Counter_Value"])
    if dur and ms <= 0:   # the run's own dispatch timestamps, where the csv carries them
        ms = sum(dur.values()) / len(dur)
    mean = {c: sum(v.values()) / len(v) for c, v in per.items()}
    res = {"dispatches": {c: len(v) for c, v in per.items()}, "mean_per_dispatch": mean, "ms_per_launch": ms}
    if dur:
        res["dispatch_ms_from_csv"] = round(sum(dur.values()) / len(dur), 4)
    wc = mean.get("SQ_WAVE_CYCLES")
    if wc:
        for c in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
            if c in mean:
                res[c + "_per_wave_cycle"] = round(mean[c] / wc, 4)
    if "SQ_VALU_MFMA_BUSY_CYCLES" in mean and "GRBM_GUI_ACTIVE" in mean:
        res["mfma_busy_per_gui_active"] = round(mean["SQ_VALU_MFMA_BUSY_CYCLES"] / mean["GRBM_GUI_ACTIVE"], 4)
    # the dispatches' own durations where the csv carries them (the HIP-event time of a counter run also
    # holds the profiler's work between the launches)
    wall = res.get("dispatch_ms_from_csv", ms)
    if "GRBM_GUI_ACTIVE" in mean and wall > 0:
        res["effective_clock_mhz"] = round(mean["GRBM_GUI_ACTIVE"] / 8 / (wall * 1e-3) / 1e6, 1)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    a = sys.argv[1:]
    ms = 0.0
    if "--ms" in a:
        j = a.index("--ms")
        ms = float(a[j + 1])
        del a[j: j + 2]
    main(a[0], a[1], ms)

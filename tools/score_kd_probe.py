#!/usr/bin/env python3
"""Probe: the distillation loss (score_kd, w_ce = w_kd = 1) next to score_ce at the shapes of the bench leg
train_scores (batch 512, d 768, n = 2 / 8), timed as bench_legs.run_train_scores times it: forward + backward,
eager (host clock around a synchronised window) and replayed from a captured graph (device time).  The two ops
alternate in one process: one discarded round, then --rounds measured ones; each op's own min..max over the rounds
is its spread in this session.  One JSON line per (n, round) and a summary line per n.
usage: python tools/score_kd_probe.py [--rounds 4] [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from denseretrievaltoolkits_amd.score_ce import score_ce, score_kd  # noqa: E402


def eager_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def capture(fn, dev, warmup):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def graph_ms(graph, replays):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replays * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--dim", type=int, default=768)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds: at least 3 measured rounds")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    for n in (2, 8):
        q = torch.randn((a.batch, a.dim), generator=g, device=dev).requires_grad_(True)
        p = torch.randn((a.batch * n, a.dim), generator=g, device=dev).requires_grad_(True)
        teacher = torch.randn((a.batch, n), generator=g, device=dev) * 3.0

        def ce():
            loss, _ = score_ce(q, p, n, 1.0)
            loss.backward()

        def kd():
            loss, _ = score_kd(q, p, teacher, n, temperature=2.0, w_ce=1.0, w_kd=1.0)
            loss.backward()

        ops = (("ce", ce), ("kd", kd))
        graphs = {name: capture(fn, dev, a.warmup) for name, fn in ops}
        rows = []
        for r in range(a.rounds + 1):          # round 0 is discarded
            row = {"n": n, "round": r}
            for name, fn in ops:
                row[name + "_ms"] = round(eager_ms(fn, a.steps, a.warmup), 4)
            for name, _ in ops:
                row[name + "_graph_ms"] = round(graph_ms(graphs[name], a.steps * 5), 4)
            if r == 0:
                row["discarded"] = True
            else:
                rows.append(row)
            print(json.dumps(row), flush=True)
        summ = {"n": n, "summary": True, "rounds": len(rows)}
        for key in ("ce_ms", "kd_ms", "ce_graph_ms", "kd_graph_ms"):
            v = sorted(row[key] for row in rows)
            summ[key] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
        print(json.dumps(summ), flush=True)
        del graphs


if __name__ == "__main__":
    main()

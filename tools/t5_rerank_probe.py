#!/usr/bin/env python
"""Pair-scoring throughput of HipT5PairScorer against its own encoder and against HF
T5ForConditionalGeneration in torch bf16 on the same GPU, and the cross-attention pool kernel alone.

t5-base in its relu form (12 + 12 layers x 768, d_ff 3072, 12 heads; HF's seeded random init, nothing
is downloaded), batches of 256 and 512 pairs x 160 tokens with prefix masks of 80..160 tokens.  Three
arms alternate within one process (a discarded first round, then `--rounds` rounds of `--iters`
forwards per arm, a device synchronise inside every timed window):

    a  HipT5PairScorer.logits          (encoder + one decoder step + the two-row logit head)
    b  HipT5Encoder alone              (the decoder step's share is (a - b) / b in time)
    c  HF T5ForConditionalGeneration   (torch bf16, decoder_input_ids = 0, logits[:, 0, tokens])

Then drt_t5_cross_pool_bf16 alone under HIP events at B = 32, 256, 512 (bytes/s = B L D 2 over the
kernel's time), and one profiled pass of arm a on a single stream for each kernel's share.  Prints one
JSON line per round and summary lines.

    python tools/t5_rerank_probe.py [--rounds 5] [--iters 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

TOKENS = (6136, 1176)      # any two rows of lm_head: (neg, pos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--seq", type=int, default=160)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--only-scorer", type=int, default=0, metavar="N",
                    help="run arm a N times at the first batch size and exit (the run to put under a kernel trace)")
    args = ap.parse_args()

    import torch
    from transformers import T5Config, T5ForConditionalGeneration
    from denseretrievaltoolkits_amd import _native
    from denseretrievaltoolkits_amd.model.t5_decoder import HipT5PairScorer

    if not torch.cuda.is_available():
        raise SystemExit("t5_rerank_probe: no GPU visible (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(obj):
        s = obj if isinstance(obj, str) else json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    cfg = T5Config(vocab_size=32128, d_model=768, d_kv=64, d_ff=3072, num_layers=12, num_decoder_layers=12,
                   num_heads=12, feed_forward_proj="relu", dropout_rate=0.0, decoder_start_token_id=0)
    model = T5ForConditionalGeneration(cfg).eval()
    scorer = HipT5PairScorer.from_hf(model, dev)
    hf = model.to(dev).to(torch.bfloat16)
    L, D, H = args.seq, cfg.d_model, cfg.num_heads

    def med(x):
        return sorted(x)[len(x) // 2]

    def make_batch(B):
        g = torch.Generator().manual_seed(B)
        lens = torch.randint(L // 2, L + 1, (B,), generator=g)
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
        ids = (torch.randint(1, cfg.vocab_size, (B, L), generator=g) * mask).to(dev)
        return ids, mask.to(dev)

    if args.only_scorer:
        ids, mask = make_batch(args.batches[0])
        for _ in range(args.only_scorer):
            scorer.logits(ids, mask, TOKENS)
        torch.cuda.synchronize()
        return

    for B in args.batches:
        ids, mask = make_batch(B)
        start = torch.zeros((B, 1), dtype=torch.long, device=dev)

        def run_a():
            return scorer.logits(ids, mask, TOKENS)

        def run_b():
            return scorer.encoder(ids, mask)

        def run_c():
            with torch.no_grad():
                out = hf(input_ids=ids, attention_mask=mask, decoder_input_ids=start)
                return out.logits[:, 0, list(TOKENS)]

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.iters

        arms = (("a_scorer", run_a), ("b_encoder", run_b), ("c_hf_bf16", run_c))
        for _, fn in arms:       # warm-up: code objects, allocator, library heuristics
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        diff = (run_a().float() - run_c().float()).abs()
        emit({"check": "scorer vs hf-bf16 logits", "batch": B, "max_abs_diff": float(diff.max()),
              "logits_rms": float(run_c().float().pow(2).mean().sqrt())})
        ms = {name: [] for name, _ in arms}
        for r in range(-1, args.rounds):       # round -1 is discarded
            row = {}
            for name, fn in arms:
                row[name] = timed(fn) * 1e3
            if r < 0:
                continue
            for name in row:
                ms[name].append(row[name])
            emit({"batch": B, "round": r, **{k + "_ms": round(v, 3) for k, v in row.items()},
                  "a_beats_c": row["a_scorer"] < row["c_hf_bf16"]})
        a, b, c = (med(ms[n]) for n, _ in arms)
        emit({"model": "t5-base relu 12+12 x 768", "batch": B, "seq": L, "iters": args.iters, "rounds": args.rounds,
              "a_scorer_ms": round(a, 3), "b_encoder_ms": round(b, 3), "c_hf_bf16_ms": round(c, 3),
              "a_pairs_per_s": round(B / a * 1e3, 1), "c_pairs_per_s": round(B / c * 1e3, 1),
              "decoder_share_of_encoder": round((a - b) / b, 4), "speedup_vs_hf": round(c / a, 3),
              "a_beats_c_every_round": all(x < y for x, y in zip(ms["a_scorer"], ms["c_hf_bf16"]))})

    # the pool kernel alone under HIP events: back-to-back launches that rotate over K copies of enc,
    # K * bytes >= 640 MB (well past the 256 MB Infinity Cache), so every launch reads enc from HBM
    lib = _native.load()
    for B in (32, 256, 512):
        nbytes = B * L * D * 2
        K = -(-640_000_000 // nbytes)
        torch.manual_seed(7 * B)
        enc = torch.randn(K * B, L, D, device=dev).to(torch.bfloat16)
        qt = (torch.randn(B, H, D, device=dev) * (4.0 / D ** 0.5)).to(torch.bfloat16)
        lens = torch.randint(L // 2, L + 1, (B,), device=dev)
        mask = (torch.arange(L, device=dev)[None, :] < lens[:, None]).to(torch.int64)
        out = torch.empty((B, H, D), dtype=torch.bfloat16, device=dev)
        st = _native.stream_ptr(dev)

        def sweep():
            for i in range(K):
                _native.check(lib.drt_t5_cross_pool_bf16(qt.data_ptr(), enc[i * B:].data_ptr(), mask.data_ptr(),
                                                         out.data_ptr(), B, L, H, D, st), "drt_t5_cross_pool_bf16")

        sweep()
        passes = 3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            sweep()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (passes * K)
        emit({"kernel": "t5_cross_pool", "batch": B, "seq": L, "heads": H, "d_model": D, "launches": passes * K,
              "us_per_launch": round(us, 2), "enc_bytes": nbytes, "enc_TB_per_s": round(nbytes / us / 1e6, 3)})

    # per-kernel shares of arm a, in a pass of their own (tracing slows the host) and on one stream
    from torch.profiler import ProfilerActivity, profile
    scorer.encoder.split_streams = False
    B = args.batches[0]
    ids, mask = make_batch(B)
    scorer.logits(ids, mask, TOKENS)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        scorer.logits(ids, mask, TOKENS)
        torch.cuda.synchronize()
    rows = [(e.key, e.device_time_total, e.count) for e in prof.key_averages() if e.device_time_total > 0]
    total = sum(t for _, t, _ in rows)
    emit(f"arm a, one call at batch {B} on one stream: {total / 1e3:.2f} ms of kernel time in "
         f"{sum(c for _, _, c in rows)} launches")
    for name, t, c in sorted(rows, key=lambda x: -x[1]):
        emit(f"  {100.0 * t / total:5.1f} %  {t / 1e3:8.3f} ms  x{c:<4d} {name[:110]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

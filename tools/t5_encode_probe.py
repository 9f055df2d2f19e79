#!/usr/bin/env python
"""Encode throughput of HipT5Encoder against HF T5EncoderModel in torch bf16 on the same GPU.

t5-base in its relu form (12 x 768, d_ff 3072, 12 heads; HF's seeded random init, nothing is
downloaded), batches of 512 passages x 128 tokens with prefix masks of 64..128 tokens.  The two
sides alternate within one process (rounds of `--iters` forwards each, a device synchronise inside
every timed window, both warmed up first); then one profiled pass of the HIP side, on a single
stream, gives each kernel's share of its GPU time.  Prints one JSON line per round, a summary line, and the shares.

    python tools/t5_encode_probe.py [--rounds 5] [--iters 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()

    import torch
    from transformers import T5Config, T5EncoderModel
    from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder

    if not torch.cuda.is_available():
        raise SystemExit("t5_encode_probe: no GPU visible (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(obj):
        s = obj if isinstance(obj, str) else json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    cfg = T5Config(vocab_size=32128, d_model=768, d_kv=64, d_ff=3072, num_layers=12, num_heads=12,
                   feed_forward_proj="relu", dropout_rate=0.0)
    model = T5EncoderModel(cfg).eval()
    enc = HipT5Encoder.from_hf(model, dev)
    hf = model.to(dev).to(torch.bfloat16)
    B, L = args.batch, args.seq
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
    ids = (torch.randint(1, cfg.vocab_size, (B, L), generator=g) * mask).to(dev)
    mask = mask.to(dev)

    def run_hip():
        return enc(ids, mask)

    def run_hf():
        with torch.no_grad():
            return hf(input_ids=ids, attention_mask=mask).last_hidden_state

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return B * args.iters / (time.perf_counter() - t0)

    for fn in (run_hip, run_hf):       # warm-up: code objects, allocator, library heuristics
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    a, b = run_hip().float(), run_hf().float()
    valid = mask.bool()
    cos = torch.nn.functional.cosine_similarity(a[valid], b[valid], dim=-1)
    emit({"check": "hip vs hf-bf16 per-token cosine", "min": float(cos.min()), "mean": float(cos.mean())})

    rates = {"hip": [], "hf_bf16": []}
    for r in range(args.rounds):
        rates["hip"].append(timed(run_hip))
        rates["hf_bf16"].append(timed(run_hf))
        emit({"round": r, "hip_passages_per_s": round(rates["hip"][-1], 1),
              "hf_bf16_passages_per_s": round(rates["hf_bf16"][-1], 1)})

    def med(x):
        return sorted(x)[len(x) // 2]

    emit({"model": "t5-base relu 12x768", "batch": B, "seq": L, "iters": args.iters, "rounds": args.rounds,
          "hip_passages_per_s": round(med(rates["hip"]), 1), "hip_min_max": [round(min(rates["hip"]), 1),
                                                                             round(max(rates["hip"]), 1)],
          "hf_bf16_passages_per_s": round(med(rates["hf_bf16"]), 1),
          "hf_min_max": [round(min(rates["hf_bf16"]), 1), round(max(rates["hf_bf16"]), 1)],
          "speedup": round(med(rates["hip"]) / med(rates["hf_bf16"]), 3)})

    # per-kernel shares of the HIP side, in a pass of their own (tracing slows the host) and on one
    # stream (the two halves' kernels share the chip, which stretches every kernel's own duration)
    from torch.profiler import ProfilerActivity, profile
    enc.split_streams = False
    run_hip()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run_hip()
        torch.cuda.synchronize()
    rows = [(e.key, e.device_time_total, e.count) for e in prof.key_averages() if e.device_time_total > 0]
    total = sum(t for _, t, _ in rows)
    emit(f"HIP side, one forward on one stream: {total / 1e3:.2f} ms of kernel time in {sum(c for _, _, c in rows)} launches")
    for name, t, c in sorted(rows, key=lambda x: -x[1]):
        emit(f"  {100.0 * t / total:5.1f} %  {t / 1e3:8.3f} ms  x{c:<4d} {name[:110]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

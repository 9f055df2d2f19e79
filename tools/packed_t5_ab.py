"""Padded vs padding-free T5-base encode (HipT5Encoder.forward vs forward_packed), alternating windows.

Per shape (B x L, lengths drawn uniformly from a range) each variant encodes and pools the same batch in
windows of at least one second, one variant after the other, three rounds, so a drift of the machine
shows inside every variant's figures rather than between variants:

  padded           enc(ids, mask) + pool                                  (the yardstick: unchanged code)
  packed           plan_packing + forward_packed + pool_packed + unpack   (what DRModel.encode runs with
                   hip_packed_t5, the encoder's defaults: one attention launch per batch)
  packed_classes   the same with one attention launch per length class

The reranker shape (128 pairs padded to 512) times what RRModel changes under hip_packed_t5: the encoder
pass and the unpack; the one-step decoder behind it is the same code on both sides.

--padded-only --pkg-root DIR times the padded variant alone against the package found under DIR: the
same yardstick on another build (the parent commit's).  --profile runs each variant of one shape a few
times and exits: the process to put under a kernel trace.

12-layer T5-base shapes with seeded random weights (d_model 768, 12 heads; relu d_ff 3072 and
gated-gelu d_ff 2048); one JSON record.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

SHAPES = [
    ("512x128_len32-128", 512, 128, 32, 128),
    ("2048x32_len6-20", 2048, 32, 6, 20),
    ("256x160_len60-160", 256, 160, 60, 160),
    ("rerank_128x512_len120-512", 128, 512, 120, 512),
]
TOWERS = [("relu", 3072), ("gated-gelu", 2048)]


def _window(fn, seconds):
    """ms per call over a window of at least `seconds` (the call count from one timed warm-up call)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    steps = max(3, math.ceil(seconds / max(time.perf_counter() - t0, 1e-5)))
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "packed_t5_01", "packed_t5_ab.json"))
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--padded-only", action="store_true")
    ap.add_argument("--profile", default=None, help="shape name: run its variants three times each and exit")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg_root)
    from transformers import T5Config, T5EncoderModel
    from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder
    if not args.padded_only:
        from denseretrievaltoolkits_amd.model.packing import plan_packing
    if not torch.cuda.is_available():
        raise SystemExit("packed_t5_ab: no GPU visible (timings are GPU-only)")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/packed_t5_ab.py", "seconds": args.seconds, "rounds": args.rounds,
           "pkg_root": os.path.relpath(args.pkg_root), "device": torch.cuda.get_device_name(0), "towers": {}}
    for act, d_ff in TOWERS:
        torch.manual_seed(0)
        m = T5EncoderModel(T5Config(vocab_size=32128, d_model=768, d_kv=64, d_ff=d_ff, num_layers=12, num_heads=12,
                                    feed_forward_proj=act, dropout_rate=0.0)).eval()
        enc = HipT5Encoder.from_hf(m, dev)
        del m
        shapes = rec["towers"][act] = {}
        for name, B, L, lo, hi in SHAPES:
            if args.profile and name != args.profile:
                continue
            g = torch.Generator().manual_seed(B * 1000 + L)
            lens = torch.randint(lo, hi + 1, (B,), generator=g)
            mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64).to(dev)
            ids = torch.randint(1, 32128, (B, L), generator=g).to(dev) * mask
            T = int(lens.sum())
            out = {"B": B, "L": L, "T": T, "padding_share": round(1.0 - T / (B * L), 4)}

            def padded():
                return enc.pool(enc(ids, mask), mask, "mean")

            def packed(classes=False):
                def run():
                    enc.packed_classes = classes
                    plan = plan_packing(mask, L)
                    h = enc.forward_packed(ids, plan)
                    reps = enc.pool_packed(h, plan, L, "mean")
                    enc.unpack(h, plan, L)
                    return reps
                return run

            variants = {"padded": padded}
            if not args.padded_only:
                variants.update(packed=packed(), packed_classes=packed(True))
                out["max_abs_diff_reps_packed_vs_padded"] = float((variants["packed"]()[0] - padded()[0]).abs().max())
                out["attention_launches_with_classes"] = len(plan_packing(mask, L).classes())
            if args.profile:
                for fn in variants.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                continue
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    times[k].append(_window(fn, args.seconds))
            out["ms"] = times
            out["padded_spread"] = round(max(times["padded"]) / min(times["padded"]) - 1.0, 4)
            if not args.padded_only:
                for k in ("packed", "packed_classes"):
                    out[k + "_over_padded"] = round(min(times[k]) / min(times["padded"]), 4)
            shapes[name] = out
            print(act, name, json.dumps(out), flush=True)
        del enc
    if args.profile:
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

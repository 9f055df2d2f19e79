#!/usr/bin/env python3
"""A/B of one T5 encoder training step (forward + backward of sum(hidden * R)) on one GPU:

    hip   the HIP T5 training tower (model/t5_train_tower.train_hidden_t5)
    hf    the HF T5EncoderModel under torch bf16 autocast

on the same weights and batch, for T5-base (768 / 12 layers / 12 heads / 3072 relu) and a gated
1024-wide shape (1024 / 12 / 16 / 2816 gated-gelu), B x L = 128 x 128, dropout_rate 0.1 in train
mode.  The legs alternate in pairs (hip, hf, hip, hf, ...), each timed window = --steps steps between
device events after --warmup steps per leg; the medians over --pairs windows and their spread are
printed and written as JSON lines.

    python tools/t5_train_ab.py --out profiles/<session>/t5_train_ab.log
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "t5-base": dict(d_model=768, num_layers=12, num_heads=12, d_ff=3072, feed_forward_proj="relu"),
    "gated-1024": dict(d_model=1024, num_layers=12, num_heads=16, d_ff=2816, feed_forward_proj="gated-gelu"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="t5-base,gated-1024")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--layers", type=int, default=0, help="override the number of layers (0: the shape's)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from transformers import T5Config, T5EncoderModel
    from denseretrievaltoolkits_amd.model.t5_train_tower import train_hidden_t5
    if not torch.cuda.is_available():
        raise SystemExit("t5_train_ab: no GPU visible (timings are GPU-only)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for name in args.shapes.split(","):
        kw = dict(SHAPES[name])
        if args.layers:
            kw["num_layers"] = args.layers
        cfg = T5Config(vocab_size=32128, d_kv=64, dropout_rate=args.dropout, pad_token_id=0, **kw)
        torch.manual_seed(0)
        model = T5EncoderModel(cfg).to(dev).train()
        B, L = args.batch, args.seq
        g = torch.Generator(device=dev).manual_seed(1)
        ids = torch.randint(1, cfg.vocab_size, (B, L), generator=g, device=dev)
        lens = torch.randint(L // 2, L + 1, (B,), generator=g, device=dev)
        mask = (torch.arange(L, device=dev)[None, :] < lens[:, None]).to(torch.int64)
        R = torch.randn(B, L, cfg.d_model, generator=g, device=dev)

        def step_hip():
            model.zero_grad(set_to_none=True)
            (train_hidden_t5(model, ids, mask) * R).sum().backward()

        def step_hf():
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                h = model(input_ids=ids, attention_mask=mask).last_hidden_state
            (h.float() * R).sum().backward()

        legs = {"hip": step_hip, "hf": step_hf}
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.pairs):
            for k, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) / args.steps)
        rec = {"shape": name, "config": kw, "B": B, "L": L, "dropout": args.dropout, "steps": args.steps,
               "pairs": args.pairs}
        for k, v in times.items():
            rec[f"{k}_ms_median"] = round(statistics.median(v), 3)
            rec[f"{k}_ms_min"] = round(min(v), 3)
            rec[f"{k}_ms_max"] = round(max(v), 3)
        rec["hf_over_hip"] = round(rec["hf_ms_median"] / rec["hip_ms_median"], 3)
        emit(rec)
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

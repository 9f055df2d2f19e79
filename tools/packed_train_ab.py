"""Padded vs padding-free BERT-base TRAINING tower (train_hidden without / with a PackingPlan),
alternating.

Per shape (B x L, lengths drawn uniformly from a range) each variant runs forward + backward of one
tower on the same batch with the default dropout (0.1 / 0.1); the variants are timed one after the
other, three rounds each, so a drift of the machine shows up inside every variant's figures rather
than between variants:

  padded               train_hidden(ids, mask)                       (the yardstick: unchanged code)
  packed_one_launch    plan_packing + train_hidden(plan=...), one attention launch per batch
  packed_classes       the same with one attention launch per length class of the plan
  padded_plus_plan     the padded tower after a plan_packing call whose result is dropped: what the plan's
                       device-to-host copy (it drains the launch queue once per step) costs by itself
  packed_ready_plan    the packed tower with a plan built outside the timed loop (a mask that is still on
                       the CPU, as a collator leaves it, is planned without that copy)

The control shape has no padding and the plan forced: what packing costs when it saves nothing.
The attention backward of one layer is also timed alone on the shape's packed tensors in both launch
policies, against the padded kernel on the padded tensors.

--padded-only --pkg-root DIR times the padded variant alone against the package found under DIR:
the same yardstick on another build (the parent commit's).

12-layer BERT-base with seeded random weights; one JSON record.
"""
import argparse
import json
import os
import sys
import time

import torch

SHAPES = [
    ("512x128_len32-128", 512, 128, 32, 128),
    ("2048x32_len6-20", 2048, 32, 6, 20),
    ("256x160_len60-160", 256, 160, 60, 160),
    ("512x128_full_control", 512, 128, 128, 128),
]


def _time(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "packed_train01", "packed_train_ab.json"))
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--padded-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg_root)
    from transformers import BertConfig, BertModel
    from denseretrievaltoolkits_amd import _native
    from denseretrievaltoolkits_amd.model import encoder_bwd, train_tower
    if not args.padded_only:
        from denseretrievaltoolkits_amd.model.packing import plan_packing
    if not torch.cuda.is_available():
        raise SystemExit("packed_train_ab: no GPU visible (timings are GPU-only)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = BertModel(BertConfig(), add_pooling_layer=False).to(dev).train()
    lib = _native.load()
    rec = {"tool": "tools/packed_train_ab.py", "steps": args.steps, "rounds": args.rounds,
           "pkg_root": os.path.relpath(args.pkg_root), "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, B, L, lo, hi in SHAPES:
        g = torch.Generator().manual_seed(B * 1000 + L)
        lens = torch.randint(lo, hi + 1, (B,), generator=g)
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64).to(dev)
        ids = torch.randint(1000, 30522, (B, L), generator=g).to(dev)
        T = int(lens.sum())
        out = {"B": B, "L": L, "T": T, "token_share": round(T / (B * L), 4)}
        R = torch.randn(B, L, 768, device=dev) * mask[:, :, None].float()

        def step(**kw):
            m.zero_grad(set_to_none=True)
            hid = train_tower.train_hidden(m, ids, mask, seed=1234, **kw)
            (hid * R).sum().backward()
            return hid

        variants = {"padded": step}
        if not args.padded_only:
            force = lo == L

            def packed(classes):
                def run():
                    keep = train_tower.packed_train_classes
                    train_tower.packed_train_classes = classes
                    try:
                        return step(plan=plan_packing(mask, L, force=force))
                    finally:
                        train_tower.packed_train_classes = keep
                return run

            ready = plan_packing(mask, L, force=force)

            def padded_plus_plan():     # the padded tower after the plan's device-to-host copy
                plan_packing(mask, L, force=force)
                return step()

            variants.update(packed_one_launch=packed(False), packed_classes=packed(True),
                            padded_plus_plan=padded_plus_plan, packed_ready_plan=lambda: step(plan=ready))
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(_time(fn, args.steps))
        out["ms"] = times
        best = {k: min(v) for k, v in times.items()}
        out["padded_spread"] = round(max(times["padded"]) / min(times["padded"]) - 1.0, 4)
        if not args.padded_only:
            out["packed_one_launch_over_padded"] = round(best["packed_one_launch"] / best["padded"], 4)
            out["packed_classes_over_padded"] = round(best["packed_classes"] / best["padded"], 4)
            out["padded_plus_plan_over_padded"] = round(best["padded_plus_plan"] / best["padded"], 4)
            out["packed_ready_plan_over_padded"] = round(best["packed_ready_plan"] / best["padded"], 4)
            # one layer's attention backward alone (p = 0.1, the forward's keep bits)
            plan = plan_packing(mask, L, force=force)
            H, heads = 768, 12
            qkv_p = torch.randn((B * L, 3 * H), device=dev).to(torch.bfloat16)
            dctx_p = torch.randn((B * L, H), device=dev).to(torch.bfloat16)
            sel = mask.bool().view(-1)
            qkv_t, dctx_t = qkv_p[sel].contiguous(), dctx_p[sel].contiguous()
            drop = (0.1, 1234, 1)
            ctx_p, lse_p, bits_p = encoder_bwd.attention_forward(qkv_p, mask, B, L, heads, 0.125, drop=drop)
            ctx_t, lse_t, bits_t = encoder_bwd.attention_varlen_forward(qkv_t, plan, heads, 0.125, drop=drop)

            def bwd_padded():
                encoder_bwd.attention_backward(qkv_p, ctx_p, dctx_p, lse_p, mask, bits_p, B, L, heads, 0.125, drop=drop,
                                               want_dbias=True)

            def bwd_varlen(classes):
                return lambda: encoder_bwd.attention_varlen_backward(qkv_t, ctx_t, dctx_t, lse_t, bits_t, plan, heads,
                                                                      0.125, drop=drop, per_class=classes)

            def fwd_varlen(classes):
                return lambda: encoder_bwd.attention_varlen_forward(qkv_t, plan, heads, 0.125, drop=drop,
                                                                     per_class=classes)

            attn = {"bwd_padded": bwd_padded, "bwd_varlen_one_launch": bwd_varlen(False),
                    "bwd_varlen_classes": bwd_varlen(True),
                    "fwd_padded": lambda: encoder_bwd.attention_forward(qkv_p, mask, B, L, heads, 0.125, drop=drop),
                    "fwd_varlen_one_launch": fwd_varlen(False), "fwd_varlen_classes": fwd_varlen(True)}
            at = {k: [] for k in attn}
            for _ in range(args.rounds):
                for k, fn in attn.items():
                    at[k].append(_time(fn, 100, warmup=10))
            out["attention_ms"] = at
            out["attention_launches_with_classes"] = len(plan.classes())
            del qkv_p, dctx_p, qkv_t, dctx_t, ctx_p, lse_p, bits_p, ctx_t, lse_t, bits_t
        rec["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

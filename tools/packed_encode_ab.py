"""Padded vs padding-free BERT-base encode (HipBertEncoder.forward vs forward_packed), alternating.

Per shape (B x L, lengths drawn uniformly from a range) each variant encodes and pools the same
batch; the variants are timed one after the other, three rounds each, so a drift of the machine
shows up inside every variant's three figures rather than between variants:

  padded            enc(ids, mask) + pool                              (the yardstick: unchanged code)
  packed            plan_packing + forward_packed + pool_packed + unpack  (what DRModel.encode runs,
                    with the encoder's defaults)
  packed_classes / packed_one_launch    one attention launch per length class / one for the batch
  packed_two_streams / packed_one_stream   with / without the two-stream split
                    (each of the four differs from the defaults in that one switch at most)

The control shape has no padding and the plan forced: what packing costs when it saves nothing.
The attention launches of one layer are also timed alone on the shape's packed QKV, with and
without length classes, against the padded kernel on the padded QKV.  (The form with several
<= 32-token sequences per work-group is not built, so it is not timed.)

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


def _time(fn, steps, warmup=3):
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "packed01", "packed_encode_ab.json"))
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--padded-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg_root)
    from transformers import BertConfig, BertModel
    from denseretrievaltoolkits_amd import _native
    from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder
    if not args.padded_only:
        from denseretrievaltoolkits_amd.model.packing import plan_packing
    if not torch.cuda.is_available():
        raise SystemExit("packed_encode_ab: no GPU visible (timings are GPU-only)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = BertModel(BertConfig(), add_pooling_layer=False).eval()
    enc = HipBertEncoder.from_hf(m, dev)
    del m
    lib = enc.lib
    rec = {"tool": "tools/packed_encode_ab.py", "steps": args.steps, "rounds": args.rounds,
           "pkg_root": os.path.relpath(args.pkg_root), "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, B, L, lo, hi in SHAPES:
        g = torch.Generator().manual_seed(B * 1000 + L)
        lens = torch.randint(lo, hi + 1, (B,), generator=g)
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64).to(dev)
        ids = torch.randint(1000, 30522, (B, L), generator=g).to(dev)
        T = int(lens.sum())
        out = {"B": B, "L": L, "T": T, "token_share": round(T / (B * L), 4)}

        def padded():
            return enc.pool(enc(ids, mask), mask, "first")

        def padded_one_stream():
            enc.split_streams = False
            try:
                return padded()
            finally:
                enc.split_streams = True

        variants = {"padded": padded}
        if not args.padded_only:
            variants["padded_one_stream"] = padded_one_stream
            force = lo == L

            def packed():
                plan = plan_packing(mask, L, force=force)
                h = enc.forward_packed(ids, plan)
                reps = enc.pool_packed(h, plan, L, "first")
                enc.unpack(h, plan, L)
                return reps

            def with_flags(classes, split):
                def run():
                    keep = enc.packed_classes, enc.packed_split_streams
                    enc.packed_classes, enc.packed_split_streams = classes, split
                    try:
                        return packed()
                    finally:
                        enc.packed_classes, enc.packed_split_streams = keep
                return run

            variants.update(packed=packed, packed_classes=with_flags(True, enc.packed_split_streams),
                            packed_one_launch=with_flags(False, enc.packed_split_streams),
                            packed_two_streams=with_flags(enc.packed_classes, True),
                            packed_one_stream=with_flags(enc.packed_classes, False))
            diff = (variants["packed"]()[0] - padded()[0]).abs().max()
            out["max_abs_diff_reps_packed_vs_padded"] = float(diff)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(_time(fn, args.steps))
        out["ms"] = times
        if not args.padded_only:
            best = {k: min(v) for k, v in times.items()}
            out["packed_over_padded"] = round(best["packed"] / best["padded"], 4)
            out["padded_spread"] = round(max(times["padded"]) / min(times["padded"]) - 1.0, 4)
            # what the packed variant adds around the layer loop, each alone: the plan (mask
            # reduction + the one device-to-host copy, which also drains the launch queue), the
            # unpack copy, and the forward + pooling with a ready plan
            plan = plan_packing(mask, L, force=force)
            hid = enc.forward_packed(ids, plan)
            parts = {"plan_packing": lambda: plan_packing(mask, L, force=force),
                     "unpack": lambda: enc.unpack(hid, plan, L),
                     "forward_pool_ready_plan": lambda: enc.pool_packed(enc.forward_packed(ids, plan), plan, L, "first")}
            pt = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    pt[k].append(_time(fn, args.steps))
            out["parts_ms"] = pt
            # one layer's attention alone
            H, heads = enc.shape.hidden, enc.shape.heads
            qkv_p = torch.randn((B * L, 3 * H), device=dev).to(torch.bfloat16)
            qkv_t = qkv_p.view(B, L, 3 * H)[mask.bool()].contiguous()
            ctx_p = torch.empty((B * L, H), dtype=torch.bfloat16, device=dev)
            ctx_t = torch.empty((T, H), dtype=torch.bfloat16, device=dev)
            cu = plan.cu_seqlens.data_ptr()

            def attn_padded():
                s = _native.stream_ptr(dev)
                _native.check(lib.drt_attention_forward_bf16(qkv_p.data_ptr(), mask.data_ptr(), None, ctx_p.data_ptr(), None,
                                                             None, B, L, heads, 64, 0.125, 0.0, 0, 0, s), "attention")

            def attn_varlen(launches):
                def run():
                    s = _native.stream_ptr(dev)
                    for sp, n, ml in launches:
                        _native.check(lib.drt_attention_varlen_forward_bf16(
                            qkv_t.data_ptr(), cu, sp.data_ptr() if sp is not None else None, n, ml, ctx_t.data_ptr(),
                            heads, 64, 0.125, s), "varlen attention")
                return run

            attn = {"padded": attn_padded, "varlen_classes": attn_varlen(plan.classes()),
                    "varlen_one_launch": attn_varlen([(None, B, plan.max_len)])}
            at = {k: [] for k in attn}
            for _ in range(args.rounds):
                for k, fn in attn.items():
                    at[k].append(_time(fn, 200, warmup=10))
            out["attention_ms"] = at
            out["attention_launches_with_classes"] = len(plan.classes())
        rec["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

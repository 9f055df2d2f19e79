"""Attention forward A/B, one library per process (DRT_LIB=<variant>): drt_attention_forward_bf16 at the encode
leg's half batch (256 x 128 x 12 heads; all-ones and ragged masks), the query tower's (128 x 32) and a
ragged 64 x 100 -- HIP-event us per launch and an output digest -- then the encode leg (passages/s)."""
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _us(run, reps):
    """Median of 5 HIP-event timings of `reps` launches, us per launch."""
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000 / reps)
    return round(sorted(ts)[2], 2)


def both_widths(reps=2000):
    """ATTN_SHAPES=widths: both attention forwards, all-ones masks, 12 heads -- head_dim 64 at 512 x 128 and
    64 x 512, head_dim 32 at 512 x 128, 256 x 160 and 64 x 512, the padded training forward with dropout, lse and
    keep words at 1024 x 128 -- then the 12-layer tower encode at 512 x 128 for hidden 768 and 384 (ms per batch)."""
    from transformers import BertConfig, BertModel
    from denseretrievaltoolkits_amd import _native
    from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder
    lib = _native.load()
    dev = torch.device("cuda", 0)
    st = _native.stream_ptr(dev)
    heads = 12
    res = {"lib": os.path.basename(os.path.dirname(os.environ["DRT_LIB"])) if "DRT_LIB" in os.environ else "change"}
    g = torch.Generator(device=dev).manual_seed(1)
    for dh, B, L, drop in ((64, 512, 128, 0.0), (64, 64, 512, 0.0), (32, 512, 128, 0.0), (32, 256, 160, 0.0),
                           (32, 64, 512, 0.0), (64, 1024, 128, 0.1)):
        H = heads * dh
        qkv = (torch.randn((B * L, 3 * H), generator=g, device=dev) * 2).to(torch.bfloat16)
        mask = torch.ones((B, L), dtype=torch.int64, device=dev)
        ctx = torch.empty((B * L, H), dtype=torch.bfloat16, device=dev)
        sc = 1.0 / math.sqrt(dh)
        if dh == 32:
            run = lambda: _native.check(lib.drt_attention_hd32_forward_bf16(qkv.data_ptr(), mask.data_ptr(), ctx.data_ptr(),
                                                                            B, L, heads, sc, st), "attn32")
        else:
            lse = torch.empty((B, heads, L), dtype=torch.float32, device=dev) if drop else None
            bits = torch.empty((B, heads, L, (L + 31) // 32), dtype=torch.int32, device=dev) if drop else None
            run = lambda: _native.check(lib.drt_attention_forward_bf16(
                qkv.data_ptr(), mask.data_ptr(), None, ctx.data_ptr(), lse.data_ptr() if drop else None,
                bits.data_ptr() if drop else None, B, L, heads, dh, sc, drop, 7, 3, st), "attn")
        res[f"hd{dh}_{B}x{L}{'_drop' if drop else ''}_us"] = _us(run, reps)
    B, L = 512, 128
    ids = torch.randint(1000, 30522, (B, L), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    mask = torch.ones((B, L), dtype=torch.int64, device=dev)
    for hidden, inter in ((768, 3072), (384, 1536)):
        torch.manual_seed(0)
        m = BertModel(BertConfig(hidden_size=hidden, intermediate_size=inter), add_pooling_layer=False).eval()
        enc = HipBertEncoder.from_hf(m, dev)
        del m
        res[f"encode_h{hidden}_512x128_ms"] = round(_us(lambda: enc.pool(enc(ids, mask), mask, "first"), 30) / 1000, 4)
    print(json.dumps(res), flush=True)


def main(reps=50):
    if os.environ.get("ATTN_SHAPES") == "widths":
        return both_widths()
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    dev = torch.device("cuda", 0)
    st = _native.stream_ptr(dev)
    heads, dh = 12, 64
    H = heads * dh
    res = {"lib": os.path.basename(os.environ.get("DRT_LIB", "product"))}
    g = torch.Generator(device=dev).manual_seed(1)
    shapes = ((256, 128, False), (256, 128, True), (128, 32, False), (64, 100, True))
    if os.environ.get("ATTN_SHAPES") == "rerank":
        shapes = ((500, 160, False), (625, 128, False), (500, 160, True))
    for (B, L, ragged) in shapes:
        qkv = (torch.randn((B * L, 3 * H), generator=g, device=dev) * 2).to(torch.bfloat16)
        mask = torch.ones((B, L), dtype=torch.int64, device=dev)
        if ragged:
            lens = torch.randint(L // 4, L + 1, (B,), generator=g, device=dev)
            mask = (torch.arange(L, device=dev)[None, :] < lens[:, None]).to(torch.int64)
        ctx = torch.empty((B * L, H), dtype=torch.bfloat16, device=dev)
        run = lambda: _native.check(lib.drt_attention_forward_bf16(qkv.data_ptr(), mask.data_ptr(), None, ctx.data_ptr(),
                                                                   None, None, B, L, heads, dh, 1.0 / math.sqrt(dh),
                                                                   0.0, 0, 0, st), "attn")
        run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1000 / reps)
        nbytes = B * L * 4 * H * 2
        t = sorted(ts)[2]
        res[f"B{B}_L{L}{'_ragged' if ragged else ''}"] = {
            "us": round(t, 2), "hbm_frac": round(nbytes / (t * 1e-6) / 8e12, 3),
            "digest": int(ctx.view(torch.int16).reshape(-1).double().mul(
                torch.arange(ctx.numel(), device=dev, dtype=torch.float64).remainder(997)).sum().item())}
    from transformers import BertConfig, BertModel
    from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder
    torch.manual_seed(0)
    m = BertModel(BertConfig(), add_pooling_layer=False).eval()
    enc = HipBertEncoder.from_hf(m, dev)
    del m
    B, L = 512, 128
    ids = torch.randint(1000, 30522, (B, L), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    mask = torch.ones((B, L), dtype=torch.int64, device=dev)
    enc(ids, mask)
    torch.cuda.synchronize()
    pps = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(8):
            enc.pool(enc(ids, mask), mask, "first")
        torch.cuda.synchronize()
        pps.append(round(8 * B / (time.perf_counter() - t0), 1))
    res["encode_pps"] = pps
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

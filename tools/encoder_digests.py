#!/usr/bin/env python3
"""sha256 digests of the encoder paths' outputs for one source tree, to show that a host-side change
leaves every bit alone: padded / packed / two-stream BERT forward, pooling, unpack, the training tower's
output and parameter gradients (padded and packed), and the T5 encoder, on tiny seeded models.

Run it once per tree, each in a fresh process, and compare the two files, e.g. against the parent commit:
    git archive HEAD~1 | tar -x -C /tmp/parent && (cd /tmp/parent && python -m denseretrievaltoolkits_amd.build_native)
    python tools/encoder_digests.py /tmp/parent parent.txt && python tools/encoder_digests.py . this.txt
    paste -d' ' parent.txt this.txt; diff parent.txt this.txt
usage: python tools/encoder_digests.py <tree root> <out file>"""
import hashlib
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch  # noqa: E402
from transformers import BertConfig, BertModel, T5Config, T5EncoderModel  # noqa: E402

import denseretrievaltoolkits_amd  # noqa: E402
from denseretrievaltoolkits_amd.model.encoder import HipBertEncoder  # noqa: E402
from denseretrievaltoolkits_amd.model.packing import plan_packing  # noqa: E402
from denseretrievaltoolkits_amd.model.t5_encoder import HipT5Encoder  # noqa: E402
from denseretrievaltoolkits_amd.model.train_tower import train_hidden  # noqa: E402

assert os.path.abspath(denseretrievaltoolkits_amd.__file__).startswith(root + os.sep), denseretrievaltoolkits_amd.__file__
dev = torch.device("cuda", 0)
lines = []


def dig(name, t):
    t = t.detach().contiguous().cpu()
    assert torch.isfinite(t.float()).all(), name
    h = hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
    lines.append(f"{name} {tuple(t.shape)} {h}")
    print(lines[-1], flush=True)


def batch(B, L, lens, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, 1000, (B, L), generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)
    return ids.to(dev), mask.to(dev)


torch.manual_seed(1)
cfg = BertConfig(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                 max_position_embeddings=512)
model = BertModel(cfg, add_pooling_layer=False).to(dev).eval()
enc = HipBertEncoder.from_hf(model, dev)

for B, L, lens in ((4, 40, [40, 7, 33, 1]), (3, 160, [160, 129, 5]), (2, 200, [200, 61])):
    ids, mask = batch(B, L, lens, 10 + B)
    dig(f"forward[{B},{L}]", enc(ids, mask))

lens, L = [5, 1, 32, 17, 40], 40
ids, mask = batch(5, L, lens, 20)
for classes in (False, True):
    enc.packed_classes = classes
    plan = plan_packing(mask, L, device=dev, min_saving=0.0)
    hid = enc.forward_packed(ids, plan)
    dig(f"forward_packed classes={classes}", hid)
    for pooling in ("first", "mean", "max"):
        dig(f"pool_packed {pooling} classes={classes}", enc.pool_packed(hid, plan, L, pooling)[0])
    dig(f"unpack classes={classes}", enc.unpack(hid, plan, L))
enc.packed_classes = False

ids, mask = batch(4, 40, [40, 7, 33, 1], 14)
enc.split_min_tokens = 64
dig("forward[4,40] two streams", enc(ids, mask))
enc.split_min_tokens = 8192

lens, L = [5, 33, 160, 64], 160
ids, mask = batch(4, L, lens, 30)
model.train()
fixed = torch.randn((4, L, 256), generator=torch.Generator().manual_seed(31)).to(dev)
for packed in (False, True):
    plan = plan_packing(mask, L, device=dev, min_saving=0.0) if packed else None
    model.zero_grad(set_to_none=True)
    out = train_hidden(model, ids, mask, seed=1234, plan=plan)
    (out * fixed).sum().backward()
    tag = "packed" if packed else "padded"
    dig(f"train_hidden {tag} out", out)
    for n, p in model.named_parameters():
        dig(f"train_hidden {tag} grad {n}", p.grad)
model.eval()

torch.manual_seed(2)
t5 = T5EncoderModel(T5Config(vocab_size=1000, d_model=256, d_kv=64, d_ff=1024, num_layers=2, num_heads=4,
                             feed_forward_proj="relu")).to(dev).eval()
t5enc = HipT5Encoder.from_hf(t5, dev)
ids, mask = batch(4, 40, [40, 7, 33, 1], 40)
dig("t5 forward[4,40]", t5enc(ids, mask))
t5enc.split_min_tokens = 64
dig("t5 forward[4,40] two streams", t5enc(ids, mask))

torch.cuda.synchronize()
with open(sys.argv[2], "w") as f:
    f.write("\n".join(lines) + "\n")
print("DIGESTS DONE", len(lines))

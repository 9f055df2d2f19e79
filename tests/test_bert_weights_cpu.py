"""The weight snapshot shared by the inference encoder and the training tower (model/encoder.py
bert_weights), no GPU: on a random 1-layer, hidden-256 BertModel state dict every tensor equals what
the two loaders it replaced produced, restated here in plain torch -- fp32 embeddings, biases and
LayerNorm, bf16 linears, and Q | K | V concatenated in fp32 and rounded to bf16 once."""
import pytest
import torch

H, I, VOCAB, POS = 256, 1024, 50, 40
LAYER = "encoder.layer.0."
LINEARS = {"wo": "attention.output.dense", "wi": "intermediate.dense", "wf": "output.dense"}
VECTORS = {"bo": "attention.output.dense.bias", "g1": "attention.output.LayerNorm.weight",
           "b1": "attention.output.LayerNorm.bias", "bi": "intermediate.dense.bias", "bf": "output.dense.bias",
           "g2": "output.LayerNorm.weight", "b2": "output.LayerNorm.bias"}
EMB = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
       "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias")


def _state(prefix=""):
    g = torch.Generator().manual_seed(7)
    shapes = {EMB[0]: (VOCAB, H), EMB[1]: (POS, H), EMB[2]: (2, H), EMB[3]: (H,), EMB[4]: (H,)}
    for n in ("query", "key", "value"):
        shapes[LAYER + f"attention.self.{n}.weight"] = (H, H)
        shapes[LAYER + f"attention.self.{n}.bias"] = (H,)
    shapes[LAYER + "attention.output.dense.weight"] = (H, H)
    shapes[LAYER + "intermediate.dense.weight"] = (I, H)
    shapes[LAYER + "output.dense.weight"] = (H, I)
    for name in VECTORS.values():
        shapes[LAYER + name] = (I,) if name.startswith("intermediate") else (H,)
    # parameters, as the training tower's named_parameters() hands them over
    return {prefix + k: torch.nn.Parameter(torch.randn(s, generator=g)) for k, s in shapes.items()}


@pytest.mark.parametrize("prefix", ["", "lm_q."])
def test_snapshot_equals_the_loaders_it_replaced(prefix):
    from denseretrievaltoolkits_amd.model.encoder import bert_weights
    sd = _state(prefix)
    emb, layers = bert_weights(sd, torch.device("cpu"), 1, prefix)
    assert len(emb) == 5 and len(layers) == 1
    for got, name in zip(emb, EMB):
        assert got.dtype == torch.float32 and not got.requires_grad and torch.equal(got, sd[prefix + name].detach())
    ly = layers[0]
    assert sorted(ly) == sorted(["wqkv", "bqkv", *LINEARS, *VECTORS])
    qkv = [prefix + LAYER + f"attention.self.{n}." for n in ("query", "key", "value")]
    wqkv = torch.cat([sd[p + "weight"].detach().float() for p in qkv], 0).to(torch.bfloat16)
    bqkv = torch.cat([sd[p + "bias"].detach().float() for p in qkv], 0)
    assert ly["wqkv"].dtype == torch.bfloat16 and ly["wqkv"].shape == (3 * H, H) and torch.equal(ly["wqkv"], wqkv)
    assert ly["bqkv"].dtype == torch.float32 and torch.equal(ly["bqkv"], bqkv)
    for key, name in LINEARS.items():
        want = sd[prefix + LAYER + name + ".weight"].detach().to(torch.bfloat16)
        assert ly[key].dtype == torch.bfloat16 and ly[key].is_contiguous() and torch.equal(ly[key], want)
    for key, name in VECTORS.items():
        assert ly[key].dtype == torch.float32 and torch.equal(ly[key], sd[prefix + LAYER + name].detach())
    assert not any(t.requires_grad for t in ly.values())

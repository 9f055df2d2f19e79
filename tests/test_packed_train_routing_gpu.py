"""The one routing of the packed training tower's attention (PackingPlan.split()): which of the four
varlen training entries a batch calls, with what launch arguments, on both sides of the 160 / 161
boundary, and the result against the padded tower at the tolerances of
tests/test_packed_train_long_tower_gpu.py (tests/test_packed_train_tower_gpu.py _close_to_flag_off)."""
import pytest

import test_packed_train_tower_gpu as pt
import test_train_tower_gpu as tt
from oracle import bert_weights as bw

pytestmark = pytest.mark.gpu

B, L, LAYERS = 4, 192, 1
# 161 and 160: the two sides of the boundary; 161 tokens are 2 tiles of 128 rows
BATCHES = {"mixed": (161, 5, 160, 33), "short": (150, 5, 160, 33)}
SHORT_FWD, SHORT_BWD = pt.VARLEN_FWD, pt.VARLEN_BWD
LONG_FWD, LONG_BWD = "drt_attention_varlen_long_train_forward_bf16", "drt_attention_varlen_long_backward_bf16"
# position of (seq_ids or tiles, n, max_len) in the entry's arguments
LIST_AT = {SHORT_FWD: 2, LONG_FWD: 2, SHORT_BWD: 5, LONG_BWD: 5}

_padded = {}   # batch -> (ids, mask, R, loss, grads) of the padded tower, computed once


class _Recorder:
    """The (list given?, n, max_len) of every call of one native entry (the ctypes handle is shared)."""

    def __init__(self, monkeypatch, name):
        from denseretrievaltoolkits_amd import _native
        lib = _native.load()
        self.calls = []
        real, at = getattr(lib, name), LIST_AT[name]

        def recorded(*args):
            self.calls.append((args[at] is not None, args[at + 1], args[at + 2]))
            return real(*args)

        monkeypatch.setattr(lib, name, recorded)


def _run(m, ids_t, mask_t, R, **kw):
    from denseretrievaltoolkits_amd.model.train_tower import train_hidden
    hid = train_hidden(m, ids_t, mask_t, seed=77, **kw)
    loss = (hid * R).sum()
    loss.backward()
    return hid, loss.detach(), pt._grads(m)


def _padded_run(batch, dev):
    import torch
    if batch not in _padded:
        ids, mask = bw.token_batch(B, L, seed=L + B)
        mask[:] = 0
        for b, n in enumerate(BATCHES[batch]):
            mask[b, :n] = 1
        ids_t, mask_t = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        R = torch.randn(B, L, 768, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
        R = R * mask_t[:, :, None].float()
        _, loss, grads = _run(tt._bert(LAYERS, 29, dev).train(), ids_t, mask_t, R)
        _padded[batch] = (ids_t, mask_t, R, loss, grads)
    return _padded[batch]


# (batch, packed_train_classes) -> the calls of one layer, forward and backward alike unless stated
EXPECT = {
    ("mixed", False): dict(long_fwd=[(True, 1, 161)], short=[(True, 3, 160)]),
    ("mixed", True): dict(long_fwd=[(True, 1, 161)], short=[(True, 1, 160), (True, 1, 33), (True, 1, 5)]),
    ("short", False): dict(long_fwd=[], short=[(False, 4, 160)]),
}


@pytest.mark.parametrize("batch,classes", list(EXPECT), ids=[f"{b}-{'per-class' if c else 'one-launch'}" for b, c in EXPECT])
def test_routing_and_result_against_the_padded_tower(dev, monkeypatch, batch, classes):
    from denseretrievaltoolkits_amd.model import train_tower
    from denseretrievaltoolkits_amd.model.packing import plan_packing
    ids_t, mask_t, R, loss_padded, grads_padded = _padded_run(batch, dev)
    plan = plan_packing(mask_t, L, force=True)
    monkeypatch.setattr(train_tower, "packed_train_classes", classes)
    spies = {name: _Recorder(monkeypatch, name) for name in LIST_AT}
    hid, loss, grads = _run(tt._bert(LAYERS, 29, dev).train(), ids_t, mask_t, R, plan=plan, packed_long=True)
    want = EXPECT[batch, classes]
    assert spies[LONG_FWD].calls == want["long_fwd"] * LAYERS
    assert spies[SHORT_FWD].calls == want["short"] * LAYERS
    assert spies[SHORT_BWD].calls == want["short"] * LAYERS
    # the streamed backward is one launch pair over the tile table whatever the launch policy is
    n_tiles = sum(-(-n // 128) for n in BATCHES[batch] if n > 160)
    assert spies[LONG_BWD].calls == ([(True, n_tiles, plan.max_len)] if n_tiles else []) * LAYERS
    assert n_tiles == (2 if batch == "mixed" else 0)
    assert (hid[~mask_t.bool()] == 0).all()
    pt._close_to_flag_off(loss, loss_padded, grads, grads_padded)

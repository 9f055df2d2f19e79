"""CPU: the distillation loss's C ABI (symbols, argument validation before any device call, workspace),
its torch operators (schema, fake kernels, no CPU fallback), pack_pairs against the tokenizer's own
pair encoding (the reference's RRCollator recipe), and the overlay entry of DRT.trainer.distill."""
import ctypes
import sys

import pytest
import torch

SYMBOLS = ["drt_kd_fwd", "drt_kd_bwd", "drt_score_kd_workspace", "drt_score_kd_fwd", "drt_score_kd_bwd"]


@pytest.fixture(scope="module")
def lib():
    from denseretrievaltoolkits_amd import _native
    return _native.load()


@pytest.fixture(scope="module")
def drt():
    from denseretrievaltoolkits_amd import ops
    return ops.load()


def test_symbols_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name


# (m, n, d, group, T, w_ce, w_kd) that must be refused; the good tuple is (4, 8, 64, 2, 1.0, 1.0, 1.0)
GOOD = (4, 8, 64, 2, 1.0, 1.0, 1.0)
BAD = {
    "group 0": (4, 8, 64, 0, 1.0, 1.0, 1.0),
    "group negative": (4, 8, 64, -1, 1.0, 1.0, 1.0),
    "m * group > n": (4, 7, 64, 2, 1.0, 1.0, 1.0),
    "m * group > n (large group)": (2, 8, 64, 5, 1.0, 1.0, 1.0),
    "T = 0": (4, 8, 64, 2, 0.0, 1.0, 1.0),
    "T < 0": (4, 8, 64, 2, -1.0, 1.0, 1.0),
    "T = inf": (4, 8, 64, 2, float("inf"), 1.0, 1.0),
    "T = nan": (4, 8, 64, 2, float("nan"), 1.0, 1.0),
    "w_ce < 0": (4, 8, 64, 2, 1.0, -0.5, 1.0),
    "w_kd < 0": (4, 8, 64, 2, 1.0, 1.0, -0.5),
    "w_kd nan": (4, 8, 64, 2, 1.0, 1.0, float("nan")),
    "m = 0": (0, 8, 64, 2, 1.0, 1.0, 1.0),
    "d = 0": (4, 8, 0, 2, 1.0, 1.0, 1.0),
}


def _calls(lib, args, ptr, null_at=None, ws_bytes=None):
    """The two fused entries with every pointer `ptr` (a host address: a call that passes validation would
    only fail in HIP, never dereference it here) except the null_at-th, which is NULL."""
    m, n, d, g, T, wce, wkd = args
    need = lib.drt_score_kd_workspace(max(m, 1), max(n, 1), max(d, 1)) if ws_bytes is None else ws_bytes

    def P(count):
        return [None if null_at == i else ptr for i in range(count)]
    q, p, t, S, lse, aux, loss, ws = P(8)
    # null_at = 8 is the backward's workspace: the forward would get eight non-null pointers, pass validation
    # and, where there is a GPU, launch its kernels on `ptr`, a host address -- so it is not called then
    fwd = None if null_at == 8 else lib.drt_score_kd_fwd(q, p, t, m, n, d, g, T, wce, wkd, 1.0, S, lse, aux, loss, ws,
                                                         need, None)
    q, p, t, S, lse, aux, dq, dp = P(8)
    ws = ptr if null_at != 8 else None
    bwd = lib.drt_score_kd_bwd(q, p, t, S, lse, aux, m, n, d, g, T, wce, wkd, None, 1.0, dq, dp, ws, need, None)
    return fwd, bwd


def test_invalid_arguments_rejected_without_gpu(lib):
    from denseretrievaltoolkits_amd import _native
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    for why, args in BAD.items():
        assert _calls(lib, args, ptr) == (_native.DRT_EINVAL, _native.DRT_EINVAL), why
    for k in range(9):   # each pointer in turn NULL (the backward's upstream gradient may be NULL)
        fwd, bwd = _calls(lib, GOOD, ptr, null_at=k)
        if k < 8:
            assert fwd == _native.DRT_EINVAL, k
        assert bwd == _native.DRT_EINVAL, k
    need = lib.drt_score_kd_workspace(*GOOD[:3])
    assert need > 0
    assert _calls(lib, GOOD, ptr, ws_bytes=need - 1) == (_native.DRT_EINVAL, _native.DRT_EINVAL)
    # the unfused pair validates the same way
    for why, (m, n, d, g, T, wce, wkd) in BAD.items():
        if why == "d = 0":
            continue
        assert lib.drt_kd_fwd(ptr, ptr, m, n, g, T, wce, wkd, 1.0, ptr, ptr, ptr, ptr, None) == _native.DRT_EINVAL, why
        assert lib.drt_kd_bwd(ptr, ptr, ptr, ptr, m, n, g, T, wce, wkd, None, 1.0, ptr, None) == _native.DRT_EINVAL, why
    m, n, d, g, T, wce, wkd = GOOD
    assert lib.drt_kd_fwd(None, ptr, m, n, g, T, wce, wkd, 1.0, ptr, ptr, ptr, ptr, None) == _native.DRT_EINVAL
    assert lib.drt_kd_bwd(ptr, None, ptr, ptr, m, n, g, T, wce, wkd, None, 1.0, ptr, None) == _native.DRT_EINVAL


def test_workspace_covers_score_ce(lib):
    for m, n, d in [(8, 16, 64), (37, 111, 100), (32, 64, 32), (96, 224, 160), (512, 1024, 768), (512, 4096, 768),
                    (2, 600, 32)]:
        assert lib.drt_score_kd_workspace(m, n, d) >= lib.drt_score_ce_workspace(m, n, d) > 0
    assert lib.drt_score_kd_workspace(0, 16, 64) == 0


def test_ops_registered(drt):
    for name in ("score_kd_fwd", "score_kd_bwd"):
        assert getattr(torch.ops.drt, name).default._schema.name == f"drt::{name}"
    args = [a.name for a in torch.ops.drt.score_kd_fwd.default._schema.arguments]
    assert args == ["q", "p", "teacher", "group", "temperature", "w_ce", "w_kd", "scale"]
    assert len(torch.ops.drt.score_kd_fwd.default._schema.returns) == 4


def test_fake_kernels(drt):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q = torch.empty(8, 96, device="cuda", requires_grad=True)
        p = torch.empty(24, 96, device="cuda", requires_grad=True)
        t = torch.empty(8, 3, device="cuda")
        loss, S, lse, aux = drt.score_kd_fwd(q, p, t, 3, 2.0, 0.5, 1.0, 1.0)
        assert loss.shape == () and S.shape == (8, 24) and lse.shape == (8,) and aux.shape == (8, 2)
        assert {x.dtype for x in (loss, S, lse, aux)} == {torch.float32}
        assert loss.requires_grad and not S.requires_grad and not aux.requires_grad
        dq, dp = drt.score_kd_bwd(torch.empty((), device="cuda"), q, p, t, S, lse, aux, 3, 2.0, 0.5, 1.0, 1.0)
        assert dq.shape == (8, 96) and dp.shape == (24, 96) and dq.dtype == dp.dtype == torch.float32


def test_cpu_tensors_refused(drt):
    from denseretrievaltoolkits_amd.score_ce import score_kd
    q, p, t = torch.zeros(4, 32), torch.zeros(8, 32), torch.zeros(4, 2)
    with pytest.raises((NotImplementedError, RuntimeError)):
        drt.score_kd_fwd(q, p, t, 2, 1.0, 0.0, 1.0, 1.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        drt.score_kd_bwd(torch.ones(()), q, p, t, torch.zeros(4, 8), torch.zeros(4), torch.zeros(4, 2), 2, 1.0, 0.0,
                         1.0, 1.0)
    with pytest.raises(ValueError):
        score_kd(q, p, t, 2)


VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(40)]


@pytest.mark.parametrize("n", [1, 3])
def test_pack_pairs_matches_tokenizer(tmp_path, n):
    from transformers import BertTokenizerFast

    from denseretrievaltoolkits_amd.trainer.distill import pack_pairs
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(VOCAB) + "\n")
    tok = BertTokenizerFast(str(vocab), do_lower_case=False)
    Lq, Lp = 8, 12
    g = torch.Generator().manual_seed(n)

    def raw(maxlen):
        return torch.randint(5, len(VOCAB), (int(torch.randint(1, maxlen + 1, (1,), generator=g)),),
                             generator=g).tolist()
    # raw token lists of at most L - 2 tokens: an empty query, a full one, an empty passage, a full one
    queries = [[], raw(Lq - 2), torch.arange(5, 5 + Lq - 2).tolist(), raw(Lq - 2)]
    passages = [raw(Lp - 2) for _ in range(len(queries) * n)]
    passages[0] = []
    passages[-1] = torch.arange(10, 10 + Lp - 2).tolist()
    if n > 1:
        passages[n + 1] = []

    def encode(first, second, L):
        """One example as RRCollator.create_one_example builds it: prepare_for_model on the raw token ids
        (truncation="only_first", max_length, no padding).  Tokenizers of transformers 5.x no longer have that
        method; there the same tokenizer's backend applies the same truncation and its own single / pair
        template to the same tokens (an empty member stays a member: [CLS] q [SEP] [SEP])."""
        if hasattr(tok, "prepare_for_model"):
            return tok.prepare_for_model(first, second, truncation="only_first", max_length=L, padding=False,
                                         return_attention_mask=False, return_token_type_ids=False)
        bt = tok.backend_tokenizer
        bt.enable_truncation(max_length=L, strategy="only_first")
        a, b = (None if x is None else bt.encode([VOCAB[t] for t in x], is_pretokenized=True,
                                                  add_special_tokens=False) for x in (first, second))
        assert a.ids == list(first) and (b is None or b.ids == list(second))
        return {"input_ids": bt.post_process(a, b).ids}

    def collate(lists, L):   # the bi-encoder's own batch: [CLS] x [SEP], right-padded to L
        return dict(tok.pad([encode(x, None, L) for x in lists], padding="max_length", max_length=L,
                            return_tensors="pt"))

    got = pack_pairs(collate(queries, Lq), collate(passages, Lp), n, tok.pad_token_id)
    pairs = [encode(queries[i // n], passages[i], Lq + Lp) for i in range(len(passages))]
    want = tok.pad(pairs, padding="max_length", max_length=Lq + Lp, return_tensors="pt")
    assert want["input_ids"].shape == (len(passages), Lq + Lp)
    cls, sep = tok.cls_token_id, tok.sep_token_id
    assert want["input_ids"][0].tolist()[:3] == [cls, sep, sep]   # empty query, empty passage
    assert set(got) == {"input_ids", "attention_mask"}
    assert got["input_ids"].shape == (len(passages), Lq + Lp)
    assert torch.equal(got["input_ids"], want["input_ids"])
    assert torch.equal(got["attention_mask"], want["attention_mask"])


def test_pack_pairs_rejects_mismatched_batches():
    from denseretrievaltoolkits_amd.trainer.distill import pack_pairs
    q = {"input_ids": torch.zeros(2, 4, dtype=torch.long), "attention_mask": torch.ones(2, 4, dtype=torch.long)}
    p = {"input_ids": torch.zeros(5, 4, dtype=torch.long), "attention_mask": torch.ones(5, 4, dtype=torch.long)}
    with pytest.raises(ValueError):
        pack_pairs(q, p, 2, 0)


def test_overlay_serves_distill():
    from denseretrievaltoolkits_amd import drt_overlay
    saved = {k: v for k, v in sys.modules.items() if k == "DRT" or k.startswith("DRT.")}
    try:
        drt_overlay.install()
        import DRT.trainer.distill as d
        from denseretrievaltoolkits_amd.trainer import distill
        assert d is distill
        assert hasattr(d, "DistillTrainer") and hasattr(d, "pack_pairs") and hasattr(d, "teacher_scores")
        from DRT.trainer.losses import DistillContrastiveLoss  # noqa: F401
    finally:
        for k in [k for k in sys.modules if k == "DRT" or k.startswith("DRT.")]:
            del sys.modules[k]
        sys.modules.update(saved)

"""GPU: the fused score + CE + KL distillation loss (torch.ops.drt.score_kd_fwd / _bwd, score_ce.score_kd)
and what is built on it (DRModel.forward(teacher_scores=), trainer/distill.py).

    S = q p^T;  CE_i = lse_j S_ij - S[i, i g];  s_i = S[i, i g : i g + g] / T;  t_i = teacher_i / T
    loss = scale * mean_i (w_ce CE_i + w_kd KL(softmax t_i || softmax s_i))

The reference is torch fp64 autograd of a NaN-safe restatement (-inf teacher entries are masked before any
product; the naive `where` version has NaN gradients).  Inputs are N(0, 1) rows like the project's other loss
tests, teacher scores N(0, 9); tolerances are the project's own for this score path (test_golden_gpu.py,
test_torch_ops_gpu.py): scores rtol 1e-5 / atol 1e-4, loss rtol 1e-5, gradients rtol 1e-4 / atol 1e-6.  The same
closed form evaluated in fp32 on the host (scores rounded from fp64) stays within 0.32 of the gradient band on
these shapes; the kernels, whose scores carry their own fp32 rounding, measured 0.86 at worst on an MI355X.
"""
import functools
import math
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu

# (m, n, d, g): ragged 64 x 64 split-K path; one row, group = whole row; large-tile path (multiples of 32) with
# n > m g; g > 256 (strided group pass); the training shapes of the benchmark's train_scores leg
SHAPES = [(8, 16, 64, 2), (37, 111, 100, 3), (1, 5, 64, 5), (32, 64, 32, 2), (96, 224, 160, 2), (160, 320, 96, 2),
          (2, 600, 32, 300), (512, 1024, 768, 2), (512, 4096, 768, 8)]
TEMPS = [0.5, 1.0, 4.0]
W_CE, W_KD, SCALE, UPSTREAM = 0.7, 1.3, 1.5, 2.0


def _inputs(dev, m, n, d, g):
    import torch
    gen = torch.Generator(device=dev).manual_seed(m * 131 + n)
    q = torch.randn(m, d, generator=gen, device=dev)
    p = torch.randn(n, d, generator=gen, device=dev)
    t = torch.randn(m, g, generator=gen, device=dev) * 3.0
    if g > 1:
        t[0, g - 1] = -math.inf      # one passage dropped from the distillation
    if m > 2:
        t[2] = -math.inf             # one query dropped
    return q, p, t


def ref_fp64(q, p, t, g, T, w_ce, w_kd, scale):
    """(loss, S) in the dtype of q; -inf teacher entries are masked before they meet a product."""
    import torch
    m = q.shape[0]
    rows = torch.arange(m, device=q.device)
    idx = rows[:, None] * g + torch.arange(g, device=q.device)[None]
    S = q @ p.T
    ce = torch.logsumexp(S, 1) - S[rows, rows * g]
    s = S.gather(1, idx) / T
    keep = torch.isfinite(t)
    live = keep.any(1, keepdim=True)
    tt = torch.where(keep, t, torch.zeros_like(t)) / T
    lt = torch.logsumexp(torch.where(keep, tt, torch.full_like(tt, -1e300)), 1, keepdim=True)
    logpt = torch.where(keep & live, tt - torch.where(live, lt, torch.zeros_like(lt)), torch.zeros_like(tt))
    pt = torch.where(keep & live, logpt.exp(), torch.zeros_like(tt))
    kl = (pt * (logpt - torch.log_softmax(s, 1))).sum(1)
    return scale * (w_ce * ce + w_kd * kl).mean(), S


def _run_kd(q, p, t, g, T, w_ce, w_kd, scale=SCALE, upstream=UPSTREAM):
    from denseretrievaltoolkits_amd.score_ce import score_kd
    q, p = q.detach().clone().requires_grad_(True), p.detach().clone().requires_grad_(True)
    loss, S = score_kd(q, p, t, g, temperature=T, w_ce=w_ce, w_kd=w_kd, scale=scale)
    (upstream * loss).backward()
    return loss.detach(), S.detach(), q.grad, p.grad


@functools.lru_cache(maxsize=None)
def _case(dev, m, n, d, g, T):
    """One KD run and its fp64 reference per (shape, T), shared by the tests below (never modified)."""
    q, p, t = _inputs(dev, m, n, d, g)
    got = _run_kd(q, p, t, g, T, W_CE, W_KD)
    qd, pd = q.double().requires_grad_(True), p.double().requires_grad_(True)
    loss, S = ref_fp64(qd, pd, t.double(), g, T, W_CE, W_KD, SCALE)
    (UPSTREAM * loss).backward()
    return (q, p, t), got, (loss.detach(), S.detach(), qd.grad, pd.grad)


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("m,n,d,g", SHAPES)
def test_score_kd_against_fp64_autograd(dev, m, n, d, g, T):
    import torch
    _, (loss, S, dq, dp), (rl, rS, rdq, rdp) = _case(dev, m, n, d, g, T)
    for x in (loss, S, dq, dp):
        assert torch.isfinite(x).all()
    for name, got, want in (("dq", dq, rdq), ("dp", dp, rdp)):
        err = (got.double() - want).abs()
        print(f"{name}: worst |err| / band = {float((err / (1e-6 + 1e-4 * want.abs())).max()):.3f}")
    print(f"loss {loss.item():.8g} vs {rl.item():.8g}; scores worst / band = "
          f"{float(((S.double() - rS).abs() / (1e-4 + 1e-5 * rS.abs())).max()):.3f}")
    torch.testing.assert_close(S.double(), rS, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(loss.double(), rl, rtol=1e-5, atol=0.0)
    torch.testing.assert_close(dq.double(), rdq, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dp.double(), rdp, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("m,n,d,g", SHAPES)
def test_w_kd_zero_is_score_ce_bit_for_bit(dev, m, n, d, g):
    import torch
    from denseretrievaltoolkits_amd.score_ce import score_ce
    q, p, t = _inputs(dev, m, n, d, g)
    loss, S, dq, dp = _run_kd(q, p, t, g, 4.0, 1.0, 0.0)
    q2, p2 = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
    l2, S2 = score_ce(q2, p2, g, SCALE)
    (UPSTREAM * l2).backward()
    assert torch.equal(loss, l2.detach()) and torch.equal(S, S2.detach())
    assert torch.equal(dq, q2.grad) and torch.equal(dp, p2.grad)


@pytest.mark.parametrize("m,n,d", [(8, 16, 64), (37, 111, 100), (32, 64, 32), (1, 5, 64)])
@pytest.mark.parametrize("T", [0.5, 3.0])
def test_group_of_one_has_no_distillation_term(dev, m, n, d, T):
    """g = 1: both softmaxes are exactly 1, so KL = 0 and its gradient is 0, bit for bit -- also for a
    dropped query."""
    import torch
    q, p, t = _inputs(dev, m, n, d, 1)
    a = _run_kd(q, p, t, 1, T, W_CE, W_KD)
    b = _run_kd(q, p, t, 1, T, W_CE, 0.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("m,n,d,g", SHAPES)
def test_fused_against_unfused_kernels(dev, m, n, d, g):
    """drt_score_kd_fwd / _bwd == drt_gemm_f32 + drt_kd_fwd + drt_kd_bwd + drt_gemm_f32 x 2: bit for bit on the
    ragged shapes (the same fixed-order split-K sums), to the gradient tolerance where m, n, d are multiples of
    32 (the large-tile GEMMs sum in another order), as test_fused_score_ce_bit_identical_to_unfused_kernels."""
    import torch
    from denseretrievaltoolkits_amd import _native
    from denseretrievaltoolkits_amd.score_ce import gemm_f32
    lib = _native.load()
    T = 0.5
    (q, p, t), (loss, S, dq, dp), _ = _case(dev, m, n, d, g, T)
    s = _native.stream_ptr(dev)
    S2 = gemm_f32(q, p, True, True, m, n, d)
    lse, rl, l2 = torch.empty(m, device=dev), torch.empty(m, device=dev), torch.empty((), device=dev)
    aux = torch.empty(m, 2, device=dev)
    _native.check(lib.drt_kd_fwd(S2.data_ptr(), t.data_ptr(), m, n, g, T, W_CE, W_KD, SCALE, lse.data_ptr(),
                                 aux.data_ptr(), rl.data_ptr(), l2.data_ptr(), s), "drt_kd_fwd")
    up = torch.tensor([UPSTREAM], device=dev)
    dS = torch.empty_like(S2)
    _native.check(lib.drt_kd_bwd(S2.data_ptr(), t.data_ptr(), lse.data_ptr(), aux.data_ptr(), m, n, g, T, W_CE, W_KD,
                                 up.data_ptr(), SCALE, dS.data_ptr(), s), "drt_kd_bwd")
    dq2 = gemm_f32(dS, p, True, False, m, d, n)
    dp2 = gemm_f32(dS, q, False, False, n, d, m)
    if m % 32 or n % 32 or d % 32:
        assert torch.equal(S, S2) and torch.equal(loss, l2)
        assert torch.equal(dq, dq2) and torch.equal(dp, dp2)
    else:
        torch.testing.assert_close(S, S2, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(loss, l2, rtol=1e-5, atol=0.0)
        torch.testing.assert_close(dq, dq2, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(dp, dp2, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("m,n,d,g", SHAPES)
def test_same_inputs_same_bits(dev, m, n, d, g):
    import torch
    (q, p, t), first, _ = _case(dev, m, n, d, g, 1.0)
    again = _run_kd(q, p, t, g, 1.0, W_CE, W_KD)
    for x, y in zip(first, again):
        assert torch.equal(x, y)


def test_bf16_inputs_promoted_and_bad_arguments_refused(dev):
    import torch
    from denseretrievaltoolkits_amd.score_ce import score_kd
    q, p, t = _inputs(dev, 8, 16, 64, 2)
    qb, pb = q.bfloat16().requires_grad_(True), p.bfloat16().requires_grad_(True)
    loss, S = score_kd(qb, pb, t, 2, temperature=2.0, w_ce=1.0)
    loss.backward()
    assert S.dtype == torch.float32 and qb.grad.dtype == torch.bfloat16 and torch.isfinite(qb.grad.float()).all()
    want, _ = score_kd(qb.detach().float(), pb.detach().float(), t, 2, temperature=2.0, w_ce=1.0)
    assert torch.equal(loss.detach(), want)
    for kw in (dict(temperature=0.0), dict(temperature=float("inf")), dict(w_ce=-1.0), dict(w_kd=-1.0)):
        with pytest.raises(ValueError):
            score_kd(q, p, t, 2, **kw)
    with pytest.raises(ValueError):
        score_kd(q, p, t[:, :1], 2)
    with pytest.raises(ValueError):
        score_kd(q, p[:15], t, 2)          # m g > n
    with pytest.raises(ValueError):
        torch.ops.drt.score_kd_fwd(q, p, t.double(), 2, 1.0, 0.0, 1.0, 1.0)   # the op itself checks dtypes


def test_opcheck_score_kd(dev):
    import torch
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    q, p, t = _inputs(dev, 8, 16, 64, 2)
    q.requires_grad_(True)
    p.requires_grad_(True)
    torch.library.opcheck(drt.score_kd_fwd.default, (q, p, t, 2, 2.0, 0.5, 1.0, 1.0), None,
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration",
                                      "test_aot_dispatch_dynamic"))
    loss, S, lse, aux = drt.score_kd_fwd(q, p, t, 2, 2.0, 0.5, 1.0, 1.0)
    assert not S.requires_grad and not lse.requires_grad and not aux.requires_grad
    tg = t.clone().requires_grad_(True)
    loss, *_ = drt.score_kd_fwd(q, p, tg, 2, 2.0, 0.5, 1.0, 1.0)
    loss.backward()
    assert tg.grad is None and q.grad is not None


def test_score_kd_captures_as_one_graph(dev):
    """No host synchronisation or allocation inside the entries: forward + backward replay from a graph."""
    import torch
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    q, p, t = _inputs(dev, 37, 111, 100, 3)
    up = torch.ones((), device=dev)
    want = drt.score_kd_fwd(q, p, t, 3, 2.0, 0.5, 1.0, 1.0)
    wantg = drt.score_kd_bwd(up, q, p, t, want[1], want[2], want[3], 3, 2.0, 0.5, 1.0, 1.0)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = drt.score_kd_fwd(q, p, t, 3, 2.0, 0.5, 1.0, 1.0)
            grads = drt.score_kd_bwd(up, q, p, t, out[1], out[2], out[3], 3, 2.0, 0.5, 1.0, 1.0)
        for x in out + grads:
            x.zero_()
        graph.replay()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    for x, y in zip(out + grads, want + wantg):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ model / trainer
def _tower(layers, seed, dev):
    import torch
    from transformers import BertModel
    from oracle import bert_weights as bw
    torch.manual_seed(0)
    lm = BertModel(bw.bert_config(layers=layers), add_pooling_layer=False)
    return bw.init_model_(lm, seed).to(dev)


def _batch(dev, B, n, Lq, Lp):
    import torch
    from oracle import bert_weights as bw
    qi, qm = bw.token_batch(B, Lq, seed=31)
    pi, pm = bw.token_batch(B * n, Lp, seed=32)
    return ({"input_ids": torch.from_numpy(qi).to(dev), "attention_mask": torch.from_numpy(qm).to(dev)},
            {"input_ids": torch.from_numpy(pi).to(dev), "attention_mask": torch.from_numpy(pm).to(dev)})


def test_drmodel_forward_with_teacher_scores(dev):
    import torch
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    B, n = 4, 3
    lm = _tower(2, 5, dev)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="first", data_args=SimpleNamespace(train_n_passages=n),
                    train_args=SimpleNamespace(negatives_x_device=False, distill_temperature=2.0,
                                               distill_ce_weight=0.5, distill_kd_weight=1.5))
    model.train()
    query, passage = _batch(dev, B, n, 16, 32)
    before = model(query=query, passage=passage)          # before anything of the distillation is built
    from denseretrievaltoolkits_amd.score_ce import score_kd
    gen = torch.Generator(device=dev).manual_seed(3)
    teacher = torch.randn(B, n, generator=gen, device=dev) * 3.0
    teacher[1, 2] = -math.inf
    out = model(query=query, passage=passage, teacher_scores=teacher)
    want_loss, want_scores = score_kd(out.q_reps.detach(), out.p_reps.detach(), teacher, n, temperature=2.0,
                                      w_ce=0.5, w_kd=1.5)
    assert torch.equal(out.loss.detach(), want_loss) and torch.equal(out.scores.detach(), want_scores)
    out.loss.backward()
    g = model.lm_q.embeddings.word_embeddings.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    # the defaults: T = 1, w_ce = 0, w_kd = 1 when the training arguments do not carry the fields
    model.train_args = SimpleNamespace(negatives_x_device=False)
    dflt = model(query=query, passage=passage, teacher_scores=teacher.cpu())   # moved to the reps' device
    want_loss, _ = score_kd(dflt.q_reps.detach(), dflt.p_reps.detach(), teacher, n)
    assert torch.equal(dflt.loss.detach(), want_loss)
    after = model(query=query, passage=passage)
    assert torch.equal(after.loss, before.loss) and torch.equal(after.scores, before.scores)
    assert torch.equal(after.q_reps, before.q_reps) and torch.equal(after.p_reps, before.p_reps)


def test_distill_trainer_train_step(dev):
    import torch
    from oracle import bert_weights as bw
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.model.linear import LinearHead
    from denseretrievaltoolkits_amd.model.reranker import RRModel
    from denseretrievaltoolkits_amd.score_ce import score_kd
    from denseretrievaltoolkits_amd.trainer.distill import DistillTrainer, pack_pairs, teacher_scores
    B, n, Lq, Lp = 4, 3, 16, 32
    lm = _tower(2, 5, dev)
    student = DRModel(lm_q=lm, lm_p=lm, pooling="first", data_args=SimpleNamespace(train_n_passages=n),
                      train_args=SimpleNamespace(negatives_x_device=False, distill_temperature=2.0,
                                                 distill_ce_weight=1.0, distill_kd_weight=4.0))
    head = LinearHead(768, 1)
    with torch.no_grad():
        head.linear.weight.copy_(torch.from_numpy(bw.param_value(2, "rr_head.linear.weight", (1, 768))))
    rr = RRModel(lm=_tower(1, 2, dev), head=head, pooling="first")
    args = SimpleNamespace(loss_fn="SimpleContrastiveLoss", learning_rate=1e-5, optimizer="adamw")
    tr = DistillTrainer(args, student, rr, pad_token_id=0)
    tr.model.train()
    opt_params = {id(p) for grp in tr.optimizer.param_groups for p in grp["params"]}
    assert not any(id(p) in opt_params for p in rr.parameters())
    assert all(not p.requires_grad and p.is_cuda for p in rr.parameters()) and not rr.training
    query, passage = _batch(dev, B, n, Lq, Lp)

    pairs = pack_pairs(query, passage, n, 0)
    assert pairs["input_ids"].shape == (B * n, Lq + Lp)
    with torch.no_grad():
        t_want = rr.encode(pairs).float().view(B, n)
        # 12 pairs in chunks of 5, 5, 2: the bf16 tower picks its GEMM plans by batch size, so the chunked
        # scores are those of the same chunks (bit for bit), and close to the one-pass ones
        t_chunks = torch.cat([rr.encode({k: v[a: a + 5] for k, v in pairs.items()}).float().view(-1)
                              for a in (0, 5, 10)]).view(B, n)
    assert torch.equal(teacher_scores(rr, query, passage, n, 0), t_want)
    assert torch.equal(teacher_scores(rr, query, passage, n, 0, chunk=5), t_chunks)
    torch.testing.assert_close(t_chunks, t_want, rtol=2e-2, atol=2e-2)
    assert float(t_want.std()) > 0

    loss = tr.train_step([query, passage])
    reps = tr.model(query=query, passage=passage)
    want, _ = score_kd(reps.q_reps.detach(), reps.p_reps.detach(), t_want, n, temperature=2.0, w_ce=1.0, w_kd=4.0)
    torch.testing.assert_close(loss.detach(), want, rtol=1e-5, atol=0.0)
    tr.optimizer.zero_grad()
    loss.backward()
    assert all(p.grad is None for p in rr.parameters())
    grads = [p.grad for p in lm.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0

    # a loader-supplied teacher_scores replaces the teacher
    given = torch.flip(t_want, dims=(1,)) + 1.0
    loss2 = tr.train_step([query, passage, {"teacher_scores": given}])
    want2, _ = score_kd(reps.q_reps.detach(), reps.p_reps.detach(), given, n, temperature=2.0, w_ce=1.0, w_kd=4.0)
    torch.testing.assert_close(loss2.detach(), want2, rtol=1e-5, atol=0.0)
    assert abs(loss2.item() - loss.item()) > 1e-4 * abs(loss.item())

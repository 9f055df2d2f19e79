"""GPU: filtered search and hard-negative mining end to end -- FlatIPIndex / ShardedFlatIP
``search_filtered_*``, ``pair_scores``, trainer.mining.mine_negatives and DenseNegatives -- against a numpy
restatement: mask the excluded rows, take fp64 scores of the bf16-valued inputs, order by (score descending,
id ascending).  Reference flow replaced: BM25Negatives.load_passages, DRT/trainer/sampler.py:57-99."""
import numpy as np
import pytest

from helpers import gauss_bf16, int_bf16, to_dev_bf16

pytestmark = pytest.mark.gpu

PAD_S = np.float32(-3.402823466e+38)


def masked_topk(q, p, lists, m, skip=0, ceiling=None, id_offset=0):
    """(ids [nq, m], fp64 scores [nq, m], count [nq]) of the corpus minus each query's list, below its
    ceiling (compared with the fp32-rounded score, as the index reports it), after ``skip``; pads -1."""
    S = q.astype(np.float64) @ p.astype(np.float64).T
    n = p.shape[0]
    ids = np.full((len(q), m), -1, np.int64)
    sc = np.full((len(q), m), np.float64(PAD_S))
    cnt = np.zeros(len(q), np.int64)
    for j in range(len(q)):
        ok = np.ones(n, bool)
        ex = np.asarray(list(lists[j]), np.int64) - id_offset
        ok[ex[(ex >= 0) & (ex < n)]] = False
        if ceiling is not None:
            ok &= S[j].astype(np.float32) < ceiling[j]
        rows = np.nonzero(ok)[0]
        order = rows[np.lexsort((rows, -S[j, rows]))]
        cnt[j] = order.size
        order = order[skip: skip + m]
        ids[j, : order.size] = order + id_offset
        sc[j, : order.size] = S[j, order]
    return ids, sc, cnt


def assert_scores(got, want64, exact):
    want = want64.astype(np.float32)
    if exact:
        np.testing.assert_array_equal(got, want)
    else:   # two fp64 summation orders rounded to fp32: at most one ulp apart
        assert (np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(want))).all()


@pytest.fixture(scope="module")
def int_case():
    """20,000 x 64 integer rows with heavy score ties, 130 queries; each excludes its true top-3 plus 5
    random ids.  The reference answer is computed once."""
    rng = np.random.default_rng(31)
    q, p = int_bf16(rng, (130, 64), -2, 2), int_bf16(rng, (20000, 64), -2, 2)
    top3, _, _ = masked_topk(q, p, [[]] * 130, 3)
    lists = [list(top3[j]) + list(rng.integers(0, 20000, size=5)) for j in range(130)]
    return q, p, lists, masked_topk(q, p, lists, 10)


@pytest.mark.parametrize("grouped", [False, True])
def test_integer_corpus_per_batch_and_grouped(dev, int_case, grouped, monkeypatch):
    import torch
    from denseretrievaltoolkits_amd import search as srch
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    q, p, lists, (ei, es, ec) = int_case
    if grouped:   # forced the way tests/test_search_gpu.py forces it
        monkeypatch.setattr(srch, "GROUP_MIN_ROWS", 0)
        monkeypatch.setattr(srch, "GROUP_QUERIES", 64)
        monkeypatch.setattr(srch, "GROUP_CHUNK_ROWS", 6000)
    idx = srch.FlatIPIndex.from_rows(to_dev_bf16(p, dev))
    assert idx._use_groups(18) == grouped
    excl, off = build_exclusions(lists, dev)
    qd = to_dev_bf16(q, dev)
    res = list(idx.search_filtered_batches_iter([qd[a: a + 32] for a in range(0, 130, 32)], 10, excl, off))
    torch.cuda.synchronize()
    gi = torch.cat([r[1] for r in res]).cpu().numpy()
    gs = torch.cat([r[0] for r in res]).cpu().numpy()
    gc = torch.cat([r[2] for r in res]).cpu().numpy()
    np.testing.assert_array_equal(gi, ei)
    assert_scores(gs, es, exact=True)
    # the depth-18 list lost exactly the excluded rows it held
    assert ((gc >= 10) & (gc <= 15)).all()
    # host form and the one-batch form
    hs, hi, hc = next(idx.search_filtered_batches_iter([qd[:32]], 10, excl[: int(off[32])], off[:33], to_host=True))
    assert isinstance(hi, np.ndarray)
    np.testing.assert_array_equal(hi, ei[:32])
    s1, i1, c1 = idx.search_filtered_device(qd[:7], 10, excl[: int(off[7])], off[:8])
    np.testing.assert_array_equal(i1.cpu().numpy(), ei[:7])
    if not grouped:
        from denseretrievaltoolkits_amd.evaluator.index import BaseFaissIPRetriever
        ret = BaseFaissIPRetriever(p[:1], device=dev)
        ret.add(p)
        np.testing.assert_array_equal(ret.search(q, 10, exclude=lists), ei)
        np.testing.assert_array_equal(ret.batch_search(q, 10, 48, exclude=lists), ei)
        np.testing.assert_array_equal(ret.last_scores, es.astype(np.float32))
        np.testing.assert_array_equal(ret.search(q[:5], 10), masked_topk(q[:5], p, [[]] * 5, 10)[0])


def test_gaussian_skip_and_ragged_exclusions(dev):
    """50,000 x 768 Gaussian rows, 64 queries, m = 100, skip = 20, 0-8 exclusions drawn from each query's own
    top 150 (so they bite): ids equal the fp64 masked order, no query left in the fp32 order."""
    import torch
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    rng = np.random.default_rng(32)
    q, p = gauss_bf16(rng, (64, 768)), gauss_bf16(rng, (50000, 768))
    top, _, _ = masked_topk(q, p, [[]] * 64, 150)
    lists = [list(rng.choice(top[j], size=j % 9, replace=False)) for j in range(64)]
    ei, es, _ = masked_topk(q, p, lists, 100, skip=20)
    idx = FlatIPIndex.from_rows(to_dev_bf16(p, dev))
    excl, off = build_exclusions(lists, dev)
    qd = to_dev_bf16(q, dev)
    res = list(idx.search_filtered_batches_iter([qd[:40], qd[40:]], 100, excl, off, skip=20))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat([r[1] for r in res]).cpu().numpy(), ei)
    assert_scores(torch.cat([r[0] for r in res]).cpu().numpy(), es, exact=False)
    assert idx.order_uncertified == 0


def test_depth_crossing_2048(dev):
    """5,000 rows, m = 2040 and 20 exclusions: depth 2060 takes the large-k path."""
    import torch
    from denseretrievaltoolkits_amd import kernels
    from denseretrievaltoolkits_amd.search import FlatIPIndex, filtered_depth
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    rng = np.random.default_rng(33)
    q, p = int_bf16(rng, (4, 128), -3, 3), int_bf16(rng, (5000, 128), -3, 3)
    top, _, _ = masked_topk(q, p, [[]] * 4, 100)
    lists = [list(rng.choice(top[j], size=20, replace=False)) for j in range(4)]
    ei, es, _ = masked_topk(q, p, lists, 2040)
    idx = FlatIPIndex.from_rows(to_dev_bf16(p, dev))
    excl, off = build_exclusions(lists, dev)
    assert filtered_depth(2040, 0, off, idx.ntotal) == 2060 > kernels.MAX_K
    s, i, c = idx.search_filtered_device(to_dev_bf16(q, dev), 2040, excl, off)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), ei)
    assert_scores(s.cpu().numpy(), es, exact=True)
    assert (c.cpu().numpy() == 2040).all()
    with pytest.raises(ValueError, match=str(kernels.MAX_K_LARGE)):
        idx.search_filtered_device(to_dev_bf16(q, dev), kernels.MAX_K_LARGE - 10, excl, off)


@pytest.fixture(scope="module")
def ceiling_case():
    """3,000 Gaussian rows, 20 queries whose positive is the row at true rank 200 (0-based)."""
    rng = np.random.default_rng(34)
    q, p = gauss_bf16(rng, (20, 128)), gauss_bf16(rng, (3000, 128))
    top, ts, _ = masked_topk(q, p, [[]] * 20, 201)
    return q, p, [[int(top[j, 200])] for j in range(20)], ts[:, 200].astype(np.float32)


def test_ceiling_escalation(dev, ceiling_case):
    """Positive-aware filtering from an initial depth of 16: the ceiling (0.95 x the positive's score, the
    product in fp32) removes each query's top ~200, so every query is searched again at doubled depths until
    10 candidates survive; the result equals the masked order below the ceiling."""
    import torch
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    from denseretrievaltoolkits_amd.trainer.mining import mine_negatives
    q, p, pos, pos_s = ceiling_case
    ceil = (pos_s * np.float32(0.95)).astype(np.float32)
    ei, es, ec = masked_topk(q, p, pos, 10, ceiling=ceil)
    assert ((3000 - ec) > 200).all()
    idx = FlatIPIndex.from_rows(to_dev_bf16(p, dev))
    ids, sc, cnt, incomplete = mine_negatives(idx, to_dev_bf16(q, dev), pos, 10, max_pos_ratio=0.95, depth=16,
                                              batch_size=8)
    torch.cuda.synchronize()
    assert incomplete == 0
    np.testing.assert_array_equal(ids.cpu().numpy(), ei)
    assert_scores(sc.cpu().numpy(), es, exact=False)
    assert (cnt.cpu().numpy() >= 10).all()
    # no ceiling, a rank offset and extra exclusions: one search at the exact rule's depth
    top3 = masked_topk(q, p, [[]] * 20, 3)[0]
    extra = [[int(r) for r in top3[j]] for j in range(20)]
    ids2, _, cnt2, inc2 = mine_negatives(idx, to_dev_bf16(q, dev), pos, 10, skip=4, extra_exclude=extra)
    want = masked_topk(q, p, [pos[j] + extra[j] for j in range(20)], 10, skip=4)[0]
    np.testing.assert_array_equal(ids2.cpu().numpy(), want)
    # depth 4 + 10 + 4 = 18: the list lost the three top rows (the positive, at rank 200, is not in it)
    assert inc2 == 0 and (cnt2.cpu().numpy() == 15).all()


def test_ceiling_below_every_score(dev, ceiling_case):
    """A ceiling below every score: the depth doubles until the list is the whole corpus -- nothing survives,
    and no query counts as incomplete because the corpus is exhausted."""
    from denseretrievaltoolkits_amd.search import FlatIPIndex
    from denseretrievaltoolkits_amd.trainer.mining import mine_negatives
    q, p, pos, pos_s = ceiling_case
    assert (pos_s > 0).all()
    idx = FlatIPIndex.from_rows(to_dev_bf16(p, dev))
    ids, sc, cnt, incomplete = mine_negatives(idx, to_dev_bf16(q, dev), pos, 10, max_pos_ratio=-1e6, depth=16)
    assert incomplete == 0
    assert (cnt.cpu().numpy() == 0).all() and (ids.cpu().numpy() == -1).all() and (sc.cpu().numpy() == PAD_S).all()


def test_sharded_world1_with_offset(dev, int_case):
    """ShardedFlatIP at world size 1 whose shard starts at a nonzero global id: exclusions, results and
    pair_scores speak global ids."""
    import torch
    from denseretrievaltoolkits_amd.search import ShardedFlatIP
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    q, p, lists, (ei, es, _) = int_case
    off0 = 1_000_003
    idx = ShardedFlatIP(64, device=dev)
    idx.add_shard(to_dev_bf16(p, dev))
    idx.offset = off0
    excl, off = build_exclusions([[i + off0 for i in l] for l in lists], dev)
    qd = to_dev_bf16(q, dev)
    res = list(idx.search_filtered_batches_iter([qd[:100], qd[100:]], 10, excl, off))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat([r[1] for r in res]).cpu().numpy(), ei + off0)
    assert_scores(torch.cat([r[0] for r in res]).cpu().numpy(), es, exact=True)
    s1, i1, _ = idx.search_filtered_device(qd[:5], 10, excl[: int(off[5])], off[:6])
    np.testing.assert_array_equal(i1.cpu().numpy(), ei[:5] + off0)
    ps = idx.pair_scores(qd, [0, 1, 2, 3], [off0, off0 + 19999, off0 - 1, off0 + 20000]).cpu().numpy()
    want = [np.float32(q[0].astype(np.float64) @ p[0]), np.float32(q[1].astype(np.float64) @ p[19999]), PAD_S, PAD_S]
    np.testing.assert_array_equal(ps, np.array(want, np.float32))


def _w_sharded_filtered(rank, world, dev):
    import torch
    from oracle import search_oracle as orc
    from denseretrievaltoolkits_amd.search import ShardedFlatIP
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions, mine_negatives
    rng = np.random.default_rng(35)
    q, p = gauss_bf16(rng, (21, 768)), gauss_bf16(rng, (30001, 768))
    top, ts, _ = masked_topk(q, p, [[]] * 21, 40)
    lists = [list(rng.choice(top[j], size=j % 6, replace=False)) for j in range(21)]
    ei, es, _ = masked_topk(q, p, lists, 25, skip=3)
    lo, hi = orc.shard_bounds(p.shape[0], world, rank)
    idx = ShardedFlatIP(768, device=dev)
    idx.add_shard(to_dev_bf16(p[lo:hi], dev))
    excl, off = build_exclusions(lists, dev)
    qd = to_dev_bf16(q, dev)
    res = list(idx.search_filtered_batches_iter([qd[:8], qd[8:]], 25, excl, off, skip=3))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat([r[1] for r in res]).cpu().numpy(), ei)
    assert_scores(torch.cat([r[0] for r in res]).cpu().numpy(), es, exact=False)
    # pair_scores across the two shards: every pair's row lives on one rank, the MAX all-reduce completes it
    qidx = np.repeat(np.arange(21), 40)
    ps = idx.pair_scores(qd, qidx, top.reshape(-1)).cpu().numpy().reshape(21, 40)
    assert_scores(ps, ts, exact=False)
    assert idx.pair_scores(qd, [0], [30001]).item() == PAD_S
    # mining through the sharded index, positive-aware: the positive is each query's 10th row
    pos = [[int(top[j, 9])] for j in range(21)]
    ceil = (ts[:, 9].astype(np.float32) * np.float32(0.98)).astype(np.float32)
    wi, _, _ = masked_topk(q, p, pos, 5, ceiling=ceil)
    ids, _, _, incomplete = mine_negatives(idx, qd, pos, 5, max_pos_ratio=0.98)
    np.testing.assert_array_equal(ids.cpu().numpy(), wi)
    return incomplete


def test_sharded_world2_filtered_search_and_pair_scores():
    from test_multirank_gpu import _spawn
    res = _spawn(_w_sharded_filtered, 2)
    assert res == {0: 0, 1: 0}


# ---------------------------------------------------------------------------
# DenseNegatives
# ---------------------------------------------------------------------------
class StubTokenizer:
    """The two tokenizer calls the collators make (DRT/dataset/data_collator.py:6-15, 48-53): [CLS] tokens
    [SEP] truncated to max_length, then right-padding with 0 and an attention mask."""
    cls_id, sep_id, pad_id = 101, 102, 0

    def prepare_for_model(self, ids, truncation=None, max_length=None, padding=False, return_attention_mask=False,
                          return_token_type_ids=False):
        return {"input_ids": [self.cls_id] + list(ids)[: max_length - 2] + [self.sep_id]}

    def pad(self, items, padding=None, max_length=None, return_tensors=None):
        import torch
        ids = torch.full((len(items), max_length), self.pad_id, dtype=torch.int64)
        mask = torch.zeros((len(items), max_length), dtype=torch.int64)
        for j, it in enumerate(items):
            n = len(it["input_ids"])
            ids[j, :n] = torch.tensor(it["input_ids"])
            mask[j, :n] = 1
        return {"input_ids": ids, "attention_mask": mask}


class CountingModel:
    def __init__(self, model):
        self.model, self.calls = model, 0

    def parameters(self):
        return self.model.parameters()

    def encode_passage(self, items):
        self.calls += 1
        return self.model.encode_passage(items)

    def encode_query(self, items):
        self.calls += 1
        return self.model.encode_query(items)


def test_dense_negatives(dev, tmp_path):
    """300 samples of 1 positive + 3 negatives over a pool with shared passages, a one-layer tower: every
    sample gets exactly num_negative negatives, none token-equal to one of its positives, equal to the masked
    order over the miner's own index rows and query reps; the second call reads the cache."""
    from types import SimpleNamespace
    import torch
    from transformers import BertModel
    from oracle import bert_weights as bw
    from denseretrievaltoolkits_amd.model.biencoder import DRModel
    from denseretrievaltoolkits_amd.trainer.mining import DenseNegatives
    rng = np.random.default_rng(36)
    pool = [[int(t) for t in rng.integers(1000, 30000, size=int(rng.integers(5, 30)))] for _ in range(500)]
    corpus = []
    for j in range(300):
        picks = rng.choice(500, size=4, replace=False)   # passages are shared between samples
        corpus.append({"query": [int(t) for t in rng.integers(1000, 30000, size=int(rng.integers(3, 12)))],
                       "positives": [pool[picks[0]]], "negatives": [pool[i] for i in picks[1:]]})
    torch.manual_seed(0)
    lm = BertModel(bw.bert_config(layers=1), add_pooling_layer=False).eval()
    bw.init_model_(lm, 5)
    model = CountingModel(DRModel(lm_q=lm, lm_p=lm, pooling="first", normalize=True).to(dev).eval())
    args = SimpleNamespace(data_cache_dir=str(tmp_path), train_n_passages=8, q_max_len=16, p_max_len=32)
    miner = DenseNegatives(args, model, StubTokenizer(), batch_size=128)
    data = miner.load_passages(corpus)
    assert len(data) == 300 and model.calls > 0 and miner.incomplete == 0
    # passages with identical token lists share one row: a positive of one sample is never another row
    assert len(miner.passages) == len({tuple(x) for x in miner.passages}) <= 500
    rows = miner.index.rows.float().cpu().numpy()
    qr = miner.q_reps.to(torch.bfloat16).float().cpu().numpy()
    want, _, _ = masked_topk(qr, rows, miner.pos_rows, 7)
    for j in range(300):
        negs = data[j]["negatives"]
        assert len(negs) == 7
        assert all(n not in corpus[j]["positives"] for n in negs)
        assert negs == [miner.passages[r] for r in want[j]]
        assert data[j]["query"] == corpus[j]["query"] and data[j]["positives"] == corpus[j]["positives"]
    assert len(corpus[0]["negatives"]) == 3   # the caller's samples are left as they were
    calls = model.calls
    again = DenseNegatives(args, model, StubTokenizer()).load_passages(corpus)
    assert model.calls == calls
    assert [again[j] for j in range(300)] == [data[j] for j in range(300)]

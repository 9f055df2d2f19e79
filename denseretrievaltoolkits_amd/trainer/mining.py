"""Dense hard-negative mining on the exact index (served as ``DRT.trainer.mining`` by the overlay).

The reference mines hard negatives with BM25 only (run_BM25_negative.py through
``BM25Negatives.load_passages``, DRT/trainer/sampler.py:57-99): it searches
``num_negative + len(positives)`` passages, skips the sample's own positives and keeps the first
``num_negative`` -- in pure Python, on the CPU.  This module does the same with the model's own
embeddings and the device-resident exact index:

``build_exclusions``   per-query id lists -> the sorted CSR the filtered search takes.
``mine_negatives``     exact top-m of (corpus minus each query's positives), optionally below a
                       fraction of the positive's score (positive-aware filtering) and after a rank
                       offset; everything stays on the GPU.
``DenseNegatives``     ``BM25Negatives``-shaped: ``load_passages(train_dataset)`` returns the dataset with
                       every sample's ``negatives`` replaced by mined ones.

Exactness (DESIGN.md "Filtered search"): the index's top-K list in canonical order loses at most |E_q|
entries to a query's exclusions, so its first skip + m survivors are the top-(skip + m) of the corpus
minus E_q when K >= skip + m + |E_q|.  A score ceiling drops an unknown number of entries: the
filter reports how many survived and the queries that came up short are searched again, only those, at
doubled depth.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import kernels


def build_exclusions(lists: Sequence[Sequence[int]], device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(excl int64 [E], excl_off int64 [len(lists) + 1]): every list sorted ascending and de-duplicated,
    concatenated; list j is ``excl[excl_off[j]:excl_off[j + 1]]``.  Empty lists (and no lists) are fine."""
    segs = [np.unique(np.asarray(list(x), dtype=np.int64).reshape(-1)) for x in lists]
    off = np.zeros(len(segs) + 1, dtype=np.int64)
    if segs:
        off[1:] = np.cumsum([s.size for s in segs])
    excl = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int64)
    excl_t, off_t = torch.from_numpy(excl.astype(np.int64, copy=False)), torch.from_numpy(off)
    if device is not None:
        excl_t, off_t = excl_t.to(device), off_t.to(device)
    return excl_t, off_t


def positive_ceilings(index, q_reps: torch.Tensor, positives: Sequence[Sequence[int]], ratio: float) -> torch.Tensor:
    """fp32 [Q] score ceilings of positive-aware filtering: ``ratio`` x the largest of the query's positives'
    scores in the index's own numerics (index.pair_scores: the exact sums rounded to fp32, what its search
    reports), the product taken in fp32; +inf (no ceiling) for a query without positives."""
    dev = q_reps.device
    qidx = np.concatenate([np.full(len(p), j, dtype=np.int32) for j, p in enumerate(positives)]
                          or [np.zeros(0, np.int32)])
    rows = np.concatenate([np.asarray(list(p), dtype=np.int64).reshape(-1) for p in positives]
                          or [np.zeros(0, np.int64)])
    ceil = torch.full((len(positives),), float("inf"), dtype=torch.float32, device=dev)
    if rows.size == 0:
        return ceil
    qi = torch.from_numpy(qidx).to(dev)
    ps = index.pair_scores(q_reps, qi, torch.from_numpy(rows).to(dev))
    best = torch.full((len(positives),), float("-inf"), dtype=torch.float32, device=dev)
    best.scatter_reduce_(0, qi.long(), ps, reduce="amax")
    has = torch.zeros(len(positives), dtype=torch.bool, device=dev)
    has[qi.long()] = True
    return torch.where(has, best * float(ratio), ceil)


def mine_negatives(index, q_reps, positives: Sequence[Sequence[int]], num_negatives: int, *, skip: int = 0,
                   max_pos_ratio: Optional[float] = None, extra_exclude: Optional[Sequence[Sequence[int]]] = None,
                   batch_size: int = 128, depth: Optional[int] = None):
    """Hard negatives of every query from ``index`` (a FlatIPIndex or ShardedFlatIP holding the passages).

    ``positives[j]``: index ids of query j's positives, always excluded (``extra_exclude[j]``: more ids to
    leave out).  ``max_pos_ratio`` = r: only passages scoring below r x the best positive's score
    (``positive_ceilings``); a query with no positive has no ceiling.  ``skip``: drop each query's first
    ``skip`` surviving candidates.  ``depth``: first search depth, at least the exact rule's
    skip + num_negatives + the longest exclusion list.

    A query is complete once ``skip + num_negatives`` candidates survived or its list held the whole corpus.
    With a ceiling the others are searched again -- only they -- at doubled depth until MAX_K_LARGE.
    Returns (neg_ids int64 [Q, m], neg_scores fp32 [Q, m], counts int32 [Q] = survivors in the deepest list
    searched for that query, incomplete = queries still short at the depth limit, never silently cut);
    rows short of m negatives are padded (-1, -FLT_MAX).  Device tensors."""
    dev = index.local.device if hasattr(index, "local") else index.device
    qd = (index.local if hasattr(index, "local") else index)._queries(q_reps)
    nq, m = qd.shape[0], int(num_negatives)
    if len(positives) != nq:
        raise ValueError(f"{len(positives)} positive lists for {nq} queries")
    if extra_exclude is not None and len(extra_exclude) != nq:
        raise ValueError(f"{len(extra_exclude)} extra exclusion lists for {nq} queries")
    lists = [list(p) + (list(extra_exclude[j]) if extra_exclude is not None else [])
             for j, p in enumerate(positives)]
    ceiling = positive_ceilings(index, qd, positives, max_pos_ratio) if max_pos_ratio is not None else None
    neg_ids = torch.full((nq, m), -1, dtype=torch.int64, device=dev)
    neg_scores = torch.full((nq, m), torch.finfo(torch.float32).min, dtype=torch.float32, device=dev)
    counts = torch.zeros((nq,), dtype=torch.int32, device=dev)
    if nq == 0:
        return neg_ids, neg_scores, counts, 0
    from ..search import filtered_depth

    todo = torch.arange(nq, device=dev)
    K = None
    while True:
        sub = [lists[j] for j in todo.tolist()] if K is not None else lists
        excl, excl_off = build_exclusions(sub, dev)
        # the depth actually searched: the exact rule, the caller's / the doubled depth, at most the corpus
        K = filtered_depth(m, skip, excl_off, index.ntotal, depth if K is None else K)
        qs = qd if todo.numel() == nq else qd.index_select(0, todo)
        cs = None if ceiling is None else (ceiling if todo.numel() == nq else ceiling.index_select(0, todo))
        res = list(index.search_filtered_batches_iter([qs[a: a + batch_size] for a in range(0, qs.shape[0], batch_size)],
                                                      m, excl, excl_off, skip=skip, ceiling=cs, depth=K))
        neg_scores.index_copy_(0, todo, torch.cat([r[0] for r in res]))
        neg_ids.index_copy_(0, todo, torch.cat([r[1] for r in res]))
        cnt = torch.cat([r[2] for r in res])
        counts.index_copy_(0, todo, cnt)
        if K >= index.ntotal:   # every row was in the list: the corpus is exhausted, nothing deeper exists
            return neg_ids, neg_scores, counts, 0
        short = todo[cnt < skip + m]
        if short.numel() == 0:
            return neg_ids, neg_scores, counts, 0
        if K >= kernels.MAX_K_LARGE:
            return neg_ids, neg_scores, counts, int(short.numel())
        todo, K = short, min(2 * K, kernels.MAX_K_LARGE)


class ListDataset(Dataset):
    """A plain list-backed dataset (the ``ListDataset`` BM25Negatives.load_passages returns, sampler.py:99,
    without defining it)."""

    def __init__(self, data: List):
        self.data = data

    def __getitem__(self, item):
        return self.data[item]

    def __len__(self):
        return len(self.data)


def pool_passages(corpus):
    """Every sample's positives, then its negatives, pooled into one passage set in first-seen order, passages
    with identical token lists merged into one row.  Returns (passages: token lists by row, pos_rows: per
    sample the rows of its positives).  (The reference's contiguous-range skip, sampler.py:74, knows nothing
    of duplicates: a positive of one sample comes back as a "negative" of another that shares it.)"""
    row_of, passages, pos_rows = {}, [], []

    def row(tokens):
        key = tuple(int(t) for t in tokens)
        r = row_of.get(key)
        if r is None:
            r = row_of[key] = len(passages)
            passages.append(list(key))
        return r

    for sample in corpus:
        pos_rows.append([row(p) for p in sample["positives"]])
        for p in sample.get("negatives", ()):
            row(p)
    return passages, pos_rows


class DenseNegatives:
    """``BM25Negatives`` (DRT/trainer/sampler.py:49-99) with the model's own embeddings: in the reference's
    run_BM25_negative.py, ``DenseNegatives(data_args, model, tokenizer).load_passages(train_dataset)`` in
    place of ``BM25Negatives(data_args, tokenizer.vocab_size).load_passages(train_dataset)``."""

    cache_name = "densenegatives"

    def __init__(self, data_args, model, tokenizer, *, skip: int = 0, max_pos_ratio: Optional[float] = None,
                 batch_size: int = 128):
        self.cache_dir = data_args.data_cache_dir
        self.num_negative = data_args.train_n_passages - 1
        self.q_max_len = data_args.q_max_len
        self.p_max_len = data_args.p_max_len
        self.model, self.tokenizer = model, tokenizer
        self.skip, self.max_pos_ratio, self.batch_size = skip, max_pos_ratio, batch_size
        # what the last mining run worked on (inspection / tests)
        self.index = self.q_reps = self.passages = self.pos_rows = None
        self.incomplete = 0

    def _inputs(self, token_lists, max_len):
        # as the collators build them (DRT/dataset/data_collator.py:6-15 create_one_example, then pad)
        enc = [self.tokenizer.prepare_for_model(t, truncation="only_first", max_length=max_len, padding=False,
                                                return_attention_mask=False, return_token_type_ids=False)
               for t in token_lists]
        return self.tokenizer.pad(enc, padding="max_length", max_length=max_len, return_tensors="pt")

    def _encode(self, token_lists, max_len, encode):
        dev = next(self.model.parameters()).device
        out = []
        with torch.no_grad():
            for a in range(0, len(token_lists), self.batch_size):
                items = self._inputs(token_lists[a: a + self.batch_size], max_len)
                out.append(encode({k: v.to(dev) for k, v in items.items()})[1].float())
        return torch.cat(out)

    def load_passages(self, corpus):
        out_dir = os.path.join(self.cache_dir, "DenseNegativesdata")
        path = os.path.join(out_dir, self.cache_name)
        if os.path.exists(path):
            with open(path, "r", encoding="utf-8") as f:
                return ListDataset([json.loads(line) for line in f])
        from ..search import FlatIPIndex
        samples = [corpus[j] for j in range(len(corpus))]
        self.passages, self.pos_rows = pool_passages(samples)
        p_reps = self._encode(self.passages, self.p_max_len, self.model.encode_passage)
        self.q_reps = self._encode([s["query"] for s in samples], self.q_max_len, self.model.encode_query)
        self.index = FlatIPIndex(p_reps.shape[1], device=p_reps.device)
        self.index.add(p_reps)
        ids, _, _, self.incomplete = mine_negatives(self.index, self.q_reps, self.pos_rows, self.num_negative,
                                                    skip=self.skip, max_pos_ratio=self.max_pos_ratio,
                                                    batch_size=self.batch_size)
        data = []
        for sample, row_ids in zip(samples, ids.cpu().tolist()):
            sample = dict(sample)
            sample["negatives"] = [self.passages[r] for r in row_ids if r >= 0]
            data.append(sample)
        self.save(data, out_dir, self.cache_name)
        return ListDataset(data)

    def save(self, data, out_dir, data_name):
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, data_name), "w", encoding="utf-8") as f:
            for sample in data:
                json.dump(sample, f, ensure_ascii=False)
                f.write("\n")

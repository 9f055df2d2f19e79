"""Drop-in for DRT/evaluator/index.py on the MI355X search kernels.

``BaseFaissIPRetriever`` keeps the reference constructor / add / search /
batch_search contract (DRT/evaluator/index.py:16-44) and its public ``index``
attribute, but the index is a device-resident bf16 ``FlatIPIndex`` searched by
the fused HIP scan + top-k kernels instead of a CPU faiss.IndexFlatIP.

Behaviour notes (vs the reference):
* ``search`` returns only the ids, [nq, k] int64, ordered by descending score
  (index.py:32-33); ties are ordered by ascending id (the reference's
  ``np.argsort(-scores)`` leaves them unspecified).  The scores of the last
  search stay available as ``last_scores``.
* ``batch_search`` returns the concatenated ids (the reference's version
  unpacks ``search``'s single return value into two names and raises; the
  intent — batching over queries — is kept).
* rows are stored as bf16: scores are exact fp32 dot products of the
  bf16-rounded embeddings.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from ..search import FlatIPIndex


class BaseFaissIPRetriever:
    def __init__(self, init_reps, device=None):
        if isinstance(init_reps, np.ndarray):
            index = FlatIPIndex(init_reps.shape[1], device=device)
        elif init_reps is None:
            index = None
        else:
            index = FlatIPIndex(int(init_reps), device=device)
        self.index = index
        self.docid: List = []
        self.last_scores: Optional[np.ndarray] = None
        self.last_rows: Optional[np.ndarray] = None   # best-row ids of the last grouped search

    def add(self, p_reps) -> None:
        self.index.add(p_reps)

    def search(self, q_reps, k: int = 1000, exclude=None) -> np.ndarray:
        """``exclude``: a sequence of per-query id sequences (or None) -- query j's result is then the
        top-k of the rows NOT in ``exclude[j]``, exactly (FlatIPIndex.search_filtered_device; the skip
        loop of BM25Negatives.load_passages, DRT/trainer/sampler.py:69-80, without its over-fetch
        guess).  Rows short of k hits are padded -1."""
        if exclude is None:
            scores, indices = self.index.search(q_reps, k)
            self.last_scores = scores
            return indices
        return self.batch_search(q_reps, k, max(1, q_reps.shape[0]), exclude=exclude)

    def search_device(self, q_reps, k: int = 1000):
        """Device tensors (scores fp32, ids int64) without the host round trip."""
        return self.index.search_device(q_reps, k)

    def batch_search(self, q_reps, k: int, batch_size: int, quiet: bool = False, exclude=None) -> np.ndarray:
        """All query batches enqueued back to back (FlatIPIndex.search_batches_iter: batch j + 1 is
        on the GPU while batch j is certified and its results land in pinned host memory).
        ``exclude``: per-query id sequences to leave out (see ``search``)."""
        n = q_reps.shape[0]
        if n == 0:
            return np.zeros((0, k), dtype=np.int64)
        qd = self.index._queries(q_reps)
        if exclude is not None:
            from ..trainer.mining import build_exclusions
            if len(exclude) != n:
                raise ValueError(f"exclude holds {len(exclude)} id lists for {n} queries")
            excl, excl_off = build_exclusions(exclude, self.index.device)
            res = list(self.index.search_filtered_batches_iter(
                [qd[a: a + batch_size] for a in range(0, n, batch_size)], k, excl, excl_off, to_host=True))
            self.last_scores = np.concatenate([r[0] for r in res])
            return np.concatenate([r[1] for r in res])
        res = list(self.index.search_batches_iter([qd[a: a + batch_size] for a in range(0, n, batch_size)], k,
                                                  to_host=True))
        self.last_scores = np.concatenate([r[0] for r in res])
        return np.concatenate([r[1] for r in res])

    # document-level (MaxP) retrieval: rows are passages, groups the documents they were cut from
    def set_groups(self, groups) -> None:
        """``groups[row]`` = the group (document) id of every indexed row (FlatIPIndex.set_groups)."""
        self.index.set_groups(groups)

    def search_grouped(self, q_reps, k: int = 1000, groups=None) -> np.ndarray:
        """Group ids [nq, k] of the best k groups, each scored by its best row, exactly
        (FlatIPIndex.search_grouped_batches_iter: no over-fetch guess, no host-side dedup); rows short of k
        groups are padded -1.  ``last_scores`` / ``last_rows`` keep the best rows' scores and ids.
        ``groups``: a row -> group map to set first (None: the one ``set_groups`` stored)."""
        return self.batch_search_grouped(q_reps, k, max(1, q_reps.shape[0]), groups=groups)

    def batch_search_grouped(self, q_reps, k: int, batch_size: int, groups=None) -> np.ndarray:
        """``search_grouped`` in query batches of ``batch_size`` (batch j + 1 is searched while batch j is
        collapsed and copied to the host)."""
        if groups is not None:
            self.index.set_groups(groups)
        n = q_reps.shape[0]
        if n == 0:
            self.last_scores = np.zeros((0, k), dtype=np.float32)
            self.last_rows = np.zeros((0, k), dtype=np.int64)
            return np.zeros((0, k), dtype=np.int32)
        qd = self.index._queries(q_reps)
        res = list(self.index.search_grouped_batches_iter([qd[a: a + batch_size] for a in range(0, n, batch_size)], k,
                                                          to_host=True))
        self.last_scores = np.concatenate([r[0] for r in res])
        self.last_rows = np.concatenate([r[2] for r in res])
        return np.concatenate([r[1] for r in res])


class FaissRetriever(BaseFaissIPRetriever):
    """index_factory ANN retriever of the reference (index.py:47-54).  Never called by
    the reference's scripts and out of scope here: importable, but building
    one raises instead of silently degrading to brute force."""

    def __init__(self, init_reps: np.ndarray, factory_str: str):
        raise NotImplementedError("FaissRetriever (faiss.index_factory ANN) is not part of the MI355X hot path; "
                                  "use BaseFaissIPRetriever (exact) instead")


def BM25Retriever(*args, **kwargs):  # noqa: N802 - keeps the reference's importable name (sampler.py:5)
    """Sparse BM25 negative mining is CPU data prep, out of scope; the
    reference's own implementation should be used for it."""
    raise NotImplementedError("BM25Retriever is out of scope for the MI355X build (CPU negative mining)")

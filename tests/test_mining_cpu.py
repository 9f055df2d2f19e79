"""CPU: the boundary of dense hard-negative mining -- the two C entries (declared, exported, shape limits
rejected before any HIP call), the torch op schemas and fake kernels, the exclusion CSR, the depth rule, the
passage pool and the retriever's ``exclude=`` argument.  No GPU compute.
Reference flow replaced: BM25Negatives.load_passages, DRT/trainer/sampler.py:57-99."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO


def test_entries_declared_and_exported():
    from denseretrievaltoolkits_amd import _native
    hdr = open(os.path.join(REPO, "include", "drt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _native.load()
    for name in ("drt_topk_exclude", "drt_pair_scores_bf16"):
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} not declared in include/drt.h"
        assert name in _native.EXPORTED and hasattr(lib, name)
    # each comment cites the reference site it replaces and states the exactness rule
    assert "sampler.py:69-80" in hdr and "K >= skip + m + |E_q|" in hdr


@pytest.mark.parametrize("k_in,skip,k_out", [(0, 0, 1), (32769, 0, 1), (10, 0, 0), (10, -1, 1)])
def test_topk_exclude_rejects_bad_shapes_without_gpu(k_in, skip, k_out):
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    rc = lib.drt_topk_exclude(None, None, 4, k_in, None, None, None, skip, k_out, None, None, None, None)
    assert rc == _native.DRT_EINVAL


def test_pair_scores_rejects_bad_d_without_gpu():
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    for d in (0, 12, 1032):
        assert lib.drt_pair_scores_bf16(None, 4, None, 10, d, None, None, 3, None, None) == _native.DRT_EINVAL


def test_op_schemas_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    assert str(drt.topk_exclude.default._schema) == (
        "drt::topk_exclude(Tensor scores, Tensor ids, Tensor excl, Tensor excl_off, Tensor? ceiling, int skip, "
        "int k_out) -> (Tensor, Tensor, Tensor)")
    assert str(drt.pair_scores.default._schema) == "drt::pair_scores(Tensor q, Tensor p, Tensor qidx, Tensor rows) -> Tensor"
    for device in ("meta", "cuda"):   # meta tensors, and FakeTensors standing for GPU ones
        with FakeTensorMode() if device == "cuda" else torch.device("meta"):
            s = torch.empty(7, 300, device=device)
            i = torch.empty(7, 300, dtype=torch.int64, device=device)
            ex = torch.empty(11, dtype=torch.int64, device=device)
            off = torch.empty(8, dtype=torch.int64, device=device)
            ce = torch.empty(7, device=device)
            for ceiling in (None, ce):
                os_, oi, cnt = drt.topk_exclude(s, i, ex, off, ceiling, 3, 20)
                assert (os_.shape, os_.dtype) == ((7, 20), torch.float32)
                assert (oi.shape, oi.dtype) == ((7, 20), torch.int64)
                assert (cnt.shape, cnt.dtype) == ((7,), torch.int32)
            q = torch.empty(7, 64, dtype=torch.bfloat16, device=device)
            p = torch.empty(100, 64, dtype=torch.bfloat16, device=device)
            out = drt.pair_scores(q, p, torch.empty(13, dtype=torch.int32, device=device),
                                  torch.empty(13, dtype=torch.int64, device=device))
            assert (out.shape, out.dtype) == ((13,), torch.float32)


def test_build_exclusions_sorts_and_dedups():
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    big = 1 << 33
    excl, off = build_exclusions([[5, 1, 5, 3], [], [big + 2, 7, big + 2], (), np.array([9])])
    assert excl.dtype == torch.int64 and off.dtype == torch.int64
    assert off.tolist() == [0, 3, 3, 5, 5, 6]
    assert excl.tolist() == [1, 3, 5, 7, big + 2, 9]
    excl, off = build_exclusions([[], []])
    assert excl.numel() == 0 and off.tolist() == [0, 0, 0]
    excl, off = build_exclusions([])
    assert excl.numel() == 0 and off.tolist() == [0]


def test_depth_rule():
    from denseretrievaltoolkits_amd import kernels, search
    from denseretrievaltoolkits_amd.trainer.mining import build_exclusions
    assert kernels.filtered_depth(10, 0, 0) == 10
    assert kernels.filtered_depth(32, 5, 4) == 41
    assert kernels.filtered_depth(kernels.MAX_K_LARGE - 3, 1, 2) == kernels.MAX_K_LARGE
    with pytest.raises(ValueError, match=str(kernels.MAX_K_LARGE)):
        kernels.filtered_depth(kernels.MAX_K_LARGE - 3, 2, 2)
    with pytest.raises(ValueError):
        kernels.filtered_depth(0, 0, 0)
    with pytest.raises(ValueError):
        kernels.filtered_depth(5, -1, 0)
    # the index layer's form: the longest segment counts, a deeper request wins, the corpus size caps
    _, off = build_exclusions([[1, 2, 3], [], [4]])
    assert search.filtered_depth(10, 2, off, 1_000_000) == 15
    assert search.filtered_depth(10, 2, off, 1_000_000, depth=64) == 64
    assert search.filtered_depth(10, 2, off, 12) == 12
    assert search.filtered_depth(2040, 0, build_exclusions([list(range(20))])[1], 5000) == 2060
    with pytest.raises(ValueError, match=str(kernels.MAX_K_LARGE)):
        search.filtered_depth(kernels.MAX_K_LARGE, 0, off, 1_000_000)
    with pytest.raises(ValueError, match=str(kernels.MAX_K_LARGE)):
        search.filtered_depth(10, 0, off, 1_000_000, depth=kernels.MAX_K_LARGE + 1)


def test_passage_pool_merges_identical_token_lists():
    from denseretrievaltoolkits_amd.trainer.mining import pool_passages
    corpus = [{"query": [1], "positives": [[5, 6, 7]], "negatives": [[8, 9], [10]]},
              {"query": [2], "positives": [[8, 9], [11]], "negatives": [[5, 6, 7], [10], [12, 13]]}]
    passages, pos_rows = pool_passages(corpus)
    assert passages == [[5, 6, 7], [8, 9], [10], [11], [12, 13]]
    assert pos_rows == [[0], [1, 3]]


def test_retriever_accepts_exclude_and_overlay_serves_mining():
    from denseretrievaltoolkits_amd import drt_overlay
    from denseretrievaltoolkits_amd.evaluator.index import BaseFaissIPRetriever
    from denseretrievaltoolkits_amd.search import FlatIPIndex, ShardedFlatIP
    for fn in (BaseFaissIPRetriever.search, BaseFaissIPRetriever.batch_search):
        assert inspect.signature(fn).parameters["exclude"].default is None
    for cls in (FlatIPIndex, ShardedFlatIP):
        sig = inspect.signature(cls.search_filtered_batches_iter)
        assert list(sig.parameters)[:5] == ["self", "batches", "k", "excl", "excl_off"]
        assert sig.parameters["skip"].default == 0 and sig.parameters["ceiling"].default is None
        assert sig.parameters["to_host"].default is False
        assert hasattr(cls, "search_filtered_device") and hasattr(cls, "pair_scores")
    assert drt_overlay.HOT_PATH_MODULES["DRT.trainer.mining"] == "denseretrievaltoolkits_amd.trainer.mining"
    from denseretrievaltoolkits_amd.trainer import mining
    sig = inspect.signature(mining.mine_negatives)
    assert list(sig.parameters)[:4] == ["index", "q_reps", "positives", "num_negatives"]

"""Argument checks of the five filter entry points (no GPU): every return that happens before the first
HIP call -- DRT_EINVAL for dimensions, offsets and the per-entry arguments, DRT_OK for an empty query
set -- with all device pointers null."""
import ctypes

import pytest

NQ, N, NG, D, K, OFF = 4, 1000, 8000, 128, 10, 3000


def _lib():
    from denseretrievaltoolkits_amd import _native
    return _native, _native.load()


def _starts(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _call(lib, entry, nq=NQ, n=N, ng=NG, d=D, k=K, off=OFF, starts=None, nchunks=None, npasses=8, nlists=1,
          stride=None):
    """One call with null device pointers; the entry's own arguments default to valid values."""
    head = (None, nq, None, n, ng, d, k, off)
    if entry == "filter":
        return lib.drt_ip_topk_dist_filter(*head, None, None, None, 0, None)
    if entry == "chunks":
        st = _starts(0, n) if starts is None else starts
        nc = len(st) - 1 if nchunks is None else nchunks
        return lib.drt_ip_topk_dist_filter_chunks(*head, None, None, st, nc, None, 0, None)
    if entry == "passes":
        return lib.drt_ip_topk_filter_passes(*head, None, None, npasses, -1, None, None, None, 0, None)
    if entry == "lists":
        return lib.drt_ip_topk_dist_filter_lists(*head, None, nlists, None, None, None, 0, None)
    assert entry == "lists_at"
    r = lib.drt_ip_topk_sample_rank(k)
    return lib.drt_ip_topk_dist_filter_lists_at(*head, None, nlists, nq * r if stride is None else stride, None, None,
                                                None, 0, None)


ENTRIES = ["filter", "chunks", "passes", "lists", "lists_at"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("bad", [
    dict(d=100),                     # d % 64 != 0
    dict(n=1000, ng=999),            # n_global < n_local
    dict(n=1000, ng=8000, off=7001),  # id_offset + n_local > n_global
    dict(k=0),
    dict(k=2049),
])
def test_shared_dimension_checks(entry, bad):
    native, lib = _lib()
    assert _call(lib, entry, **bad) == native.DRT_EINVAL


@pytest.mark.parametrize("bad", [
    dict(d=832),
    dict(nchunks=0),
    dict(starts=_starts(1, N)),            # starts[0] != 0
    dict(starts=_starts(0, 500, N - 1)),   # starts[nchunks] != n_local
    dict(starts=_starts(0, 600, 500, N)),  # decreasing
])
def test_chunks_checks(bad):
    native, lib = _lib()
    assert _call(lib, "chunks", **bad) == native.DRT_EINVAL
    assert _call(lib, "chunks", nq=0, **bad) == native.DRT_EINVAL   # checked before the empty-set return


@pytest.mark.parametrize("bad", [dict(d=832), dict(npasses=0), dict(npasses=1025)])
def test_passes_checks(bad):
    native, lib = _lib()
    assert _call(lib, "passes", **bad) == native.DRT_EINVAL
    assert _call(lib, "passes", nq=0, **bad) == native.DRT_EINVAL


def test_lists_checks():
    native, lib = _lib()
    r = lib.drt_ip_topk_sample_rank(K)
    assert 0 < r <= 4096
    too_many = 4096 // r + 1
    for entry in ("lists", "lists_at"):
        assert _call(lib, entry, nlists=0) == native.DRT_EINVAL
        assert _call(lib, entry, nlists=too_many) == native.DRT_EINVAL
        assert _call(lib, entry, nq=0, nlists=0) == native.DRT_EINVAL
    assert _call(lib, "lists_at", nlists=2, stride=NQ * r - 1) == native.DRT_EINVAL
    # one list: the stride is not read
    assert _call(lib, "lists_at", nq=0, nlists=1, stride=0) == native.DRT_OK


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", [N, 0])
def test_empty_query_set_returns_ok_with_null_pointers(entry, n):
    native, lib = _lib()
    assert _call(lib, entry, nq=0, n=n) == native.DRT_OK

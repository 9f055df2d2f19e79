"""GPU: drt_topk_exclude (csrc/exclude.hip) against a numpy restatement on synthetic sorted lists.

The kernel is a stable compaction of a canonical top-k list -- the device form of the skip loop of
BM25Negatives.load_passages (DRT/trainer/sampler.py:69-80).  It is called through the C ABI into output
buffers pre-filled with garbage (an unwritten slot shows) and through torch.ops.drt.topk_exclude; ids,
scores and counts must equal the restatement exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD_S = np.float32(-3.402823466e+38)
LDS_IDS = 4096                                  # kExclLds (csrc/exclude.hip): longer segments are searched in HBM
SEG_LENS = [0, 1, 40, LDS_IDS, LDS_IDS + 1]


def restate(scores, ids, segs, ceiling, skip, k_out):
    nq = scores.shape[0]
    os_ = np.full((nq, k_out), PAD_S, np.float32)
    oi = np.full((nq, k_out), -1, np.int64)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        keep = (ids[q] >= 0) & ~np.isin(ids[q], segs[q])
        if ceiling is not None:
            keep &= scores[q] < ceiling[q]
        j = np.nonzero(keep)[0]
        cnt[q] = j.size
        j = j[skip: skip + k_out]
        os_[q, : j.size] = scores[q, j]
        oi[q, : j.size] = ids[q, j]
    return os_, oi, cnt


def make_lists(rng, nq, k_in, id_base=0, n_pad=0):
    """[nq, k_in] lists in (score desc, id asc) order with many exact score ties; the last n_pad entries pads."""
    space = 4 * k_in + 20000
    ids = np.stack([rng.choice(space, size=k_in, replace=False) for _ in range(nq)]).astype(np.int64) + id_base
    scores = rng.integers(-40, 41, size=(nq, k_in)).astype(np.float32) / 4
    for q in range(nq):
        o = np.lexsort((ids[q], -scores[q]))
        ids[q], scores[q] = ids[q][o], scores[q][o]
    if n_pad:
        ids[:, k_in - n_pad:] = -1
        scores[:, k_in - n_pad:] = PAD_S
    return scores, ids, space


def make_segment(rng, ids_q, length, space, id_base=0):
    """A sorted exclusion segment of exactly ``length`` ids: about half taken from the list (hits), the rest
    drawn with replacement from the id space (absent ids, duplicates)."""
    if length == 0:
        return np.zeros(0, np.int64)
    real = ids_q[ids_q >= 0]
    h = min(real.size, (length + 1) // 2)
    hits = rng.choice(real, size=h, replace=False) if h else np.zeros(0, np.int64)
    other = rng.integers(0, space, size=length - h).astype(np.int64) + id_base
    return np.sort(np.concatenate([hits, other]))


def csr(segs):
    off = np.zeros(len(segs) + 1, np.int64)
    off[1:] = np.cumsum([s.size for s in segs])
    return (np.concatenate(segs) if segs else np.zeros(0, np.int64)).astype(np.int64), off


def run_both(dev, scores, ids, segs, ceiling, skip, k_out):
    """The C entry into garbage-filled buffers and the torch op; both must agree.  Host arrays back."""
    import torch
    from denseretrievaltoolkits_amd import _native, ops
    lib = _native.load()
    nq, k_in = scores.shape
    excl, off = csr(segs)
    s_d, i_d = torch.from_numpy(scores).to(dev), torch.from_numpy(ids).to(dev)
    e_d, o_d = torch.from_numpy(excl).to(dev), torch.from_numpy(off).to(dev)
    c_d = None if ceiling is None else torch.from_numpy(np.asarray(ceiling, np.float32)).to(dev)
    os_ = torch.full((nq, k_out), 12345.0, dtype=torch.float32, device=dev)
    oi = torch.full((nq, k_out), 777, dtype=torch.int64, device=dev)
    cnt = torch.full((nq,), -9, dtype=torch.int32, device=dev)
    rc = lib.drt_topk_exclude(s_d.data_ptr(), i_d.data_ptr(), nq, k_in, e_d.data_ptr() if excl.size else None,
                              o_d.data_ptr(), None if c_d is None else c_d.data_ptr(), skip, k_out, os_.data_ptr(),
                              oi.data_ptr(), cnt.data_ptr(), _native.stream_ptr(dev))
    assert rc == 0
    ts, ti, tc = ops.load().topk_exclude(s_d, i_d, e_d, o_d, c_d, skip, k_out)
    torch.cuda.synchronize()
    assert torch.equal(ts, os_) and torch.equal(ti, oi) and torch.equal(tc, cnt)
    return os_.cpu().numpy(), oi.cpu().numpy(), cnt.cpu().numpy()


def check(dev, scores, ids, segs, ceiling, skip, k_out):
    got = run_both(dev, scores, ids, segs, ceiling, skip, k_out)
    want = restate(scores, ids, segs, ceiling, skip, k_out)
    for g, w, name in zip(got, want, ("scores", "ids", "count")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return want


@pytest.mark.parametrize("nq,k_in,k_out,skip", [(1, 1, 1, 0), (3, 63, 10, 0), (5, 64, 64, 0), (5, 65, 20, 5),
                                                (130, 257, 100, 7), (2, 2049, 2048, 0), (2, 5000, 300, 100)])
def test_shapes_and_segment_lengths(dev, nq, k_in, k_out, skip):
    """Every shape with every segment length (0, 1, 40, one on each side of the LDS staging limit): query q of
    round r takes SEG_LENS[(r + q) % 5], enough rounds that every length occurs."""
    rng = np.random.default_rng(1000 * nq + k_in)
    for r in range(0, len(SEG_LENS), min(nq, len(SEG_LENS))):
        scores, ids, space = make_lists(rng, nq, k_in)
        segs = [make_segment(rng, ids[q], SEG_LENS[(r + q) % len(SEG_LENS)], space) for q in range(nq)]
        check(dev, scores, ids, segs, None, skip, k_out)


def test_identity_at_the_largest_list(dev):
    """(1, 32768, 32768, 0) with nothing excluded: the output is the input."""
    rng = np.random.default_rng(3)
    scores, ids, _ = make_lists(rng, 1, 32768)
    os_, oi, cnt = run_both(dev, scores, ids, [np.zeros(0, np.int64)], None, 0, 32768)
    np.testing.assert_array_equal(oi, ids)
    np.testing.assert_array_equal(os_, scores)
    assert cnt.tolist() == [32768]


def test_everything_excluded_and_pads_in_the_tail(dev):
    rng = np.random.default_rng(4)
    scores, ids, space = make_lists(rng, 4, 300, n_pad=37)
    # every real entry excluded: all pads, count 0
    os_, oi, cnt = check(dev, scores, ids, [np.sort(ids[q][ids[q] >= 0]) for q in range(4)], None, 0, 50)
    assert (oi == -1).all() and (os_ == PAD_S).all() and (cnt == 0).all()
    # the input's pads are never kept: count = real entries minus the excluded ones
    segs = [make_segment(rng, ids[q], 40, space) for q in range(4)]
    _, oi, cnt = check(dev, scores, ids, segs, None, 0, 300)
    assert (cnt <= 300 - 37).all() and (oi[:, -37:] == -1).all()


def test_ids_beyond_32_bits(dev):
    """Ids offset by 2^33 (a sharded index's global ids): the comparison is on all 64 bits -- an excluded id
    that differs from a listed one only above bit 32 must not match."""
    rng = np.random.default_rng(5)
    base = 1 << 33
    scores, ids, space = make_lists(rng, 3, 500, id_base=base)
    segs = []
    for q in range(3):
        low = ids[q][:50] - base                      # the same low words without the offset: absent
        segs.append(np.sort(np.concatenate([make_segment(rng, ids[q], 40, space, id_base=base), low])))
    _, _, cnt = check(dev, scores, ids, segs, None, 2, 200)
    assert (cnt >= 500 - 40).all()


def test_ceiling(dev):
    rng = np.random.default_rng(6)
    scores, ids, space = make_lists(rng, 6, 400)
    segs = [make_segment(rng, ids[q], [0, 1, 40][q % 3], space) for q in range(6)]
    inf = np.float32(np.inf)
    _, _, cnt = check(dev, scores, ids, segs, np.full(6, inf, np.float32), 0, 400)      # +inf: no effect
    assert (cnt >= 400 - 40).all()
    _, oi, cnt = check(dev, scores, ids, segs, np.full(6, -inf, np.float32), 0, 30)     # -inf: nothing passes
    assert (cnt == 0).all() and (oi == -1).all()
    # a mid value that coincides exactly with some scores: strict <, the tied entries go too
    mid = scores[:, 150].copy()
    assert all((scores[q] == mid[q]).sum() > 1 for q in range(6))
    _, _, cnt = check(dev, scores, ids, segs, mid, 3, 100)
    assert all(cnt[q] <= (scores[q] < mid[q]).sum() for q in range(6))
    mixed = np.array([inf, -inf, mid[2], mid[3], inf, -inf], np.float32)                 # per-query ceilings
    check(dev, scores, ids, segs, mixed, 0, 64)


def test_skip_and_k_out_beyond_the_survivors(dev):
    rng = np.random.default_rng(7)
    scores, ids, space = make_lists(rng, 3, 100, n_pad=10)
    segs = [make_segment(rng, ids[q], 40, space) for q in range(3)]
    kept = restate(scores, ids, segs, None, 0, 1)[2]
    _, oi, _ = check(dev, scores, ids, segs, None, int(kept.max()), 16)        # skip >= kept: all pads
    assert (oi == -1).all()
    check(dev, scores, ids, segs, None, int(kept.min()) - 1, 16)               # one survivor left for some query
    _, oi, _ = check(dev, scores, ids, segs, None, 0, 1000)                    # k_out > kept (and > k_in)
    assert all((oi[q] >= 0).sum() == kept[q] for q in range(3))


def test_op_argument_checks(dev):
    import torch
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    s = torch.zeros(2, 8, device=dev)
    i = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    off = torch.zeros(3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="nq \\+ 1"):
        drt.topk_exclude(s, i, e, off[:2], None, 0, 4)
    with pytest.raises(ValueError):
        drt.topk_exclude(s, i.int(), e, off, None, 0, 4)
    with pytest.raises(ValueError):
        drt.topk_exclude(s, i, e, off, None, -1, 4)
    with pytest.raises(ValueError):
        drt.topk_exclude(s, i, e, off, None, 0, 0)
    with pytest.raises(ValueError):
        drt.topk_exclude(s, i, e, off, torch.zeros(3, device=dev), 0, 4)
    with pytest.raises(ValueError):
        drt.topk_exclude(torch.zeros(1, 32769, device=dev), torch.zeros(1, 32769, dtype=torch.int64, device=dev), e,
                         off[:2], None, 0, 4)


def test_opcheck_both_ops(dev):
    import torch
    from helpers import int_bf16, to_dev_bf16
    from denseretrievaltoolkits_amd import ops
    drt = ops.load()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic")
    rng = np.random.default_rng(8)
    scores, ids, space = make_lists(rng, 4, 90)
    excl, off = csr([make_segment(rng, ids[q], 7, space) for q in range(4)])
    args = [torch.from_numpy(x).to(dev) for x in (scores, ids, excl, off)]
    torch.library.opcheck(drt.topk_exclude.default, (*args, None, 2, 30), test_utils=utils)
    torch.library.opcheck(drt.topk_exclude.default, (*args, torch.from_numpy(scores[:, 20].copy()).to(dev), 0, 30),
                          test_utils=utils)
    q = to_dev_bf16(int_bf16(rng, (4, 64), -3, 3), dev)
    p = to_dev_bf16(int_bf16(rng, (50, 64), -3, 3), dev)
    torch.library.opcheck(drt.pair_scores.default,
                          (q, p, torch.tensor([0, 3, 1], dtype=torch.int32, device=dev),
                           torch.tensor([49, 0, -1], dtype=torch.int64, device=dev)), test_utils=utils)

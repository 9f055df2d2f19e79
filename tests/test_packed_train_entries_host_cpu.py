"""The refusal table of the four varlen training entries (forward / backward, whole-sequence / streamed),
no GPU: one checked constructor per direction states their argument checks once, so one table probes all
four -- DRT_EINVAL before any HIP call, the shape and probability checks before the DRT_OK of an empty
input, the pointer / L_pad / W checks after it -- and each entry's own length bound, which the Python
constants of model/train_tower.py must equal."""
import pytest

P = 0x1000   # a non-null "device pointer": the checks under test return before anything reads it

# entry -> (its length bound, the defaults of a well-formed call: max_len, L_pad, T, W)
ENTRIES = {
    "drt_attention_varlen_train_forward_bf16": (160, dict(max_len=64, L_pad=64, T=100, W=2)),
    "drt_attention_varlen_backward_bf16": (160, dict(max_len=64, L_pad=64, T=100, W=2)),
    "drt_attention_varlen_long_train_forward_bf16": (512, dict(max_len=300, L_pad=320, T=700, W=10)),
    "drt_attention_varlen_long_backward_bf16": (512, dict(max_len=300, L_pad=320, T=700, W=10)),
}


def _call(lib, name, n=3, max_len=None, L_pad=None, T=None, W=None, hd=64, p=0.0, ptr=None, heads=12, table=P):
    d = ENTRIES[name][1]
    max_len, L_pad = d["max_len"] if max_len is None else max_len, d["L_pad"] if L_pad is None else L_pad
    T, W = d["T"] if T is None else T, d["W"] if W is None else W
    fn = getattr(lib, name)
    if "forward" in name:
        return fn(ptr, ptr, None, n, max_len, L_pad, T, W, ptr, ptr, ptr, heads, hd, 0.125, p, 1, 2, None)
    ids = table if "long" in name else None    # the tile table, or no sequence list
    return fn(ptr, ptr, ptr, ptr, ptr, ids, n, max_len, L_pad, T, W, ptr, ptr, ptr, heads, hd, 0.125, p, 1, 2, None)


# (case, arguments as a function of the entry's bound M and default max_len D, accepted?)
CASES = [
    ("over_the_bound", lambda M, D: dict(max_len=M + 1, L_pad=M + 1), False),
    ("max_len_0", lambda M, D: dict(max_len=0), False),
    ("head_dim_32", lambda M, D: dict(hd=32), False),
    ("p_1", lambda M, D: dict(p=1.0), False),
    ("p_negative", lambda M, D: dict(p=-0.1), False),
    ("heads_0", lambda M, D: dict(heads=0), False),
    ("n_negative", lambda M, D: dict(n=-1), False),
    ("null_tensors_with_work", lambda M, D: dict(), False),
    ("L_pad_below_max_len", lambda M, D: dict(ptr=P, L_pad=D - 1), False),
    ("keep_words_too_few", lambda M, D: dict(ptr=P, p=0.1, W=(D + 31) // 32 - 1), False),
    ("empty_n", lambda M, D: dict(n=0), True),
    ("empty_T", lambda M, D: dict(T=0), True),
    # the shape checks come before the empty-input return, so n = 0 probes the bound with no launch
    ("empty_over_the_bound_default_pad", lambda M, D: dict(n=0, max_len=M + 1), False),
    ("empty_at_the_bound", lambda M, D: dict(n=0, max_len=M, L_pad=M, W=(M + 31) // 32), True),
    ("empty_over_the_bound", lambda M, D: dict(n=0, max_len=M + 1, L_pad=M + 1, W=(M + 32) // 32), False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_refusal_table(name, case):
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    M, d = ENTRIES[name]
    _, kw, ok = case
    assert _call(lib, name, **kw(M, d["max_len"])) == (_native.DRT_OK if ok else _native.DRT_EINVAL)


def test_long_backward_needs_its_tile_table_only_with_work():
    from denseretrievaltoolkits_amd import _native
    lib, name = _native.load(), "drt_attention_varlen_long_backward_bf16"
    assert _call(lib, name, ptr=P, table=None) == _native.DRT_EINVAL
    assert _call(lib, name, n=0, table=None) == _native.DRT_OK


def test_long_forward_takes_a_whole_sequence_class():
    """max_len <= 160 goes to the short entry, with that entry's checks."""
    from denseretrievaltoolkits_amd import _native
    lib, name = _native.load(), "drt_attention_varlen_long_train_forward_bf16"
    assert _call(lib, name, n=0, max_len=160, L_pad=160, W=5) == _native.DRT_OK
    assert _call(lib, name, max_len=64, L_pad=64, W=2) == _native.DRT_EINVAL          # null tensors with work
    assert _call(lib, name, n=0, max_len=64, p=1.0) == _native.DRT_EINVAL


def test_python_bounds_are_the_entries_bounds():
    from denseretrievaltoolkits_amd.model import packing, train_tower
    assert train_tower.MAX_PACKED_TRAIN_LEN == packing._SHORT_MAX == 160 == 32 * packing._CLASS_MAX_BLOCKS
    assert train_tower.MAX_PACKED_TRAIN_LONG_LEN == 512
    assert {M for M, _ in ENTRIES.values()} == {train_tower.MAX_PACKED_TRAIN_LEN, train_tower.MAX_PACKED_TRAIN_LONG_LEN}

"""Host-side argument checks of the MiniLM-class entries (no device work): the head_dim-32 attention
pair refuses each bad argument with DRT_EINVAL and accepts an empty input; the four inference row
entries take H = 384 next to the multiples of 256 and still refuse 700 and 1280."""
import pytest

P = 4096   # a non-null, 16-byte aligned address: every call below returns before it is read


def test_hd32_attention_argument_checks():
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    fwd, var = lib.drt_attention_hd32_forward_bf16, lib.drt_attention_hd32_varlen_forward_bf16
    bad = [fwd(P, None, P, 2, 64, heads, 0.17, None) for heads in (11, 0, -2)]
    bad += [fwd(P, None, P, 2, L, 12, 0.17, None) for L in (0, 513, -1)]
    bad += [fwd(None, None, P, 2, 64, 12, 0.17, None), fwd(P, None, None, 2, 64, 12, 0.17, None),
            fwd(P + 8, None, P, 2, 64, 12, 0.17, None), fwd(P, None, P, -1, 64, 12, 0.17, None)]
    bad += [var(P, P, None, 2, 64, P, heads, 0.17, None) for heads in (11, 0)]
    bad += [var(P, P, None, 2, ml, P, 12, 0.17, None) for ml in (0, 513)]
    bad += [var(None, P, None, 2, 64, P, 12, 0.17, None), var(P, None, None, 2, 64, P, 12, 0.17, None),
            var(P, P, None, 2, 64, None, 12, 0.17, None), var(P, P, None, -1, 64, P, 12, 0.17, None)]
    assert bad == [_native.DRT_EINVAL] * len(bad)
    assert fwd(None, None, None, 0, 64, 12, 0.17, None) == _native.DRT_OK
    assert var(None, None, None, 0, 64, None, 12, 0.17, None) == _native.DRT_OK


@pytest.mark.parametrize("H,want", [(384, 0), (768, 0), (700, -1), (1280, -1)])
def test_row_entries_widths(H, want):
    """Empty inputs: the shape checks run, nothing is launched."""
    from denseretrievaltoolkits_amd import _native
    lib = _native.load()
    assert lib.drt_embed_ln(None, None, 0, 8, None, None, None, None, None, 1e-12, H, None, None) == want
    assert lib.drt_embed_ln_packed(None, None, None, 0, 8, 0, None, None, None, None, None, 1e-12, H, None, None) == want
    assert lib.drt_layernorm_bf16(None, 0, H, None, None, 1e-12, None, None) == want
    assert lib.drt_layernorm_f32_bf16(None, 0, H, None, None, 1e-12, None, None) == want
    # the training forms keep their widths
    pre = lib.drt_embed_ln_pre(None, None, 0, 8, None, None, None, None, None, 1e-12, H, None, None, None)
    assert pre == (want if H != 384 else _native.DRT_EINVAL)

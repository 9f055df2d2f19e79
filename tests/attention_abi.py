"""The one place the tests spell the ctypes calls of the attention pair (include/drt.h,
"Attention"): tensors in, the entry's status code out.  Callers wrap the code in ``_native.check``,
or assert it where the test is about a refusal.  head_dim is 64; the stream is the current one of
``qkv``'s device.
"""


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    from denseretrievaltoolkits_amd import _native
    return _native.stream_ptr(t.device)


def forward(lib, qkv, ctx, B, L, heads, *, mask=None, relbias=None, lse=None, bits=None, scale, drop=(0.0, 0, 0)):
    """drt_attention_forward_bf16 into ``ctx`` (and ``lse`` / ``bits`` when given); drop = (p, seed, site)."""
    p, seed, site = drop
    return lib.drt_attention_forward_bf16(qkv.data_ptr(), _ptr(mask), _ptr(relbias), ctx.data_ptr(), _ptr(lse),
                                          _ptr(bits), B, L, heads, 64, scale, p, seed, site, _stream(qkv))


def backward(lib, qkv, ctx, dctx, lse, dqkv, B, L, heads, *, mask=None, relbias=None, bits=None, scale,
             drop=(0.0, 0, 0), dbias=None, dtable=None, ws=None, ws_bytes=0):
    """drt_attention_backward_bf16 into ``dqkv`` (and ``dbias`` / ``dtable`` when given, through ``ws`` of
    ``ws_bytes`` = drt_attention_backward_workspace bytes)."""
    p, seed, site = drop
    return lib.drt_attention_backward_bf16(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), _ptr(mask),
                                           _ptr(relbias), _ptr(bits), dqkv.data_ptr(), B, L, heads, 64, scale, p, seed,
                                           site, _ptr(dbias), _ptr(dtable), _ptr(ws), ws_bytes, _stream(qkv))

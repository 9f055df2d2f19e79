"""The two shape gates of model/encoder.py, message by message (no device work): the training tower's
``_check_supported`` and the inference encoder's ``_check_inference_supported``, which adds hidden 384 at
head_dim 32.  The texts are what a caller sees and are pinned as they stand."""
import pytest

from denseretrievaltoolkits_amd.model.encoder import BertShape, _check_inference_supported, _check_supported

ERF_ONLY = "only erf GELU ('gelu') is implemented"
INTERMEDIATE = "intermediate size must be a multiple of 64"
GATES = [_check_supported, _check_inference_supported]


def bert(**kw):
    return BertShape(**{**dict(hidden=768, layers=2, heads=12, intermediate=3072, eps=1e-12, act="gelu"), **kw})


def minilm(**kw):
    return bert(**{**dict(hidden=384, intermediate=1536), **kw})


def refusal(gate, shape):
    with pytest.raises(ValueError) as e:
        gate(shape)
    return str(e.value)


@pytest.mark.parametrize("gate", GATES)
def test_supported_shapes_pass(gate):
    gate(bert())
    gate(bert(hidden=1024, heads=16, intermediate=4096))


@pytest.mark.parametrize("gate", GATES)
def test_activation_messages(gate):
    """Two texts: an activation that is no GELU at all, and the tanh GELU."""
    assert refusal(gate, bert(act="relu")) == "activation relu unsupported (erf GELU only)"
    assert refusal(gate, bert(act="gelu_pytorch_tanh")) == "activation gelu_pytorch_tanh unsupported (erf GELU only)"
    assert refusal(gate, bert(act="gelu_new")) == ERF_ONLY


@pytest.mark.parametrize("gate", GATES)
def test_shape_messages(gate):
    assert refusal(gate, bert(hidden=640, heads=10)) == "hidden size 640 unsupported (multiple of 256, <= 1024)"
    assert refusal(gate, bert(hidden=1280, heads=20)) == "hidden size 1280 unsupported (multiple of 256, <= 1024)"
    assert refusal(gate, bert(heads=6)) == "head_dim must be 64"
    assert refusal(gate, bert(intermediate=3000)) == INTERMEDIATE
    # the order of the tests: intermediate size before activation
    assert refusal(gate, bert(intermediate=3000, act="relu")) == INTERMEDIATE


def test_minilm_inference_only():
    _check_inference_supported(minilm())
    assert refusal(_check_supported, minilm()) == "hidden size 384 unsupported (multiple of 256, <= 1024)"


def test_minilm_messages():
    gate = _check_inference_supported
    assert refusal(gate, minilm(act="relu")) == ERF_ONLY
    assert refusal(gate, minilm(act="gelu_new")) == ERF_ONLY
    assert refusal(gate, minilm(intermediate=1500)) == INTERMEDIATE
    assert refusal(gate, minilm(intermediate=1500, act="relu")) == INTERMEDIATE
    # any other head count at 384 (head_dim 64 or 48) falls to the training tower's gate and its message
    assert refusal(gate, minilm(heads=6)) == "hidden size 384 unsupported (multiple of 256, <= 1024)"
    assert refusal(gate, minilm(heads=8)) == "hidden size 384 unsupported (multiple of 256, <= 1024)"

"""basd_gemm_bf16_act: the QuickGELU and tanh-GELU epilogues of csrc/gemm_bf16.hip in all four kernel families (GPU
box only).  One shape per family from tests/_gemm_cases.py -- the smallest that reaches each epilogue with a ragged last
row block -- and that module's ``random_inputs``.

The bound, per element, in the form tests/test_gemm_schedule_gpu.py derives for the plain epilogues:

    |y - act(z)| <= 2^-8 |act(z)| + L (K + 2) 2^-24 S + c 2^-24 max(1, |z|)

z = x w^T + b and act(z) in fp64 from the same bf16 inputs, S = |x| |w|^T + |b|.
  * first term: the single rounding to bf16;
  * second term: the fp32 accumulation error of z, (K + 2) 2^-24 S, carried through the activation, whose slope is at
    most L = 1.10 (QuickGELU, at z ~ 1.8) or 1.13 (tanh-GELU, at z ~ 1.4);
  * third term: the activation's own evaluation in fp32.  The kernel computes z * rcp(1 + exp2(-s log2 e)) with s the
    sigmoid's argument (1.702 z, or 2 sqrt(2/pi) (z + 0.044715 z^3)); v_exp_f32 and v_rcp_f32 are documented to 1 ulp
    = 2 units of 2^-24 each, the sum 1 + e and the final product round to 1 unit each, and the argument's own roundings
    (<= 5 units relative in s) move the result by |z| sigma (1 - sigma) |s| <= 0.3 times that: 2 + 2 + 1 + 1 + 1.5 < 8
    units of 2^-24 relative to |z| sigma <= max(1, |z|).  c = 8.
"""
import math

import pytest
import torch

from tests import _gemm_cases as C

pytestmark = pytest.mark.gpu

SHAPES = {(257, 256, 64): "nt128", (255, 192, 64): "nt192", (8193, 1024, 64): "ring", (5889, 3072, 192): "pring"}
SLOPE = {2: 1.10, 3: 1.13}
C_EVAL = 8.0
TAIL = 8
BASD_ERR_SHAPE = 1


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    _INPUTS.clear()


_INPUTS = {}


def _inputs(shape):
    """(x, w, b, z, S): the bf16 inputs on the device and the fp64 pre-activation / magnitude sums WITHOUT the bias;
    built once per shape and shared, never modified"""
    if shape not in _INPUTS:
        x, w, b, _ = (t.cuda() for t in C.random_inputs(*shape))
        wt = w.double().t().contiguous()
        _INPUTS[shape] = (x, w, b, x.double() @ wt, x.double().abs() @ wt.abs())
    return _INPUTS[shape]


def _sentinel(M, N):
    return torch.full((M + TAIL, N), C.SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _act_gemm(nat, x, w, b, act, tile_run=0):
    M, (N, K) = x.shape[0], w.shape
    y = _sentinel(M, N)
    rc = nat.lib().basd_gemm_bf16_act(nat._ptr(x), nat._ptr(w), nat._ptr(b), nat._ptr(y), M, N, K, act, tile_run,
                                      nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    assert bool((y[M:].view(torch.int16) == C.SENTINEL).all()), "rows behind M were written"
    return y[:M]


def _act64(z, act):
    if act == 2:
        return z / (1.0 + torch.exp(-1.702 * z))
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def _ratio(y, z, S, act, K):
    ref = _act64(z, act)
    err = (y.double() - ref).abs()
    bound = (2.0 ** -8 * ref.abs() + SLOPE[act] * (K + 2) * 2.0 ** -24 * S
             + C_EVAL * 2.0 ** -24 * z.abs().clamp_min(1.0))
    assert bool(torch.isfinite(y.float()).all()), "non-finite output"
    return float((err / bound).max())


def test_shapes_still_reach_their_kernel_family():
    for shape, family in SHAPES.items():
        assert C.dispatch(*shape) == family, shape
        assert shape[0] % C.GBM != 0                                  # a ragged last row block


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", [2, 3], ids=["quick_gelu", "gelu_tanh"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=C.case_id)
def test_activation_epilogues_against_fp64(nat, shape, act, with_bias):
    """every element within the derived bound; the output buffer has 8 sentinel rows behind M that must survive.
    Largest error / bound ratios measured on an MI355X: profiles/gemm_act_margins.txt."""
    x, w, b, z, S = _inputs(shape)
    y = _act_gemm(nat, x, w, b if with_bias else None, act)
    if with_bias:
        z, S = z + b.double(), S + b.double().abs()
    ratio = _ratio(y, z, S, act, shape[2])
    print(f"gemm-act-bound {C.case_id(shape)} {SHAPES[shape]} act {act} {'bias' if with_bias else 'nobias'} "
          f"ratio {ratio:.4f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("shape", list(SHAPES), ids=C.case_id)
def test_act_0_and_1_are_the_existing_epilogues_bit_for_bit(nat, shape):
    x, w, b, _, _ = _inputs(shape)
    M, N, K = shape
    L = nat.lib()
    for act, epilogue, bias in ((1, 2, b), (0, 1, b), (0, 0, None), (1, 2, None)):
        want = _sentinel(M, N)
        rc = L.basd_gemm_bf16(nat._ptr(x), nat._ptr(w), nat._ptr(bias), nat._ptr(want), M, N, K, epilogue, 0,
                              nat._stream())
        assert rc == 0, L.basd_last_error()
        got = _act_gemm(nat, x, w, bias, act)
        assert torch.equal(got.view(torch.int16), want[:M].view(torch.int16)), (act, epilogue, bias is None)


@pytest.mark.parametrize("act", [4, -1, 7, 6])
def test_unknown_activation_is_refused_before_the_launch(nat, act):
    shape = (257, 256, 64)
    x, w, b, _, _ = _inputs(shape)
    y = _sentinel(shape[0], shape[1])
    rc = nat.lib().basd_gemm_bf16_act(nat._ptr(x), nat._ptr(w), nat._ptr(b), nat._ptr(y), *shape, act, 0, nat._stream())
    torch.cuda.synchronize()
    assert rc == BASD_ERR_SHAPE and b"act" in nat.lib().basd_last_error()
    assert bool((y.view(torch.int16) == C.SENTINEL).all()), "a refused call wrote to y"


def test_basd_gemm_bf16_still_refuses_epilogues_above_2(nat):
    shape = (257, 256, 64)
    x, w, b, _, _ = _inputs(shape)
    y = _sentinel(shape[0], shape[1])
    for epilogue in (3, 6, 7):
        rc = nat.lib().basd_gemm_bf16(nat._ptr(x), nat._ptr(w), nat._ptr(b), nat._ptr(y), *shape, epilogue, 0,
                                      nat._stream())
        assert rc == BASD_ERR_SHAPE, epilogue


@pytest.mark.parametrize("act", [2, 3], ids=["quick_gelu", "gelu_tanh"])
@pytest.mark.parametrize("shape", [(257, 256, 64), (5889, 3072, 192)], ids=C.case_id)
def test_large_preactivations_saturate_without_overflow(nat, shape, act):
    """x scaled by 32 (exact in bf16): pre-activations beyond +-60 on both sides, where exp2 of the sigmoid's argument
    overflows to +inf (negative z: the result must be -0 or a tiny negative, not NaN) or underflows to 0 (positive z:
    the result is z).  Finite everywhere and within the same bound (both the LDS-staged and the direct epilogue)."""
    x, w, b, z, S = _inputs(shape)
    z, S = 32.0 * z + b.double(), 32.0 * S + b.double().abs()
    assert float(z.max()) >= 60.0 and float(z.min()) <= -60.0
    y = _act_gemm(nat, (x.float() * 32.0).bfloat16(), w, b, act)
    ratio = _ratio(y, z, S, act, shape[2])
    far = z <= -60.0
    print(f"gemm-act-bound-large {C.case_id(shape)} {SHAPES[shape]} act {act} ratio {ratio:.4f} "
          f"max |y| where z <= -60: {float(y[far].float().abs().max()):.3g}")
    assert ratio <= 1.0, ratio
    assert float(y[far].float().abs().max()) <= 1e-30
    assert bool((y[z >= 60.0].float() > 0).all())


def test_wrapper_names_the_activations(nat):
    shape = (257, 256, 64)
    x, w, b, _, _ = _inputs(shape)
    assert torch.equal(nat.gemm_bf16(x, w, b, act="gelu"), nat.gemm_bf16(x, w, b, gelu=True))
    assert torch.equal(nat.gemm_bf16(x, w, b, act="quick_gelu"), _act_gemm(nat, x, w, b, 2))
    assert torch.equal(nat.gemm_bf16(x, w, b, act="gelu_tanh"), _act_gemm(nat, x, w, b, 3))
    with pytest.raises(nat.BasdNativeError):
        nat.gemm_bf16(x, w, b, act="swish")

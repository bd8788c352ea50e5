"""The short attention backward (csrc/attention_bwd.hip, basd_attention_bwd_bf16: hd 64, T <= 224) at the pair and tile
edges of both of its instances: T <= 96 (three key pairs, one per wave of a 4-wave workgroup) and T > 96 (seven, one
per wave of an 8-wave workgroup, the eighth wave idle; waves whose pair holds no token skip the work).

Inputs: qkv ~ N(0, 1) bf16, out and lse from basd_attention_fwd_bf16, dO ~ N(0, 1) bf16.  Reference: fp64 autograd of
the plain softmax attention on the same bf16 inputs.  dQ, dK and dV are compared per slice in relative L2 against the
cap the project already has for this kernel family (tests/_attn_regimes.py::CAP_SHORT).  At T = 1 the reference's dQ and
dK are exactly zero (the softmax of one logit is constant), so a relative error over the result has no meaning there:
those two slices are measured over the magnitude of the computation, scale (P o (|dP| + |delta|)) |K| (resp. |Q|), the
denominator tests/_attn_regimes.py::bwd_a_ref defines for cancelling dS, against the same cap.

B = 3 and H in {1, 3}: the smallest that exercise the batch / head indexing and make the padding rows of one image
border the next image's real rows."""
import ctypes

import pytest
import torch

from tests import _attn_regimes as R

pytestmark = pytest.mark.gpu

HD = 64
SCALE = HD ** -0.5
B = 3
T_NP3 = [1, 16, 31, 32, 33, 64, 65, 96]
T_NP7 = [97, 128, 161, 192, 193, 197, 223, 224]
SENTINEL = 0x7FA5                  # a bf16 NaN no arithmetic produces: "still there" = never written, "finite" = written
GUARD = 4                          # token rows in front of and behind dqkv


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


def _inputs(T, H, salt=0):
    g = torch.Generator().manual_seed((T * 131 + H) * 31 + 7919 * salt)
    qkv = torch.randn(B, T, 3 * H * HD, generator=g).to(torch.bfloat16).cuda()
    dout = torch.randn(B, T, H * HD, generator=g).to(torch.bfloat16).cuda()
    return qkv, dout


def _fwd(nat, qkv, H):
    T = qkv.shape[1]
    out = torch.empty(B, T, H * HD, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    nat._check(nat.lib().basd_attention_fwd_bf16(nat._ptr(qkv), B, T, H, HD, ctypes.c_float(SCALE), nat._ptr(out),
                                                 nat._ptr(None), nat._ptr(lse), nat._stream()), "fwd")
    return out, lse


def _bwd_guarded(nat, qkv, out, dout, lse, H):
    """-> (dqkv [B, T, 3 H hd], the guard rows in front, the guard rows behind): a fresh sentinel-filled buffer"""
    T = qkv.shape[1]
    row = 3 * H * HD
    buf = torch.full(((B * T + 2 * GUARD) * row,), SENTINEL, dtype=torch.int16, device="cuda")
    inner = buf[GUARD * row:(GUARD + B * T) * row]
    nat._check(nat.lib().basd_attention_bwd_bf16(nat._ptr(qkv), nat._ptr(out), nat._ptr(dout), nat._ptr(lse), B, T, H,
                                                 HD, ctypes.c_float(SCALE), nat._ptr(inner), nat._stream()), "bwd")
    torch.cuda.synchronize()
    return inner.view(torch.bfloat16).reshape(B, T, row), buf[:GUARD * row], buf[(GUARD + B * T) * row:]


_CASES = {}


def _case(nat, T, H):
    """inputs, forward results, the kernel's dqkv (with its guards) and the fp64 reference of one shape, computed once"""
    if (T, H) not in _CASES:
        qkv, dout = _inputs(T, H)
        out, lse = _fwd(nat, qkv, H)
        dqkv, front, back = _bwd_guarded(nat, qkv, out, dout, lse, H)
        ref = R.bwd_autograd(qkv, dout, H, HD, SCALE)
        _CASES[(T, H)] = dict(qkv=qkv, dout=dout, out=out, lse=lse, dqkv=dqkv, front=front, back=back, ref=ref)
    return _CASES[(T, H)]


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("T", T_NP3 + T_NP7)
def test_matches_fp64_autograd(nat, T, H):
    c = _case(nat, T, H)
    assert bool(torch.isfinite(c["dqkv"].float()).all())
    got = R.dqkv_parts(c["dqkv"], H, HD)
    mag = None
    for name, g, want in zip(("dq", "dk", "dv"), got, c["ref"]):
        den = want
        if float(want.norm()) == 0.0:
            assert T == 1 and name in ("dq", "dk"), (name, T)
            if mag is None:
                mag = R.bwd_a_ref(c["qkv"], c["out"], c["dout"], H, HD, SCALE)[3:]
            den = mag[0] if name == "dq" else mag[1]
        err = R.rel(g, want, den)
        print(f"T {T} H {H} {name}: rel L2 {err:.3e}")
        assert err < R.CAP_SHORT, (name, T, H, err)


@pytest.mark.parametrize("T", [197, 33])
@pytest.mark.parametrize("H", [1, 3])
def test_guard_rows_untouched_and_every_element_written(nat, T, H):
    c = _case(nat, T, H)
    assert bool((c["front"] == SENTINEL).all()), "wrote in front of dqkv"
    assert bool((c["back"] == SENTINEL).all()), "wrote behind dqkv"
    # the buffer was all sentinel NaN: finite everywhere = every element was written
    assert bool(torch.isfinite(c["dqkv"].float()).all())


def test_two_launches_are_bitwise_equal(nat):
    c = _case(nat, 197, 3)
    again, _, _ = _bwd_guarded(nat, c["qkv"], c["out"], c["dout"], c["lse"], 3)
    assert torch.equal(again.view(torch.int16), c["dqkv"].view(torch.int16))


@pytest.mark.parametrize("T", [197, 65])
def test_gradient_of_an_image_does_not_depend_on_the_next(nat, T):
    """a padded query or key row that read across the image boundary would see image b + 1's tokens"""
    H = 3
    c = _case(nat, T, H)
    other, other_dout = _inputs(T, H, salt=1)
    for b in range(B - 1):
        qkv, dout = c["qkv"].clone(), c["dout"].clone()
        qkv[b + 1], dout[b + 1] = other[b + 1], other_dout[b + 1]
        out, lse = _fwd(nat, qkv, H)
        assert torch.equal(out[b].view(torch.int16), c["out"][b].view(torch.int16))
        dqkv, _, _ = _bwd_guarded(nat, qkv, out, dout, lse, H)
        assert torch.equal(dqkv[b].view(torch.int16), c["dqkv"][b].view(torch.int16)), b
        assert not torch.equal(dqkv[b + 1].view(torch.int16), c["dqkv"][b + 1].view(torch.int16))

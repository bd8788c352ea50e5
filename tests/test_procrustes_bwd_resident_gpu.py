"""basd_procrustes_bwd_side on the resident kernel (csrc/procrustes_bwd.hip, procrustes_bwd_side_resident_kernel: the
factor's bf16 planes stay in LDS for all column groups, a workgroup owns a row tile of one matrix) and on both sides of
its dispatch boundary, against fp64.

Yardstick (tests/test_procrustes_bwd_long_gpu.py): the kernel and the CPU restatement of the contract
(tests/_pbwd_emul.py) compute the same three bf16 products with fp32 accumulation and may differ in the order of the
fp32 additions only, so the kernel's error against fp64 has to stay within 2x the restatement's on the same tensors:
rel-L2 and max-abs over max |want|, of `out` and of `rowdot`.  Every test prints its figures before it asserts."""
import ctypes

import pytest
import torch

from tests import _pbwd_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


def _side(nat, fac, w, a, gl, out, rowdot):
    batch, n, d = w.shape
    code = nat.DTYPE_F32 if out.dtype == torch.float32 else nat.DTYPE_BF16
    p = ctypes.c_void_p
    rc = nat.lib().basd_procrustes_bwd_side(p(fac.data_ptr()), p(w.data_ptr()), p(a.data_ptr()), p(gl.data_ptr()), batch, n,
                                            d, p(out.data_ptr()), code, p(rowdot.data_ptr()), nat._stream())
    nat._check(rc, "basd_procrustes_bwd_side")


def _guarded(x, guard=4096):
    """x on the device as the exact-size head of an allocation whose next `guard` elements are NaN: a read past the end
    that is not masked shows up in the result"""
    buf = torch.full((x.numel() + guard,), float("nan"), dtype=x.dtype, device="cuda")
    buf[:x.numel()] = x.reshape(-1).cuda()
    return buf[:x.numel()].view(x.shape)


def _run(nat, inputs, bf16):
    fac, w, a, gl = (_guarded(x) for x in inputs)
    batch, n, d = w.shape
    out = torch.empty(batch, n, d, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    rowdot = torch.empty(batch, n, device="cuda")
    _side(nat, fac, w, a, gl, out, rowdot)
    torch.cuda.synchronize()
    return out, rowdot


def _check(label, got, want, emul):
    out, rowdot = got
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(rowdot).all())
    kern = C.errors(out, rowdot, want)
    print(f"\n{label}: " + "; ".join(f"{k} kernel {kern[k]:.3e} emulation {emul[k]:.3e} ratio {kern[k] / emul[k]:.3f}"
                                      for k in kern))
    for k in kern:
        assert kern[k] <= 2.0 * emul[k], (label, k, kern[k], emul[k])


@pytest.mark.parametrize("batch,n,d,bf16", C.CASES)
def test_side_against_fp64_within_twice_the_emulation(nat, batch, n, d, bf16):
    inputs, want, emul = C.case("white", batch, n, d, bf16)
    _check(f"white batch={batch} n={n} d={d} {'bf16' if bf16 else 'fp32'}", _run(nat, inputs, bf16), want, emul)


@pytest.mark.parametrize("bf16", [False, True])
def test_trained_network_statistics_at_196_tokens(nat, bf16):
    inputs, want, emul = C.case("trained", 2, 196, 768, bf16)
    _check(f"trained n=196 d=768 {'bf16' if bf16 else 'fp32'}", _run(nat, inputs, bf16), want, emul)


@pytest.mark.parametrize("bf16", [False, True])
def test_two_calls_are_bitwise_equal(nat, bf16):
    inputs, _, _ = C.case("white", 3, 196, 768, True)
    first, second = _run(nat, inputs, bf16), _run(nat, inputs, bf16)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


@pytest.mark.parametrize("bf16", [False, True])
def test_nothing_is_stored_outside_the_outputs(nat, bf16):
    """n = 100, d = 112: a row tail of 12 in the seventh m tile, a K tail of 4, a ragged column group.  `out` and
    `rowdot` sit between guard bands of a sentinel in one allocation each; the bands keep it, every element between
    them is written."""
    batch, n, d, guard = 2, 100, 112, 64
    inputs, want, emul = C.case("white", batch, n, d, bf16)
    fac, w, a, gl = (_guarded(x) for x in inputs)
    out_all = torch.full((batch * n + 2 * guard, d), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32,
                         device="cuda")
    dot_all = torch.full((batch * n + 2 * guard,), float("nan"), device="cuda")
    out, rowdot = out_all[guard:guard + batch * n].view(batch, n, d), dot_all[guard:guard + batch * n].view(batch, n)
    _side(nat, fac, w, a, gl, out, rowdot)
    torch.cuda.synchronize()
    for band in (out_all[:guard], out_all[guard + batch * n:], dot_all[:guard], dot_all[guard + batch * n:]):
        assert bool(torch.isnan(band.float()).all())
    _check(f"guarded n={n} d={d}", (out, rowdot), want, emul)

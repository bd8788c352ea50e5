"""The yardstick of tests/test_procrustes_bwd_resident_gpu.py on a CPU-only machine: the restatement of the contract
(tests/_pbwd_emul.py) against fp64 at the GPU tests' constructions (tests/_pbwd_cases.py), its own errors printed, and
the bound that follows from the number formats asserted."""
import pytest
import torch

from tests import _pbwd_cases as C
from tests import _pbwd_emul


def _format_bound(fac, w, a, gl, want_out):
    """hi keeps 8 significant bits and mid the next 8, so |x - hi - mid| <= 2^-18 |x|: the three kept products miss a
    term of fac W by at most 3 x 2^-18 |fac| |W| (the third 2^-18 is the dropped mid x mid), and K = n fp32 additions
    add sqrt(K) 2^-23 |fac| |W| at most.  Per row in the Frobenius norm, scaled like the output; the element-wise
    fp32 epilogue adds 4 ulp of the result."""
    n = fac.shape[-1]
    unit = 3 * 2.0 ** -18 + n ** 0.5 * 2.0 ** -23
    rows = unit * (fac.double().abs() @ w.double().abs()).norm(dim=-1)
    c = (2.0 * gl.double()).abs().view(-1, 1) * a.double().sqrt()
    return float((c * rows).norm()) + 4 * 2.0 ** -24 * float(want_out.norm())


@pytest.mark.parametrize("batch,n,d,bf16", [c for c in C.CASES if not c[3] and c[0] <= 3])
def test_emulation_within_the_format_bound(batch, n, d, bf16):
    (fac, w, a, gl), want, emul = C.case("white", batch, n, d, bf16)
    out, _ = _pbwd_emul.procrustes_bwd_side(fac, w, a, gl)
    err, bound = float((out.double() - want[0]).norm()), _format_bound(fac, w, a, gl, want[0])
    print(f"\nemulation vs fp64, white batch={batch} n={n} d={d}: " + "; ".join(f"{k} {v:.3e}" for k, v in emul.items()) +
          f"; bound {bound / float(want[0].norm()):.3e}")
    assert 0.0 < err <= bound, (err, bound)


def test_trained_construction_does_what_it_says_and_stays_within_the_bound():
    (fac, w, a, gl), want, emul = C.case("trained", 2, 196, 768, False)
    assert float(a.sort(dim=-1, descending=True).values[:, :196 // 20].sum(-1).min()) > 0.89
    r = w.double() - fac.double() @ w.double()
    ratio = r.norm(dim=-1) / w.double().norm(dim=-1)
    assert int((ratio < 0.1).sum()) >= 2 * 24 and float(ratio.max()) > 0.5
    assert float(w.abs().max()) > 90.0
    out, _ = _pbwd_emul.procrustes_bwd_side(fac, w, a, gl)
    err, bound = float((out.double() - want[0]).norm()), _format_bound(fac, w, a, gl, want[0])
    print("\nemulation vs fp64, trained n=196 d=768: " + "; ".join(f"{k} {v:.3e}" for k, v in emul.items()) +
          f"; bound {bound / float(want[0].norm()):.3e}")
    assert 0.0 < err <= bound, (err, bound)


def test_bf16_output_is_one_rounding_of_the_fp32_output():
    (fac, w, a, gl), want, emul = C.case("white", 3, 196, 768, True)
    o32, d32 = _pbwd_emul.procrustes_bwd_side(fac, w, a, gl)
    o16, d16 = _pbwd_emul.procrustes_bwd_side(fac, w, a, gl, torch.bfloat16)
    assert torch.equal(o32.to(torch.bfloat16), o16) and torch.equal(d32, d16)
    assert emul["out"] < 2.0 ** -8

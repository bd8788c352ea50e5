"""basd_sym_tridiag_f64 and basd_tridiag_mp_rank (csrc/tridiag.hip) against the numpy restatement of
tests/_tridiag_cases.py, which tests/test_tridiag_cases_cpu.py checks against ``numpy.linalg.eigvalsh`` and the oracle.

The reduction: the eigenvalues of the returned (diag, off), taken by numpy on the host, lie within Householder's
backward error bound 4 n eps64 lambda_max of those of the input Gram; two runs agree bit for bit (every reduction has
a fixed order, no floating-point atomics); reflectors of already-reduced columns are the identity.  The input matrix
is documented as scratch.  The count: rank and status word equal the restatement's."""
import numpy as np
import pytest
import torch

from tests import _tridiag_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native_provider():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    native.lib()
    _ops.set_ops(None)
    native.status_word("cuda").zero_()
    yield
    native.status_word("cuda").zero_()


def _gram_of_order(n: int) -> np.ndarray:
    """fp64 Gram [n, n] of planted fp32 tokens with a few more rows than columns"""
    return C.gram64(C.planted_tokens(n + 40 + n // 4, n, max(1, n // 32)))


def _reduce(a: np.ndarray):
    import basd_amd._native as native
    diag, off = native.sym_tridiag(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return diag.cpu().numpy(), off.cpu().numpy()


@pytest.mark.parametrize("n", C.TRIDIAG_SIZES)
def test_reduction_keeps_the_spectrum_and_repeats_bitwise(n):
    a = _gram_of_order(n)
    lam = np.linalg.eigvalsh(a)
    diag, off = _reduce(a)
    assert diag.shape == (n,) and off.shape == (n - 1,)
    got = np.linalg.eigvalsh(C.tridiag_dense(diag, off))
    err = float(np.abs(got - lam).max())
    unit = n * C.EPS64 * float(lam.max())
    print(f"sym_tridiag n={n}: max eigenvalue error {err / unit:.4f} n eps lambda_max")
    assert err <= 4 * unit
    diag2, off2 = _reduce(a)
    assert diag.tobytes() == diag2.tobytes() and off.tobytes() == off2.tobytes()


def test_identity_reflectors_for_reduced_columns():
    """an exactly zero trailing block and a 3 x 3 diagonal matrix: tau = 0, no update, zeros come back as zeros"""
    diag, off = _reduce(np.diag([3.0, 1.0, 2.0]))
    assert diag.tolist() == [3.0, 1.0, 2.0] and off.tolist() == [0.0, 0.0]
    g = _gram_of_order(65)
    a = np.zeros((100, 100))
    a[:65, :65] = g
    diag, off = _reduce(a)
    assert not diag[65:].any() and not off[64:].any()
    lam = np.linalg.eigvalsh(g)
    got = np.linalg.eigvalsh(C.tridiag_dense(diag[:65], off[:64]))
    assert float(np.abs(got - lam).max()) <= 4 * 65 * C.EPS64 * float(lam.max())


def test_nonfinite_input_propagates():
    a = _gram_of_order(64)
    a[40, 3] = a[3, 40] = np.nan
    diag, off = _reduce(a)
    assert np.isnan(diag).any() or np.isnan(off).any()


def _count(diag, off, rows, d, cap):
    import basd_amd._native as native
    word = native.status_word("cuda")
    word.zero_()
    rank = native.tridiag_mp_rank(torch.from_numpy(np.ascontiguousarray(diag)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(off)).cuda(), rows, d, cap)
    out = int(rank.item()), int(word.item())
    word.zero_()
    return out


@pytest.mark.parametrize("m,d,r", C.CPU_CASES)
def test_count_on_the_restated_tridiagonals(m, d, r):
    _x, g, lam = C.case(m, d, r)
    n = g.shape[0]
    want, gap = C.direct_mp_rank(lam, m, d)
    assert gap >= C.GAP
    diag, off = C.householder_tridiag(g)
    assert C.counted_mp_rank(diag, off, m, d, n) == (want, 0)
    assert _count(diag, off, m, d, n) == (want, 0)
    assert _count(diag, off, m, d, 1) == (min(1, want), 0)            # cap


def test_count_on_handmade_tridiagonals():
    for name, (diag, off, rows, d) in C.handmade().items():
        want = C.counted_mp_rank(diag, off, rows, d, diag.size)
        assert _count(diag, off, rows, d, diag.size) == want, name
    diag, off, rows, d = C.handmade()["diagonal: 5 above the edge"]
    assert _count(diag, off, rows, d, 40) == (5, 0)
    assert _count(diag, off, rows, d, 3) == (3, 0)
    assert _count(*C.handmade()["identity"], 16) == (0, C.STATUS_RANK0)
    assert _count(*C.handmade()["one NaN"], 16) == (0, C.STATUS_NONFINITE)


def test_count_at_full_order():
    """2048 values: every LDS slot in use, eight full strides of the loading loop"""
    rng = np.random.default_rng(2048)
    diag = np.concatenate((rng.uniform(0.5, 1.5, 2000), rng.uniform(40.0, 90.0, 48)))
    off = rng.uniform(-0.05, 0.05, 2047)
    want, gap = C.direct_mp_rank(np.linalg.eigvalsh(C.tridiag_dense(diag, off)), 20480, 2048)
    assert gap >= C.GAP and want == 48
    assert _count(diag, off, 20480, 2048, 2048) == (want, 0)

"""The restatement and inputs of tests/test_tridiag_gpu.py / tests/test_mp_rank_wide_gpu.py are fit to judge the
eigenvalue-counting Marchenko-Pastur rank with (no GPU needed).

tests/_tridiag_cases.py restates the Householder reduction, the guarded Sturm count and the counted rank in numpy.
Here: the reduction keeps the spectrum within Householder's backward error bound, 4 n eps ||A||; the counted rank is the
direct count on ``numpy.linalg.eigvalsh`` and the oracle's, on inputs whose edge is clear of every eigenvalue; the three
C entries refuse bad shapes before anything is launched; and the start-up routing between the two rank functions."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _tridiag_cases as C


@pytest.mark.parametrize("m,d,r", C.CPU_CASES)
def test_restated_reduction_keeps_the_spectrum(m, d, r):
    """bound: c n eps ||A|| with c = 4 (Householder's backward error); the restatement measures 0.008 .. 0.36 of
    n eps lambda_max on these inputs"""
    _x, g, lam = C.case(m, d, r)
    n = g.shape[0]
    diag, off = C.householder_tridiag(g)
    got = np.linalg.eigvalsh(C.tridiag_dense(diag, off))
    err = float(np.abs(got - lam).max())
    unit = n * C.EPS64 * float(lam.max())
    print(f"tridiag-ref ({m}, {d}, {r}): n={n} max eigenvalue error {err / unit:.4f} n eps lambda_max")
    assert err <= 4 * unit


@pytest.mark.parametrize("m,d,r", C.CPU_CASES)
def test_restated_rank_is_the_direct_count_and_the_oracles(m, d, r):
    from oracle import basd_oracle as O
    x, g, lam = C.case(m, d, r)
    want, gap = C.direct_mp_rank(lam, m, d)
    print(f"tridiag-ref ({m}, {d}, {r}): rank {want}, nearest eigenvalue {gap:.2e} (relative) from the edge")
    assert gap >= C.GAP                                     # on the reference spectrum alone
    diag, off = C.householder_tridiag(g)
    rank, status = C.counted_mp_rank(diag, off, m, d, g.shape[0])
    assert (rank, status) == (want, 0)
    assert rank == O.mp_rank(x.double())
    assert C.counted_mp_rank(diag, off, m, d, 1) == (min(1, want), 0)          # cap


def test_sturm_counts_against_the_spectrum():
    _x, g, lam = C.case(400, 64, 6)
    diag, off = C.householder_tridiag(g)
    mids = 0.5 * (lam[1:] + lam[:-1])
    pivmin = C.TINY64 * max(1.0, float((off ** 2).max()))
    assert C.sturm_counts(diag, off, mids, pivmin).tolist() == list(range(1, 64))
    assert C.sturm_counts(diag, off, [lam[0] - 1.0, lam[-1] + 1.0], pivmin).tolist() == [0, 64]


def test_handmade_tridiagonals_have_the_rank_and_status_they_name():
    h = C.handmade()
    for name, (diag, off, rows, d) in h.items():
        rank, status = C.counted_mp_rank(diag, off, rows, d, diag.size)
        if np.isfinite(diag).all() and np.isfinite(off).all():
            want, gap = C.direct_mp_rank(np.linalg.eigvalsh(C.tridiag_dense(diag, off)), rows, d)
            assert gap >= C.GAP, name
            assert rank == want, name
            assert status == (C.STATUS_RANK0 if want == 0 else 0), name
        else:
            assert (rank, status) == (0, C.STATUS_NONFINITE), name
    assert C.counted_mp_rank(*h["diagonal: 5 above the edge"], 40)[0] == 5
    assert C.counted_mp_rank(*h["off = 0 in the middle"], 32)[0] == 12
    assert C.counted_mp_rank(*h["identity"], 16) == (0, C.STATUS_RANK0)


def test_tau_zero_columns_pass_through():
    """a zero trailing block and a diagonal matrix: every reflector is the identity"""
    diag, off = C.householder_tridiag(np.diag([3.0, 1.0, 2.0]))
    assert diag.tolist() == [3.0, 1.0, 2.0] and off.tolist() == [0.0, 0.0]
    _x, g, _lam = C.case(400, 64, 6)
    a = np.zeros((12, 12))
    a[:7, :7] = g[:7, :7]
    diag, off = C.householder_tridiag(a)
    assert not diag[7:].any() and not off[6:].any()
    np.testing.assert_allclose(np.linalg.eigvalsh(C.tridiag_dense(diag, off))[5:], np.linalg.eigvalsh(g[:7, :7]),
                               rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------------
# refusals: every check below returns before a kernel is launched, so no GPU is needed
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def entries():
    import basd_amd._native as native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


_NULL = ctypes.c_void_p(0)
BASD_OK, BASD_ERR_SHAPE = 0, 1


def _host(n, dtype):
    """a host buffer behind a fake pointer: nothing may be read or written through it"""
    t = torch.full((n,), -7, dtype=dtype)
    return t, ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", [-1, 0, 1, 2049, 4096])
def test_entries_refuse_orders_outside_2_to_2048(entries, n):
    t, p = _host(64, torch.float64)
    r, pr = _host(4, torch.int32)
    assert entries.basd_sym_tridiag_f64(p, n, p, p, p, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_last_error() == f"sym_tridiag_f64: n={n} outside 2 .. 2048".encode()
    assert entries.basd_tridiag_mp_rank(p, p, n, 100000, 4096, 4096, pr, pr, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_last_error() == f"tridiag_mp_rank: n={n} outside 2 .. 2048".encode()
    assert bool((t == -7).all()) and bool((r == -7).all())


@pytest.mark.parametrize("n,rows,d", [(64, 63, 64), (64, 64, 63), (1280, 16896, 1279), (2048, 2047, 4096), (2, 0, 2)])
def test_count_refuses_more_values_than_the_smaller_side(entries, n, rows, d):
    t, p = _host(64, torch.float64)
    r, pr = _host(4, torch.int32)
    assert entries.basd_tridiag_mp_rank(p, p, n, rows, d, n, pr, pr, _NULL) == BASD_ERR_SHAPE
    assert b"not the smaller side" in entries.basd_last_error()
    assert bool((t == -7).all()) and bool((r == -7).all())


def test_workspace_is_positive_and_monotone(entries):
    sizes = [entries.basd_sym_tridiag_f64_workspace_bytes(n) for n in range(2, 2049)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 2 * 2048 * 8                       # a reflector and a product vector


# ------------------------------------------------------------------------------------------------------------------
# start-up routing
# ------------------------------------------------------------------------------------------------------------------
def test_route_between_the_two_rank_functions():
    from basd_amd.losses import mp_rank_route
    from basd_amd.losses.functional import BasdShapeError
    for m, d in ((5000, 1024), (784, 2048), (4096, 192), (300, 384)):
        assert mp_rank_route(m, d) == "spectrum"
    for m, d in ((16896, 1280), (20482, 2048), (1100, 1536), (2048, 4096), (1025, 1025)):
        assert mp_rank_route(m, d) == "counted"
    with pytest.raises(BasdShapeError, match="2048"):
        mp_rank_route(2049, 2049)


def test_wide_rank_is_exported_and_names_its_limit():
    import basd_amd.losses as L
    from basd_amd.losses.functional import BasdShapeError
    assert callable(L.marchenko_pastur_rank_wide)
    assert "marchenko_pastur_rank_wide" in L.marchenko_pastur_rank.__doc__
    from tests import _emul
    from basd_amd.losses import _ops
    _ops.set_ops(_emul)                                    # the shape check comes before any kernel
    try:
        for m, d in ((2049, 2049), (1, 7), (5000, 1)):
            with pytest.raises(BasdShapeError, match="2048"):
                L.marchenko_pastur_rank_wide(torch.zeros(m, d))
    finally:
        _ops.set_ops(None)

"""The references and inputs of tests/test_factor_chain_gpu.py are fit to judge a kernel with (no GPU needed).

tests/_factor_cases.py holds plain numpy references of the pivoted Cholesky, the inverse of its factor and the
Marchenko-Pastur rank, in fp64 and in long double.  Here: the references against independent ones (torch, the oracle,
the definition); for every case of the tables, the same pivot order and rank in fp64 and in long double with a top-two
gap that rounding cannot close; eigenvalues clear of their Marchenko-Pastur edge; the size lists on the dispatch paths
they are there for; and the entries' refusals, which return before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _factor_cases as C


def test_long_double_is_wider_than_fp64():
    assert np.finfo(np.longdouble).eps < 1e-18


# ------------------------------------------------------------------------------------------------------------------
# the size lists reach the paths they name
# ------------------------------------------------------------------------------------------------------------------
def test_sizes_cover_every_dispatch_path():
    for kernel, sizes in C.PCHOL_SIZES.items():
        assert {C.pchol_kernel_of(n) for n in sizes} == {kernel}
    assert C.pchol_kernel_of(192) != C.pchol_kernel_of(193) and C.pchol_kernel_of(196) != C.pchol_kernel_of(197)
    ns = {n for n, _r, _ld in C.PCHOL_RANDOM}
    assert ns == {n for sizes in C.PCHOL_SIZES.values() for n in sizes}
    for kernel, sizes in C.PCHOL_SIZES.items():
        ranks = [(n, r) for n, r, _ld in C.PCHOL_RANDOM if n in sizes]
        assert any(r == n for n, r in ranks) and any(r == n - 1 for n, r in ranks) and any(r <= 8 < n for n, r in ranks)
    assert any(ld > C.jacobi_ld(n) for n, _r, ld in C.PCHOL_RANDOM) and all(n <= ld <= 320 for n, _r, ld in C.PCHOL_RANDOM)
    assert {C.pchol_kernel_of(n) for n in C.EXACT_SIZES} == set(C.PCHOL_SIZES)
    assert {C.pchol_kernel_of(n) for n in C.SPECTRUM_SIZES} == set(C.PCHOL_SIZES)
    # the inverse: a padded last block (n % 16 != 0) below 193, the one-row border, both ends of the border range
    assert {C.trinv_path_of(n) for n in C.TRINV_SIZES} == {"blocked", "blocked+border"}
    assert [n for n in C.TRINV_SIZES if n <= 192 and n % 16] == [1, 15, 17, 100, 191]
    assert {193, 208} <= set(C.TRINV_SIZES)
    assert {(196, 192), (208, 192), (196, 193), (208, 200), (193, 192), (193, 193), (192, 0)} <= set(C.TRINV_CASES)
    assert {C.mp_rank_threads(n) for n in C.MP_SIZES} == {256, 1024}
    assert C.mp_rank_threads(256) == 256 and C.mp_rank_threads(257) == 1024
    # the stride rule of the callers
    import basd_amd._native as native
    assert all(C.jacobi_ld(n) == native.jacobi_ld(n) for n in range(1, 321))


# ------------------------------------------------------------------------------------------------------------------
# pivoted Cholesky: the reference, and the pivot-order condition on every input
# ------------------------------------------------------------------------------------------------------------------
def _lower_chol_in_pivot_order(a, ref):
    """torch's Cholesky of P A P^T: unique, so ref.L[piv] must equal it"""
    p = ref.piv[:ref.rank]
    return torch.linalg.cholesky(torch.from_numpy(a[np.ix_(p, p)])).numpy()


@pytest.mark.parametrize("n,rank", [(7, 7), (64, 64), (65, 21), (196, 195)])
def test_ref_pchol_is_the_cholesky_factor_in_its_own_pivot_order(n, rank):
    a, r64, rld = C.pchol_random_case(n, rank)
    for m, f in zip(a, r64):
        assert f.rank == rank and sorted(f.piv.tolist()) == list(range(n))
        assert f.piv[rank:].tolist() == sorted(f.piv[rank:].tolist())
        lp = f.L[f.piv][:rank, :rank]
        assert float(np.abs(np.triu(lp, 1)).max(initial=0.0)) == 0.0
        assert bool((f.L[:, rank:] == 0).all())
        if rank == n:
            want = _lower_chol_in_pivot_order(m, f)
            assert float(np.abs(lp - want).max()) <= 1e-9 * float(np.sqrt(f.dmax0))
        # greedy: every pivot is the largest residual diagonal, so they descend
        assert bool((np.diff(f.pivots) <= 0).all()) and bool((f.gaps >= 0).all())


def test_ref_pchol_reads_the_lower_triangle_only_and_takes_dmax_ref():
    a = C.graded_psd(33, 33)[0]
    want = C.ref_pchol(a)
    up = a.copy()
    up[np.triu_indices(33, 1)] = np.nan
    got = C.ref_pchol(up)
    assert got.rank == want.rank and np.array_equal(got.L, want.L) and np.array_equal(got.piv, want.piv)
    big = C.ref_pchol(a, 1e-3, dmax_ref=float(want.dmax0) * 50)
    small = C.ref_pchol(a, 1e-3)
    assert big.rank < small.rank <= 33 and np.array_equal(big.L[:, :big.rank], small.L[:, :big.rank])
    assert big.rank == int((small.pivots > 1e-3 * 50 * small.dmax0).sum())


def test_one_per_kernel_inputs_have_their_rank():
    assert {C.pchol_kernel_of(n) for n, _r in C.ONE_PER_KERNEL} == set(C.PCHOL_SIZES)
    for n, rank in C.ONE_PER_KERNEL:
        for batch in (C.BATCH, 4):
            refs = [C.ref_pchol(m) for m in C.one_per_kernel_input(n, rank, batch)]
            assert [f.rank for f in refs] == [rank] * batch and all(C.stop_is_clear(f) for f in refs)


_FIGURES = []


@pytest.mark.parametrize("case", C.PCHOL_RANDOM, ids=C.case_id)
def test_random_cases_have_one_pivot_order_in_fp64_and_long_double(case):
    n, rank, _ld = case
    a, r64, rld = C.pchol_random_case(n, rank)
    worst_res = 0.0
    for m, f, l in zip(a, r64, rld):
        assert f.rank == l.rank == rank and C.stop_is_clear(l) and C.stop_is_clear(f)
        assert np.array_equal(f.piv, l.piv)
        steps = C.compared_steps(l)
        assert rank - steps <= rank // 10, (n, rank, steps)              # at most the last 10 % of the live steps
        assert float(l.gaps[:steps].min(initial=np.inf)) >= C.GAP_MIN, (n, rank, float(l.gaps[:steps].min()))
        # the fp64 reference inside the residual bound the kernels get
        res = float(np.abs(f.L.astype(np.longdouble) @ f.L.T.astype(np.longdouble) - np.tril(m) - np.tril(m, -1).T).max())
        assert res <= C.residual_bound(n, rank, l.dmax0), (n, rank, res)
        worst_res = max(worst_res, res / float(l.dmax0))
    e64 = C.factor_e64(r64, rld)
    gap = min(float(l.gaps[:C.compared_steps(l)].min(initial=np.inf)) for l in rld)
    _FIGURES.append(f"pchol n={n} rank={rank}: e64 {e64:.2e}, floor {C.factor_floor(max(l.dmax0 for l in rld)):.2e}, "
                    f"smallest gap {gap:.2e}, fp64 residual {worst_res:.2e} dmax0")


@pytest.mark.parametrize("kind", C.SPECTRUM_KINDS)
@pytest.mark.parametrize("n", C.SPECTRUM_SIZES)
def test_spectrum_cases_have_one_pivot_order_through_the_tolerance(n, kind):
    a, r64, rld = C.spectrum_case(n, kind)
    for f, l in zip(r64, rld):
        lo, hi = C.rank_at(l, 2 * C.TOL), C.rank_at(l, C.TOL / 2)
        assert hi == l.rank and lo <= C.rank_at(l, C.TOL) <= hi
        if kind == "gap":
            assert lo == hi == n // 2
        else:
            assert 1 <= hi - lo <= 12 and hi < n                       # pivots between tol / 2 and 2 tol: no gap there
        # every step a kernel may take has the same pivot in both, with a gap far above fp64's error at 1e-13 dmax0
        steps = min(f.rank, hi)
        assert steps >= lo and np.array_equal(f.piv[:steps], l.piv[:steps])
        assert float(l.gaps[:hi].min()) >= C.SPECTRUM_GAP_MIN
        assert sorted(l.piv[:hi].tolist()) != l.piv[:hi].tolist()       # a permuted order, not 0, 1, 2, ...


@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_exact_cases_are_exact_and_the_reference_breaks_ties_to_the_lowest_index(n):
    for name, d in C.exact_diagonals(n).items():
        assert bool(((d == 0) | (np.log2(np.where(d > 0, d, 1.0)) % 2 == 0)).all()), name      # even powers of two
        piv, rank, L = C.exact_expectation(d)
        for dtype in (np.float64, np.longdouble):
            ref = C.ref_pchol(np.diag(d), C.EXACT_TOL, dtype=dtype)
            assert ref.rank == rank and np.array_equal(ref.piv, piv) and np.array_equal(ref.L, L), name
        if name == "all-equal":
            assert piv.tolist() == list(range(n)) and rank == n
        if name == "zero":
            assert piv.tolist() == list(range(n)) and rank == 0
        if name == "runs" and n >= 194:
            # each run is taken front to back, across its boundary
            assert piv[:8].tolist() == [2, 3, 4, 5, 14, 15, 16, 17] and piv[20:24].tolist() == [190, 191, 192, 193]
    d = 2.0 ** -np.arange(n, dtype=np.float64)
    for dref in C.DMAX_REFS:
        want = int((d > C.DMAX_TOL * dref).sum())
        assert C.ref_pchol(np.diag(d), C.DMAX_TOL, dmax_ref=dref).rank == want
    assert [int((2.0 ** -np.arange(64.0) > C.DMAX_TOL * r).sum()) for r in C.DMAX_REFS] == [17, 25, 20]


# ------------------------------------------------------------------------------------------------------------------
# triangular inverse
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(17, 17), (100, 99), (196, 193), (208, 5), (16, 0)], ids=C.case_id)
def test_ref_trinv_against_solve_triangular(case):
    n, rank = case
    facs, xld, x64 = C.trinv_case(n, rank)
    for f, xl, x6 in zip(facs, xld, x64):
        assert xl.dtype == np.longdouble and xl.shape == (n, n)
        p = f.piv
        x = np.asarray(xl[:, p], dtype=np.float64)                       # undo the column scatter
        assert bool((x[rank:] == 0).all()) and bool((x[:, rank:] == 0).all()) and bool((np.triu(x, 1) == 0).all())
        if rank:
            lp = torch.from_numpy(f.L[p][:rank, :rank])
            want = torch.linalg.solve_triangular(lp, torch.eye(rank, dtype=torch.float64), upper=False).numpy()
            scale = float(np.abs(want).max())
            assert float(np.abs(x[:rank, :rank] - want).max()) <= 1e-9 * scale
            assert float(np.abs(x6 - xl).max()) <= 1e-9 * scale


@pytest.mark.parametrize("case", C.TRINV_CASES, ids=C.case_id)
def test_trinv_cases_have_the_rank_they_name(case):
    n, rank = case
    facs, xld, x64 = C.trinv_case(n, rank)                               # asserts the ranks
    assert all(C.stop_is_clear(f) for f in facs)
    tol, e64 = C.inverse_tolerance(xld, x64)
    assert tol > 0 or rank == 0
    _FIGURES.append(f"trinv n={n} rank={rank}: e64 {e64:.2e}, tolerance {tol:.2e}, max|X| "
                    f"{max(float(np.abs(x).max()) for x in xld):.2e}")


# ------------------------------------------------------------------------------------------------------------------
# Marchenko-Pastur rank
# ------------------------------------------------------------------------------------------------------------------
def test_ref_mp_rank_against_the_oracle():
    """the spectra of test_mp_rank_matches_oracle (tests/test_kernels_gpu.py)"""
    from oracle import basd_oracle as O
    g = torch.Generator().manual_seed(0)
    for r in (3, 9, 0, 31):
        z = torch.randn(400, 32, generator=g)
        if r:
            z = z + 3.0 * (torch.randn(400, r, generator=g) @ torch.randn(r, 32, generator=g)) / r ** 0.5
        ev = torch.linalg.eigvalsh((z.T @ z).double()).float().numpy()
        assert C.ref_mp_rank(ev, 400, 32, 31)[0] == min(O.mp_rank(z), 31)
    z = torch.randn(20, 32, generator=g) + 3.0 * torch.randn(20, 2, generator=g) @ torch.randn(2, 32, generator=g)
    ev = torch.linalg.eigvalsh((z.T @ z).double()).float().numpy()
    assert C.ref_mp_rank(ev, 20, 32, 31)[0] == min(O.mp_rank(z), 31)
    assert C.ref_mp_rank(np.ones(64, dtype=np.float32), 4096, 64, 63) == (0, C.STATUS_RANK0)
    assert C.ref_mp_rank(np.full(64, np.nan, dtype=np.float32), 4096, 64, 63) == (0, C.STATUS_NONFINITE)


@pytest.mark.parametrize("n", C.MP_SIZES)
def test_mp_spectra_stay_clear_of_their_edge(n):
    names = set()
    for name, evals, rows, d, cap in C.mp_launches(n):
        names.add(name)
        assert evals.dtype == np.float32 and evals.shape[1] == n and d == n
        for ev in evals:
            srt, n_eff, edge = C.mp_edge(ev, rows, d)
            assert float(np.abs(srt[:n_eff].astype(np.float64) / float(edge) - 1.0).min()) >= C.EDGE_MARGIN
            count = int((srt[:n_eff] > edge).sum())
            assert count >= 1 and C.ref_mp_rank(ev, rows, d, cap) == (min(count, cap), 0)
            if name == "cap":
                assert cap < count
            if name == "rows<n":
                assert rows < n and n_eff == rows and count < n_eff
                assert float(srt[n_eff]) < float(srt[n_eff - 1])          # the values past n_eff would change the median
        if name == "orders":
            asc, desc = evals[1], evals[0]
            assert bool((np.diff(desc) <= 0).all()) and bool((np.diff(asc) >= 0).all())
            assert not bool((np.diff(evals[2]) <= 0).all()) and not bool((np.diff(evals[2]) >= 0).all())
            assert len({C.ref_mp_rank(ev, rows, d, cap) for ev in evals[:3]}) == 1
            if n >= 4:
                assert len(np.unique(evals[3])) <= n - 3                   # exact duplicates
    assert names >= {"orders", "rows<n"} and (n < 16 or "cap" in names)


def test_report_reference_figures():
    """runs after the case tests above: e64 and tolerances per case, for the record (pytest -s)"""
    for line in _FIGURES:
        print("factor-ref", line)


# ------------------------------------------------------------------------------------------------------------------
# refusals: every check below returns before a kernel is launched, so no GPU is needed
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def entries():
    import basd_amd._native as native
    if not __import__("os").path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


_NULL = ctypes.c_void_p(0)
BASD_OK, BASD_ERR_SHAPE = 0, 1


def _host(n, dtype):
    """a host buffer behind a fake pointer: nothing may be read or written through it"""
    t = torch.full((n,), -7, dtype=dtype)
    return t, ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", [0, 209, 210, 256, 1000])
def test_trinv_refuses_sizes_outside_the_lds_resident_forms(entries, n):
    t, p = _host(64, torch.float64)
    assert entries.basd_trinv_f64(p, p, p, 3, n, p, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_last_error() == f"trinv_f64: n={n} does not fit the LDS-resident forms (n <= 208)".encode()
    assert entries.basd_trinv_f64_masked(p, p, p, 3, n, p, p, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_trinv_f64(p, p, p, 0, n, p, _NULL) == BASD_OK                      # an empty batch is a no-op
    assert bool((t == -7).all())


def test_pchol_and_mp_rank_refuse_bad_shapes(entries):
    t, p = _host(64, torch.float64)
    for n, ld in ((0, 4), (257, 260), (64, 63), (64, 321)):
        assert entries.basd_pchol_f64(p, 3, n, 1e-13, _NULL, p, ld, p, p, p, _NULL) == BASD_ERR_SHAPE
        assert entries.basd_pchol_f64_masked(p, 3, n, 1e-13, _NULL, p, ld, p, p, p, p, _NULL) == BASD_ERR_SHAPE
    for n, rows in ((0, 10), (1025, 10), (64, 0)):
        assert entries.basd_mp_rank(p, 3, n, rows, 64, 63, p, p, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_pchol_f64(p, 0, 64, 1e-13, _NULL, p, 68, p, p, p, _NULL) == BASD_OK
    assert entries.basd_mp_rank(p, 0, 64, 256, 64, 63, p, p, _NULL) == BASD_OK
    assert bool((t == -7).all())

"""The fp64 factor kernels -- pivoted Cholesky (basd_pchol_f64_masked: both register kernels and the global-memory one),
the inverse of its factor (basd_trinv_f64_masked: blocked, blocked + border) and the Marchenko-Pastur rank
(basd_mp_rank: both launch widths) -- against the plain references of tests/_factor_cases.py (GPU box only).

A factor is judged per element against the long-double reference, with the pivot sequence, the rank and the completed
tail of ``piv``; the tolerance is measured per case (8 times the distance between the fp64 and the long-double
reference, floored at 16 eps of the natural scale) and printed next to the kernel's figure (pytest -s).
tests/test_factor_cases_cpu.py holds the proof that the inputs have one pivot order whatever the arithmetic.

The C entries are called directly: every output is a caller-owned buffer pre-filled with a NaN / negative pattern no
kernel produces (torch.empty may hand back the block that held the previous launch's correct result)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _factor_cases as C

pytestmark = pytest.mark.gpu

POISON_F32 = 0x7FC00D1E
POISON_F64 = 0x7FF8000000D1E5ED
POISON_I32 = -7077


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


@pytest.fixture(autouse=True)
def _clean_status_word(nat):
    nat.status_word("cuda").zero_()
    yield


def _poisoned(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, POISON_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    if dtype == torch.float64:
        return torch.full(shape, POISON_F64, dtype=torch.int64, device="cuda").view(torch.float64)
    return torch.full(shape, POISON_I32, dtype=torch.int32, device="cuda")


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _poison_of(t):
    return {torch.float32: POISON_F32, torch.float64: POISON_F64}.get(t.dtype, POISON_I32)


def _untouched(t) -> bool:
    return bool((_bits(t) == _poison_of(t)).all())


def _same_bits(a, b) -> bool:
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _pchol(nat, a, tol=C.TOL, dmax_ref=None, ld=None, skip=None):
    """basd_pchol_f64_masked on a [batch, n, n] (numpy or device tensor) over poisoned outputs -> dict of CPU tensors"""
    a = torch.as_tensor(a, dtype=torch.float64).cuda().contiguous()
    batch, n, _ = a.shape
    ld = nat.jacobi_ld(n) if ld is None else ld
    out = {"w0": _poisoned((batch, n, ld), torch.float32), "lwork": _poisoned((batch, n, n), torch.float64),
           "piv": _poisoned((batch, n), torch.int32), "rank": _poisoned((batch,), torch.int32)}
    dref = None if dmax_ref is None else torch.as_tensor(dmax_ref, dtype=torch.float64).cuda()
    sk = None if skip is None else torch.as_tensor(skip, dtype=torch.int32).cuda()
    rc = nat.lib().basd_pchol_f64_masked(_ptr(a), batch, n, ctypes.c_double(tol), _ptr(dref), _ptr(out["w0"]), ld,
                                         _ptr(out["lwork"]), _ptr(out["piv"]), _ptr(out["rank"]), _ptr(sk),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_layout(got, b, n, rank):
    """what holds for every factorisation: everything written; w0 is the rounded factor, bit for bit; the steps from
    the rank on and the padding columns are exact zeros; piv is a permutation with an ascending tail; in pivot order the
    factor is lower triangular with EXACT zeros above the diagonal (a row pivoted before step k has no entry in
    column k: what the update leaves there is rounding residue, not a value)"""
    w0, lw, piv = got["w0"][b], got["lwork"][b], got["piv"][b]
    assert not bool(torch.isnan(lw).any()) and not bool(torch.isnan(w0).any()), "a poisoned or NaN element is left"
    assert _same_bits(w0[:, :n].contiguous(), lw.float()), "w0 is not float(lwork)"
    assert bool((_bits(w0[:, n:].contiguous()) == 0).all()), "w0 padding columns are not +0"
    assert bool((_bits(lw[rank:].contiguous()) == 0).all()) and bool((_bits(w0[rank:].contiguous()) == 0).all())
    assert sorted(piv.tolist()) == list(range(n))
    assert piv[rank:].tolist() == sorted(piv[rank:].tolist())
    lp = lw.t()[piv.long()]                                              # [row in pivot order, step]
    assert bool((torch.triu(lp, 1) == 0).all()), "an entry above the diagonal of the factor in pivot order"


def _check_against(got, b, ref_ld, steps, tol_elem, a, tol=C.TOL):
    """matrix b against its long-double reference at rank ``rank``: pivots of the first ``steps`` steps, tail, factor
    per element, residual.  Returns (largest factor deviation, residual / dmax0)."""
    n = a.shape[0]
    rank = int(got["rank"][b])
    piv = got["piv"][b].numpy()
    assert np.array_equal(piv[:steps], ref_ld.piv[:steps]), f"pivot sequence differs in the first {steps} steps"
    L = got["lwork"][b].numpy().T                                       # [row, step]
    dev = float(np.abs(L[:, :rank].astype(np.longdouble) - ref_ld.L[:, :rank]).max()) if rank else 0.0
    Lx = L.astype(np.longdouble)
    sym = np.tril(a) + np.tril(a, -1).T
    res = float(np.abs(Lx @ Lx.T - sym).max())
    assert dev <= tol_elem, f"factor deviates by {dev:.3e} > {tol_elem:.3e}"
    bound = C.residual_bound(n, rank, ref_ld.dmax0, tol)
    assert res <= bound, f"residual {res:.3e} > {bound:.3e}"
    return dev, res / float(ref_ld.dmax0) if float(ref_ld.dmax0) else 0.0


# ------------------------------------------------------------------------------------------------------------------
# pivoted Cholesky
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.PCHOL_RANDOM, ids=C.case_id)
def test_pchol_random_graded_matrices(nat, case):
    n, rank, ld = case
    a, r64, rld = C.pchol_random_case(n, rank)
    got = _pchol(nat, a, ld=ld)
    e64 = C.factor_e64(r64, rld)
    tol_elem = max(C.MARGIN * e64, C.factor_floor(max(l.dmax0 for l in rld)))
    assert got["rank"].tolist() == [rank] * len(a)
    worst, worst_res, failures = 0.0, 0.0, []
    for b, l in enumerate(rld):
        _check_layout(got, b, n, rank)
        assert np.array_equal(got["piv"][b].numpy()[rank:], l.piv[rank:])
        try:
            dev, res = _check_against(got, b, l, C.compared_steps(l), float("inf"), a[b])
        except AssertionError as e:
            failures.append(f"matrix {b}: {e}")
            continue
        worst, worst_res = max(worst, dev), max(worst_res, res)
    print(f"factor-chain pchol {C.pchol_kernel_of(n)} n={n} rank={rank} ld={ld}: e64 {e64:.2e}, kernel {worst:.2e}, "
          f"tolerance {tol_elem:.2e}, residual {worst_res:.2e} dmax0")
    assert not failures, failures
    assert worst <= tol_elem, f"factor deviates by {worst:.3e} > {tol_elem:.3e} (e64 {e64:.3e})"


@pytest.mark.parametrize("kind", C.SPECTRUM_KINDS)
@pytest.mark.parametrize("n", C.SPECTRUM_SIZES)
def test_pchol_rank_on_a_spectrum_graded_through_the_tolerance(nat, n, kind):
    a, r64, rld = C.spectrum_case(n, kind)
    got = _pchol(nat, a)
    worst, e64s = 0.0, 0.0
    for b, (f, l) in enumerate(zip(r64, rld)):
        rank = int(got["rank"][b])
        lo, hi = C.rank_at(l, 2 * C.TOL), C.rank_at(l, C.TOL / 2)
        assert lo <= rank <= hi, f"rank {rank} outside [{lo}, {hi}]"
        # everything else at the rank returned (the references ran on to tol / 2; the columns in front of a stop do
        # not depend on it)
        _check_layout(got, b, n, rank)
        assert np.array_equal(got["piv"][b].numpy()[:rank], l.piv[:rank])
        assert got["piv"][b].tolist()[rank:] == sorted(set(range(n)) - set(l.piv[:rank].tolist()))
        assert f.rank >= rank, "the fp64 reference stops before the kernel: no e64 for its last columns"
        e64s = max(e64s, float(np.abs(f.L[:, :rank] - l.L[:, :rank]).max()))
        dev, _res = _check_against(got, b, l, rank, float("inf"), a[b])
        worst = max(worst, dev)
    tol_elem = max(C.MARGIN * e64s, C.factor_floor(max(l.dmax0 for l in rld)))
    print(f"factor-chain pchol spectrum {kind} n={n}: ranks {got['rank'].tolist()}, e64 {e64s:.2e}, kernel {worst:.2e}, "
          f"tolerance {tol_elem:.2e}")
    assert worst <= tol_elem


@pytest.mark.parametrize("n", C.EXACT_SIZES)
def test_pchol_exact_diagonals_and_the_tie_rule(nat, n):
    """nothing rounds on diagonal matrices of even powers of two: every output is compared with ==.  Ties go to the
    lowest index across quads, 16-lane rows, the four rows of a wave, the lane + 64 q slots and the four waves of the
    global kernel."""
    cases = C.exact_diagonals(n)
    a = np.stack([np.diag(d) for d in cases.values()])
    got = _pchol(nat, a, tol=C.EXACT_TOL)
    for b, (name, d) in enumerate(cases.items()):
        piv, rank, L = C.exact_expectation(d)
        assert int(got["rank"][b]) == rank, name
        assert got["piv"][b].tolist() == piv.tolist(), name
        assert np.array_equal(got["lwork"][b].numpy().T, L), name
        _check_layout(got, b, n, rank)


@pytest.mark.parametrize("n", [64, 196, 256])
def test_pchol_dmax_ref_sets_the_stop_threshold(nat, n):
    """d_k = 2^-k, tol = 2^-20: rank = #{d_k > tol dmax_ref} exactly, for a dmax_ref above the matrix's own maximum, below
    it and equal to it; without dmax_ref the matrix's own maximum counts"""
    d = 2.0 ** -np.arange(n, dtype=np.float64)
    a = np.stack([np.diag(d)] * len(C.DMAX_REFS))
    got = _pchol(nat, a, tol=C.DMAX_TOL, dmax_ref=C.DMAX_REFS)
    want = [int((d > C.DMAX_TOL * r).sum()) for r in C.DMAX_REFS]
    assert want == [17, 25, 20] and got["rank"].tolist() == want
    for b, rank in enumerate(want):
        assert got["piv"][b].tolist() == list(range(n))
        L = np.zeros((n, n))
        L[np.arange(rank), np.arange(rank)] = np.sqrt(d[:rank])
        assert np.array_equal(got["lwork"][b].numpy().T, L)
        _check_layout(got, b, n, rank)
    own = _pchol(nat, a, tol=C.DMAX_TOL)
    assert own["rank"].tolist() == [20] * len(a) and _same_bits(own["lwork"][0], got["lwork"][2])


@pytest.mark.parametrize("n,rank", C.ONE_PER_KERNEL)
def test_pchol_reads_the_lower_triangle_only(nat, n, rank):
    """producers that accumulate lower tiles only (basd_token_gram) leave the strict upper triangle unspecified"""
    a = C.one_per_kernel_input(n, rank)
    want = _pchol(nat, a)
    up = a.copy()
    up[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
    got = _pchol(nat, up)
    assert want["rank"].tolist() == [rank] * len(a)
    for name in ("w0", "lwork", "piv", "rank"):
        assert _same_bits(got[name], want[name]), name


@pytest.mark.parametrize("n,rank", C.ONE_PER_KERNEL)
def test_pchol_skip_mask_leaves_masked_problems_untouched(nat, n, rank):
    a = C.one_per_kernel_input(n, rank, batch=4)
    want = _pchol(nat, a)
    mask = [0, 1, 1, 0]
    got = _pchol(nat, a, skip=mask)
    for b, m in enumerate(mask):
        for name in ("w0", "lwork", "piv", "rank"):
            if m:
                assert _untouched(got[name][b]), (name, b)
            else:
                assert _same_bits(got[name][b], want[name][b]), (name, b)
    none = _pchol(nat, a, skip=[5, -1, 1, 2])                              # any non-zero entry masks
    assert all(_untouched(none[name]) for name in none)


# ------------------------------------------------------------------------------------------------------------------
# triangular inverse
# ------------------------------------------------------------------------------------------------------------------
def _trinv(nat, lwork, piv, rank, skip=None, n=None):
    """basd_trinv_f64_masked over a poisoned output; lwork [batch, step, row], piv, rank as pchol leaves them"""
    lwork = torch.as_tensor(lwork, dtype=torch.float64).cuda().contiguous()
    piv = torch.as_tensor(piv, dtype=torch.int32).cuda().contiguous()
    rank = torch.as_tensor(rank, dtype=torch.int32).cuda().contiguous()
    batch = lwork.shape[0]
    n = lwork.shape[1] if n is None else n
    out = _poisoned((batch, lwork.shape[1], lwork.shape[1]), torch.float64)
    sk = None if skip is None else torch.as_tensor(skip, dtype=torch.int32).cuda()
    rc = nat.lib().basd_trinv_f64_masked(_ptr(lwork), _ptr(piv), _ptr(rank), batch, n, _ptr(out), _ptr(sk),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu()


def _upload(facs):
    return (np.stack([f.L.T for f in facs]), np.stack([f.piv for f in facs]), np.array([f.rank for f in facs]))


def _inverse_deviation(out, xld) -> float:
    """largest elementwise distance of the whole n x n outputs from the references; a NaN (poison left) is inf"""
    dev = 0.0
    for b, x in enumerate(xld):
        d = np.abs(out[b].numpy().astype(np.longdouble) - x)
        dev = float("inf") if bool(np.isnan(d).any()) else max(dev, float(d.max(initial=0.0)))
    return dev


@pytest.mark.parametrize("case", C.TRINV_CASES, ids=C.case_id)
def test_trinv_of_the_reference_factor(nat, case):
    """fed ref_pchol's fp64 factor: a pchol change cannot mask a trinv fault, or the reverse.  The whole n x n output is
    judged, zeros included: rows at or past the rank, the upper part, the border-pivot columns of the leading rows."""
    n, rank = case
    facs, xld, x64 = C.trinv_case(n, rank)
    rc, out = _trinv(nat, *_upload(facs))
    assert rc == 0
    tol, e64 = C.inverse_tolerance(xld, x64)
    dev = _inverse_deviation(out, xld)
    print(f"factor-chain trinv {C.trinv_path_of(n)} n={n} rank={rank}: e64 {e64:.2e}, kernel {dev:.2e}, tolerance {tol:.2e}")
    assert dev <= tol
    for b, f in enumerate(facs):                                           # what is zero in the reference is +-0 here
        assert bool((out[b].numpy()[np.asarray(xld[b] == 0)] == 0).all())


def test_trinv_after_the_kernel_factorisation(nat):
    """the chain as the Procrustes forward runs it: pchol's own outputs, on the device, into trinv"""
    n, rank = 196, 195
    a, r64, rld = C.pchol_random_case(n, rank)
    got = _pchol(nat, a, ld=C.jacobi_ld(n))
    assert got["rank"].tolist() == [rank] * len(a)
    rc, out = _trinv(nat, got["lwork"], got["piv"], got["rank"])
    assert rc == 0
    facs = [C.Pchol(got["lwork"][b].numpy().T, got["piv"][b].numpy().astype(np.int64), rank, None, None, None, None)
            for b in range(len(a))]
    xld = [C.ref_trinv(f.L, f.piv, rank) for f in facs]
    x64 = [C.ref_trinv(f.L, f.piv, rank, dtype=np.float64) for f in facs]
    tol, e64 = C.inverse_tolerance(xld, x64)
    dev = _inverse_deviation(out, xld)
    print(f"factor-chain pchol+trinv n={n} rank={rank}: e64 {e64:.2e}, kernel {dev:.2e}, tolerance {tol:.2e}")
    assert dev <= tol


@pytest.mark.parametrize("n,rank", [(100, 99), (196, 193)])
def test_trinv_skip_mask_leaves_masked_problems_untouched(nat, n, rank):
    facs, _xld, _x64 = C.trinv_case(n, rank)
    lw, piv, rk = _upload(facs)
    rc, want = _trinv(nat, lw, piv, rk)
    mask = [1, 0, 1]
    rc2, got = _trinv(nat, lw, piv, rk, skip=mask)
    assert rc == rc2 == 0
    for b, m in enumerate(mask):
        assert _untouched(got[b]) if m else _same_bits(got[b], want[b]), b


def test_trinv_refuses_209_and_launches_nothing(nat):
    lw = np.zeros((3, 209, 209))
    rc, out = _trinv(nat, lw, np.tile(np.arange(209), (3, 1)), np.full(3, 209))
    assert rc == 1 and _untouched(out)
    assert nat.lib().basd_last_error() == b"trinv_f64: n=209 does not fit the LDS-resident forms (n <= 208)"
    with pytest.raises(nat.BasdNativeError, match="n <= 208"):
        nat.trinv(torch.zeros(1, 209, 209, dtype=torch.float64, device="cuda"),
                  torch.zeros(1, 209, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------
# Marchenko-Pastur rank
# ------------------------------------------------------------------------------------------------------------------
def _mp_rank(nat, evals, rows, d, cap):
    ev = torch.as_tensor(np.ascontiguousarray(evals), dtype=torch.float32).cuda()
    ranks = _poisoned((ev.shape[0],), torch.int32)
    status = nat.status_word("cuda")
    status.zero_()
    rc = nat.lib().basd_mp_rank(_ptr(ev), ev.shape[0], ev.shape[1], ctypes.c_int64(rows), d, cap, _ptr(ranks),
                                _ptr(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    word = int(status.item())
    status.zero_()
    return ranks.cpu().tolist(), word


@pytest.mark.parametrize("n", C.MP_SIZES)
def test_mp_rank_equals_the_reference(nat, n):
    """ascending, descending, shuffled and tied input (the kernel sorts for itself), rows < n, a cap below the count; 257 and
    wider take the 1024-thread launch"""
    for name, evals, rows, d, cap in C.mp_launches(n):
        want = [C.ref_mp_rank(ev, rows, d, cap) for ev in evals]
        got, word = _mp_rank(nat, evals, rows, d, cap)
        assert got == [w[0] for w in want], (name, n)
        assert word == 0, (name, n, word)
    rows = 4 * n
    flat = np.full((3, n), 2.5 * rows, dtype=np.float32)
    assert C.ref_mp_rank(flat[0], rows, n, n - 1) == (0, C.STATUS_RANK0)
    assert _mp_rank(nat, flat, rows, n, n - 1) == ([0, 0, 0], C.STATUS_RANK0)
    nan = np.full((3, n), np.nan, dtype=np.float32)
    nan[1:] = C.mp_launches(n)[0][1][:2]                                  # a healthy spectrum with one NaN in it
    nan[1, 0] = nan[2, n - 1] = np.nan
    assert [C.ref_mp_rank(ev, rows, n, n - 1) for ev in nan] == [(0, C.STATUS_NONFINITE)] * 3
    assert _mp_rank(nat, nan, rows, n, n - 1) == ([0, 0, 0], C.STATUS_NONFINITE)

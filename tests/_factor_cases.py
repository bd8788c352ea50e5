"""Case tables, inputs and plain references of tests/test_factor_chain_gpu.py: the fp64 factor kernels behind the
Procrustes forward and the selector's eigensolver -- diagonal-pivoted Cholesky (csrc/pchol.hip), the inverse of its
factor (csrc/trinv.hip) and the Marchenko-Pastur rank count (csrc/pchol.hip).

The references are numpy, in fp64 and in ``np.longdouble`` (x87 extended, eps = 1.08e-19; ``ref_pchol`` refuses to run
where long double is no wider than that).  A kernel is judged against the long-double result; the distance between the
fp64 and the long-double reference on the same input (``e64``) is the measure of what fp64 arithmetic may cost, and a
kernel may differ from the long-double result by 8 e64 (fma, another summation order), with a floor of 16 eps times
the natural scale.  tests/test_factor_cases_cpu.py proves that the inputs are fit to judge a kernel with: the pivot
order of every case is the same in fp64 and in long double, with a gap between the two largest residual diagonals that
rounding cannot close.
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

EPS = float(np.finfo(np.float64).eps)             # 2.2e-16
TOL = 1e-13                                       # the stop tolerance of every caller (PCHOL_TOL)
GAP_MIN = 1e-6                                    # smallest relative top-two gap of a compared step
PIVOT_FLOOR = 1e-8                                # steps with pivot <= PIVOT_FLOOR dmax0 are not compared
MARGIN = 8.0                                      # a kernel may be MARGIN e64 away from the long-double reference
BATCH = 3

# ------------------------------------------------------------------------------------------------------------------
# dispatch mirror (basd_pchol_f64_masked, basd_trinv_f64_masked, basd_mp_rank)
# ------------------------------------------------------------------------------------------------------------------
PCHOL_SIZES = {"reg<6,32>": [1, 2, 7, 63, 64, 65, 129, 191, 192], "reg<7,28>": [193, 195, 196],
               "global": [197, 208, 255, 256]}


def pchol_kernel_of(n: int) -> str:
    assert 1 <= n <= 256
    return "reg<6,32>" if n <= 192 else "reg<7,28>" if n <= 196 else "global"


def trinv_path_of(n: int) -> str:
    assert 1 <= n <= 208
    return "blocked" if n <= 192 else "blocked+border"


def mp_rank_threads(n: int) -> int:
    assert 1 <= n <= 1024
    return 256 if n <= 256 else 1024


def jacobi_ld(m_rows: int) -> int:
    """_native.jacobi_ld: the column stride every caller hands to pchol"""
    ld = (m_rows + 3) // 4 * 4
    return ld + 4 if ld % 32 == 0 else ld


# ------------------------------------------------------------------------------------------------------------------
# pivoted Cholesky
# ------------------------------------------------------------------------------------------------------------------
Pchol = collections.namedtuple("Pchol", "L piv rank gaps pivots dmax0 stop")


def ref_pchol(a, tol: float = TOL, dmax_ref=None, dtype=np.float64) -> Pchol:
    """Greedy diagonal pivoting in the kernel's form: right-looking, ties to the lowest index, only the lower triangle
    of ``a`` is read, rows stay in original order.  Stops at the first step whose pivot fails
    ``pivot > tol dmax0 and pivot > 0`` (dmax0 = ``dmax_ref`` or the first pivot).

    L [n rows, n steps] (zero columns from the rank on), piv [n] (pivots, then the unpivoted indices ascending), rank,
    gaps [rank] ((largest - second largest live residual diagonal) / pivot; inf with one row left), pivots [rank],
    dmax0, stop (the pivot that failed the test; None at full rank)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than fp64 here: no reference to judge with"
    a = np.asarray(a)
    n = a.shape[0]
    low = np.tril(a).astype(dtype)
    R = low + np.tril(low, -1).T
    L = np.zeros((n, n), dtype=dtype)
    alive = np.ones(n, dtype=bool)
    piv, gaps, pivots = [], [], []
    d = R.diagonal().copy()
    dmax0, stop = dtype(0), None
    for k in range(n):
        live = np.where(alive, d, -np.inf)
        p = int(np.argmax(live))                               # first maximum: the lowest index
        pval = live[p]
        if k == 0:
            dmax0 = dtype(dmax_ref) if dmax_ref is not None else pval
        if not (pval > tol * dmax0) or not (pval > 0):
            stop = pval
            break
        live[p] = -np.inf
        second = live.max()
        gaps.append(float((pval - second) / pval) if np.isfinite(second) else float("inf"))
        pivots.append(pval)
        lkk = np.sqrt(pval)
        c = R[p, :] / lkk
        c[~alive] = 0
        c[p] = lkk
        L[:, k] = c
        R -= np.outer(c, c)
        d = R.diagonal().copy()
        alive[p] = False
        piv.append(p)
    rank = len(piv)
    piv += [i for i in range(n) if alive[i]]
    return Pchol(L, np.array(piv, dtype=np.int64), rank, np.array(gaps), np.array(pivots, dtype=dtype), dmax0, stop)


def compared_steps(ld: Pchol) -> int:
    """leading steps whose long-double pivot exceeds PIVOT_FLOOR dmax0: the steps whose pivot index a kernel must
    reproduce"""
    ok = np.asarray(ld.pivots > PIVOT_FLOOR * ld.dmax0)
    return ld.rank if bool(ok.all()) else int(np.argmin(ok))


def stop_is_clear(ref: Pchol, tol: float = TOL) -> bool:
    """the last pivot taken is 100 times above tol dmax0 and the one refused 10 times below it: the rank of the case does
    not hang on rounding (of the kernel, or of the BLAS that forms the input on another machine)"""
    taken = ref.rank == 0 or bool(ref.pivots[-1] >= 100 * tol * ref.dmax0)
    return taken and (ref.stop is None or bool(ref.stop <= tol / 10 * ref.dmax0))


def factor_floor(dmax0) -> float:
    return 16 * EPS * float(np.sqrt(np.longdouble(dmax0)))


def residual_bound(n: int, rank: int, dmax0, tol: float = TOL) -> float:
    """|L L^T - A| <= (8 n eps + tol [rank < n]) dmax0.  Every entry of the residual matrix takes at most n fma
    updates by products bounded by dmax0 (|c_i c_j| <= sqrt(d_i d_j)), each within eps / 2 of exact, and the column
    itself carries the rounding of the square root, the reciprocal and the product (3 eps / 2 on each factor): well
    inside 8 n eps dmax0.  What the stop leaves unfactored is a PSD matrix whose diagonal is below tol dmax0, so all its
    entries are."""
    return (8 * n * EPS + (tol if rank < n else 0.0)) * float(dmax0)


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1_000_003 + int(k) + 17) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


def graded_psd(n: int, rank: int, batch: int = BATCH, salt: int = 0) -> np.ndarray:
    """[batch, n, n] fp64: the Gram matrix of randn(4 n, r) logspace(0, -3, r) @ randn(r, n) -- the generator of
    test_pchol_then_jacobi_is_an_eigensolver; rank 0 is the zero matrix"""
    if rank == 0:
        return np.zeros((batch, n, n))
    g = _gen(n, rank, salt)
    x = torch.randn(batch, 4 * n, rank, dtype=torch.float64, generator=g) * torch.logspace(0, -3, rank, dtype=torch.float64)
    z = x @ torch.randn(batch, rank, n, dtype=torch.float64, generator=g)
    return (z.transpose(1, 2) @ z).numpy()


# (n, rank, ld): every size full rank at the callers' stride, and one rank-deficient case per size at a wider one
_DEFICIENT = {2: 1, 7: 3, 63: 62, 64: 5, 65: 21, 129: 128, 191: 8, 192: 63, 193: 192, 195: 7, 196: 195, 197: 196, 208: 6,
              255: 85, 256: 255}
PCHOL_RANDOM = [(n, n, jacobi_ld(n)) for sizes in PCHOL_SIZES.values() for n in sizes]
PCHOL_RANDOM += [(n, r, min(jacobi_ld(n) + 12, 320)) for n, r in _DEFICIENT.items()] + [(196, 60, 320)]


def case_id(case) -> str:
    return "-".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def pchol_random_case(n: int, rank: int):
    """inputs [BATCH, n, n] and, per matrix, the fp64 and the long-double reference"""
    a = graded_psd(n, rank)
    return a, [ref_pchol(m) for m in a], [ref_pchol(m, dtype=np.longdouble) for m in a]


ONE_PER_KERNEL = [(191, 190), (196, 195), (255, 85)]       # (n, rank) of the lower-triangle and skip-mask tests


def one_per_kernel_input(n: int, rank: int, batch: int = BATCH) -> np.ndarray:
    return graded_psd(n, rank, batch=batch, salt=3)


def factor_e64(r64, rld, steps=None) -> float:
    """largest elementwise difference of the fp64 and the long-double factors of a case (first ``steps`` columns)"""
    return max(float(np.abs(f.L[:, :steps] - l.L[:, :steps]).max()) if f.L[:, :steps].size else 0.0
               for f, l in zip(r64, rld))


# ---- spectra graded through the tolerance ------------------------------------------------------------------------
SPECTRUM_SIZES = [64, 196, 256]
SPECTRUM_KINDS = ["through", "gap"]
SPECTRUM_GAP_MIN = 0.02


def spectrum_matrix(n: int, kind: str, seed: int) -> np.ndarray:
    """A = P L0 L0^T P^T, L0 = (I + U) diag(g), U strictly lower with |u| <= 0.1, P a random permutation, formed in
    long double and rounded once.  The residual diagonal of row i at step k is g_i^2 + sum_{k <= j < i} g_j^2 u_ij^2, so
    the pivots are g_k^2 in order with a top-two gap of at least 1 - rho - 0.01 / (1 - rho), rho the ratio of successive
    g^2 (0.87 at n = 256: 0.06).
    "through": g_k^2 = 10^(-16 k / (n - 1)), no gap anywhere near tol dmax0 = 1e-13.
    "gap": the same grade down to 1e-10 over the first half, exact zero columns behind it (rank n / 2)."""
    rng = np.random.default_rng(1000 * n + seed)
    k = np.arange(n, dtype=np.longdouble)
    if kind == "through":
        g2 = np.longdouble(10) ** (-16 * k / (n - 1))
    else:
        m = n // 2
        g2 = np.where(k < m, np.longdouble(10) ** (-10 * k / (m - 1)), 0)
    u = np.tril(rng.uniform(-0.1, 0.1, (n, n)), -1).astype(np.longdouble)
    l0 = (np.eye(n, dtype=np.longdouble) + u) * np.sqrt(g2)[None, :]
    a = l0 @ l0.T
    p = rng.permutation(n)
    return np.asarray(a[np.ix_(p, p)], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def spectrum_case(n: int, kind: str):
    """inputs and references run to tol / 2: a kernel's rank may lie anywhere from the count at 2 tol to this one, and
    the columns in front of its rank do not depend on where it stops"""
    a = np.stack([spectrum_matrix(n, kind, s) for s in range(BATCH)])
    return a, [ref_pchol(m, TOL / 2) for m in a], [ref_pchol(m, TOL / 2, dtype=np.longdouble) for m in a]


def rank_at(ref: Pchol, tol: float) -> int:
    """the rank the same factorisation stops at with another tolerance (<= the run's own)"""
    ok = np.asarray(ref.pivots > tol * ref.dmax0)
    return ref.rank if bool(ok.all()) else int(np.argmin(ok))


# ---- exact cases: diagonal matrices of powers of four ------------------------------------------------------------
EXACT_TOL = 2.0 ** -80                            # below every entry's ratio to the largest (2^-62 at most)
EXACT_SIZES = [7, 192, 196, 256]                  # 256: four waves of the global kernel; 192 / 196: 3 / 4 slots per lane
BOUNDARIES = [4, 16, 32, 64, 128, 192]            # quads, 16-lane rows, (half waves), lane + 64 q slots = waves


def exact_diagonals(n: int) -> dict:
    """name -> diagonal [n] of even powers of two: square roots, quotients and updates are exact"""
    k = np.arange(n)
    out = {"all-equal": np.full(n, 0.25), "zero": np.zeros(n)}
    # equal runs of four across every boundary (two entries on each side), each run at its own level, above a
    # descending background that itself repeats every 24 entries (ties between distant lanes)
    d = 4.0 ** -(8 + k % 24)
    for level, b in enumerate(BOUNDARIES):
        if b + 2 <= n:
            d[b - 2:b + 2] = 4.0 ** -level
    out["runs"] = d
    # a descending head, then one level for all the rest
    out["descending-then-tied"] = np.where(k < min(10, n // 2), 4.0 ** -k, 4.0 ** -12)
    return out


def exact_expectation(d: np.ndarray, tol: float = EXACT_TOL):
    """piv, rank, diag(L) of a diagonal matrix, from the definition: descending value, ties by ascending index"""
    n = len(d)
    order = sorted(range(n), key=lambda i: (-d[i], i))
    rank = int(((d > 0) & (d > tol * d.max())).sum())
    piv = order[:rank] + sorted(order[rank:])
    L = np.zeros((n, n))
    for step, p in enumerate(piv[:rank]):
        L[p, step] = np.sqrt(d[p])
    return np.array(piv), rank, L


DMAX_TOL = 2.0 ** -20
DMAX_REFS = [8.0, 2.0 ** -5, 1.0]                 # above the matrix's own maximum (1), below it, equal to it


# ------------------------------------------------------------------------------------------------------------------
# triangular inverse
# ------------------------------------------------------------------------------------------------------------------
def ref_trinv(L, piv, rank: int, dtype=np.longdouble) -> np.ndarray:
    """L_p^-1 P by forward substitution, in the kernel's output layout out[k, piv[c]] = X[k, c]; L [n rows, n steps] as
    ref_pchol returns it, L_p = L[piv] lower triangular; rows at or past the rank are zero"""
    n = L.shape[0]
    piv = np.asarray(piv)
    lp = np.asarray(L)[piv][:rank, :rank].astype(dtype)
    x = np.zeros((rank, rank), dtype=dtype)
    for i in range(rank):
        row = -(lp[i, :i] @ x[:i, :]) if i else np.zeros(rank, dtype=dtype)
        row[i] += 1
        x[i, :] = row / lp[i, i]
    out = np.zeros((n, n), dtype=dtype)
    out[:rank, piv[:rank]] = x
    return out


TRINV_SIZES = [1, 15, 16, 17, 100, 176, 191, 192, 193, 196, 197, 207, 208]


def _trinv_ranks(n: int):
    ranks = {n, n - 1, min(5, n - 1), 0}
    if n in (196, 208):
        ranks |= {192, 193 if n == 196 else 200}       # the rank ends at the 192 boundary / inside the border
    return sorted(r for r in ranks if r >= 0)


TRINV_CASES = [(n, r) for n in TRINV_SIZES for r in _trinv_ranks(n)]


@functools.lru_cache(maxsize=None)
def trinv_case(n: int, rank: int):
    """per matrix: ref_pchol's fp64 factor of a graded PSD matrix of that rank (what the kernel is fed), and the
    inverse from it in long double and in fp64"""
    a = graded_psd(n, rank, salt=2)                   # (salt 1 leaves one matrix of (192, 192) at rank 191)
    facs = [ref_pchol(m) for m in a]
    assert [f.rank for f in facs] == [rank] * len(facs), (n, rank, [f.rank for f in facs])
    xld = [ref_trinv(f.L, f.piv, f.rank) for f in facs]
    x64 = [ref_trinv(f.L, f.piv, f.rank, dtype=np.float64) for f in facs]
    return facs, xld, x64


def inverse_tolerance(xld, x64):
    """(tolerance, e64) of a case: max(8 e64, 16 eps max|X_ref|)"""
    e64 = max(float(np.abs(a - b).max()) for a, b in zip(xld, x64))
    return max(MARGIN * e64, 16 * EPS * max(float(np.abs(a).max()) for a in xld)), e64


# ------------------------------------------------------------------------------------------------------------------
# Marchenko-Pastur rank
# ------------------------------------------------------------------------------------------------------------------
STATUS_NONFINITE, STATUS_RANK0 = 2, 4
EDGE_MARGIN = 1e-4


def mp_edge(evals, rows: int, d: int):
    """(descending fp32 spectrum / rows, n_eff, edge) in the kernel's fp32 arithmetic"""
    f = np.float32
    v = np.asarray(evals, dtype=f) * (f(1.0) / f(rows))
    srt = np.sort(v)[::-1]
    n_eff = min(rows, len(v))
    sigma2 = srt[n_eff - 1 - (n_eff - 1) // 2]                 # lower median of the top n_eff, in ascending order
    s = f(1.0) + np.sqrt(f(d / rows))
    return srt, n_eff, f(f(sigma2 * s) * s)


def ref_mp_rank(evals, rows: int, d: int, cap: int):
    """(rank, status bits) of one spectrum: eigenvalues of X^T X, X [rows, d]"""
    if bool(np.isnan(np.asarray(evals, dtype=np.float32)).any()):      # a NaN has no place in the order: nothing counts
        return 0, STATUS_NONFINITE
    srt, n_eff, edge = mp_edge(evals, rows, d)
    with np.errstate(invalid="ignore"):
        count = int((srt[:n_eff] > edge).sum())
    status = 0 if count else (STATUS_RANK0 if edge == edge else STATUS_NONFINITE)
    return min(count, cap), status


MP_SIZES = [7, 192, 256, 257, 384, 768, 1024]


def mp_spectrum(n: int, spikes: int, seed: int) -> np.ndarray:
    """eigenvalues of X^T X / rows as fp32 [n], descending: a bulk in [0.8, 1.2] and ``spikes`` values in [20, 40]"""
    rng = np.random.default_rng(77 * n + seed)
    v = np.concatenate([rng.uniform(20.0, 40.0, spikes), rng.uniform(0.8, 1.2, n - spikes)])
    return np.sort(v.astype(np.float32))[::-1].copy()


def mp_launches(n: int):
    """launches of one size: (name, evals [batch, n] fp32, rows, d, cap).  The orders and duplicates share one launch;
    rows < n and a cap below the count need their own (rows, d and cap are launch arguments)."""
    rng = np.random.default_rng(n)
    spikes = max(1, n // 8)
    base = mp_spectrum(n, spikes, 0)
    dup = base.copy()
    if n >= 4:
        dup[1] = dup[0]                                          # a tied pair of spikes
        dup[n // 2:n // 2 + 2] = dup[n // 2]                     # a tied pair in the bulk, next to the median
        dup[-1] = dup[-2]
    rows = 4 * n
    orders = np.stack([base, base[::-1], base[rng.permutation(n)], dup[rng.permutation(n)]]) * np.float32(rows)
    out = [("orders", orders, rows, n, n - 1)]
    short = max(2, n // 2)                                       # rows < n: only the top ``rows`` eigenvalues count
    few = max(1, short // 8)
    sp = np.stack([mp_spectrum(n, few, s)[rng.permutation(n)] for s in (1, 2, 3)])
    sp[:, :] = np.where(sp < 2.0, sp * np.float32(0.05), sp)     # X X^T has ``rows`` eigenvalues: the rest is ~ 0
    # the bulk of the short problem: the top ``short`` values are the spikes and bulk values around 1
    for b in range(3):
        idx = np.argsort(sp[b])[::-1][few:short]
        sp[b, idx] = np.random.default_rng(n + b).uniform(0.8, 1.2, len(idx)).astype(np.float32)
    out.append(("rows<n", sp * np.float32(short), short, n, n - 1))
    if spikes >= 2:
        out.append(("cap", orders[:3].copy(), rows, n, spikes - 1))
    return out

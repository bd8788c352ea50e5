"""Plain numpy restatement of the eigenvalue-counting Marchenko-Pastur rank (csrc/tridiag.hip) and its test inputs.

``householder_tridiag``: the unblocked Householder reduction (LAPACK dsytd2's arithmetic, reflectors not kept).
``sturm_counts``: the pivmin-guarded LDL^T pivot count (LAPACK dlaebz).  ``counted_mp_rank``: 256-section for the lower
median eigenvalue inside the Gershgorin bracket, the noise edge and the count above it, with the kernel's status word.
``direct_mp_rank``: the definition (reference layer_selector.py:8-20) on ``numpy.linalg.eigvalsh`` in fp64, with the
relative gap between the edge and its nearest eigenvalue, which every case asserts before it trusts a count.

Inputs are planted-rank token matrices built like those of tests/test_startup_gpu.py (rank r at SNR 3 plus unit noise,
fp32 tokens)."""
import functools
import math

import numpy as np
import torch

EPS64 = float(np.finfo(np.float64).eps)
TINY64 = float(np.finfo(np.float64).tiny)
STATUS_NONFINITE, STATUS_RANK0 = 2, 4
GAP = 1e-6                        # an eigenvalue this close (relative) to the edge makes the count a matter of rounding

# (M, D, r): restatement cases (CPU), also the (diag, off) inputs of the device count
CPU_CASES = [(40, 3, 1), (400, 64, 6), (700, 65, 6), (1500, 193, 12), (3000, 512, 30)]
# the wide route on the GPU: past the old 1024 limit on the smaller side, both orientations, and one small shape
WIDE_CASES = [(1500, 1280, 40), (1100, 1536, 24), (2600, 2048, 48), (2048, 4096, 30), (700, 65, 6)]
# orders for the reduction kernel: empty loop, one reflector, the edges of a 64-row block, a ragged last row block,
# one past the old limit
TRIDIAG_SIZES = [2, 3, 63, 64, 65, 193, 1025]


def planted_tokens(m: int, d: int, r: int, seed: int | None = None) -> torch.Tensor:
    """fp32 [m, d]: rank r at SNR 3 + unit noise (the construction of tests/test_startup_gpu.py)"""
    g = torch.Generator().manual_seed(m + d if seed is None else seed)
    return 3.0 * (torch.randn(m, r, generator=g) @ torch.randn(r, d, generator=g)) / r ** 0.5 + torch.randn(m, d, generator=g)


def gram64(x: torch.Tensor) -> np.ndarray:
    """fp64 Gram on the smaller side of fp32 tokens (the reference's rule, layer_selector.py:13-15), not divided by M"""
    a = x.double().numpy()
    return a.T @ a if a.shape[0] >= a.shape[1] else a @ a.T


@functools.lru_cache(maxsize=None)
def case(m: int, d: int, r: int):
    """-> (tokens fp32 [m, d], gram fp64, ascending eigvalsh of the gram); computed once, never modified"""
    x = planted_tokens(m, d, r)
    g = gram64(x)
    lam = np.linalg.eigvalsh(g)
    g.setflags(write=False)
    lam.setflags(write=False)
    return x, g, lam


def direct_mp_rank(lam: np.ndarray, rows: int, d: int):
    """eigenvalues of the smaller-side Gram (NOT divided by rows) -> (rank, relative gap of the nearest eigenvalue to
    the edge): lower median, lambda_+ = med / rows * (1 + sqrt(d / rows))^2, count above"""
    srt = np.sort(np.asarray(lam, dtype=np.float64)) / rows
    sigma2 = srt[(srt.size - 1) // 2]
    edge = sigma2 * (1.0 + math.sqrt(d / rows)) ** 2
    gap = float(np.min(np.abs(srt - edge)) / abs(edge)) if edge != 0 else 0.0
    return int((srt > edge).sum()), gap


def householder_tridiag(a: np.ndarray):
    """symmetric fp64 [n, n] -> (diag [n], off [n - 1]) of an orthogonally similar tridiagonal matrix"""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    diag, off = np.empty(n), np.empty(n - 1)
    for k in range(n - 2):
        x = a[k + 1:, k].copy()
        alpha = x[0]
        xnorm2 = float(x[1:] @ x[1:])
        diag[k] = a[k, k]
        if xnorm2 == 0.0:                       # H = I
            off[k] = alpha
            continue
        beta = -math.copysign(math.sqrt(alpha * alpha + xnorm2), alpha)
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1.0
        a22 = a[k + 1:, k + 1:]
        p = tau * (a22 @ v)
        w = p - (0.5 * tau * float(p @ v)) * v
        a22 -= np.outer(v, w) + np.outer(w, v)
        off[k] = beta
    diag[n - 2], off[n - 2], diag[n - 1] = a[n - 2, n - 2], a[n - 1, n - 2], a[n - 1, n - 1]
    return diag, off


def tridiag_dense(diag, off) -> np.ndarray:
    return np.diag(np.asarray(diag, dtype=np.float64)) + np.diag(off, 1) + np.diag(off, -1)


def sturm_counts(diag, off, xs, pivmin: float) -> np.ndarray:
    """number of eigenvalues of the tridiagonal matrix below each shift of ``xs``"""
    xs = np.atleast_1d(np.asarray(xs, dtype=np.float64))
    e2 = np.asarray(off, dtype=np.float64) ** 2
    q = diag[0] - xs
    neg = q <= pivmin
    q = np.where(neg, np.minimum(q, -pivmin), q)
    count = neg.astype(np.int64)
    for i in range(1, len(diag)):
        q = (diag[i] - xs) - e2[i - 1] / q
        neg = q <= pivmin
        q = np.where(neg, np.minimum(q, -pivmin), q)
        count += neg
    return count


def counted_mp_rank(diag, off, rows: int, d: int, cap: int):
    """-> (rank, status word) as basd_tridiag_mp_rank leaves them"""
    diag, off = np.asarray(diag, dtype=np.float64), np.asarray(off, dtype=np.float64)
    n = diag.size
    if not (np.isfinite(diag).all() and np.isfinite(off).all()):
        return 0, STATUS_NONFINITE
    el, er = np.concatenate(([0.0], np.abs(off))), np.concatenate((np.abs(off), [0.0]))
    gl, gu = float((diag - el - er).min()), float((diag + el + er).max())
    pivmin = TINY64 * max(1.0, float((off ** 2).max()))
    radius = gu - gl
    margin = 2.0 * max(abs(gl), abs(gu)) * EPS64 * n + 4.0 * pivmin
    lo, hi = gl - margin, gu + margin
    want = (n - 1) // 2 + 1
    tolw = math.ldexp(radius, -48)
    frac = np.arange(1, 257) / 257.0
    for _ in range(8):
        width = hi - lo
        if width <= tolw:
            break
        pts = lo + width * frac
        hit = np.nonzero(sturm_counts(diag, off, pts, pivmin) >= want)[0]
        first = int(hit[0]) if hit.size else 256
        lo, hi = (pts[first - 1] if first > 0 else lo), (pts[first] if first < 256 else hi)
    med = 0.5 * (lo + hi)
    sq = 1.0 + math.sqrt(d / rows)
    edge = med / rows * sq * sq
    above = n - int(sturm_counts(diag, off, edge * rows, pivmin)[0])
    return min(above, cap), (STATUS_RANK0 if above == 0 else 0)


# hand-made tridiagonal matrices for the device count: name -> (diag, off, rows, d)
def handmade():
    n = 40
    out = {}
    dg = np.concatenate((np.full(n - 5, 1.0), [40.0, 50.0, 60.0, 70.0, 80.0]))
    out["diagonal: 5 above the edge"] = (dg, np.zeros(n - 1), 400, n)
    d2 = np.concatenate((np.linspace(0.9, 1.1, 20), np.linspace(30.0, 60.0, 12)))
    o2 = np.concatenate((np.full(19, 0.01), [0.0], np.full(11, 0.5)))                      # two decoupled blocks
    out["off = 0 in the middle"] = (d2, o2, 640, 32)
    out["identity"] = (np.ones(16), np.zeros(15), 160, 16)
    d4 = np.linspace(1.0, 2.0, 16)
    d4[5] = np.nan
    out["one NaN"] = (d4, np.full(15, 0.1), 160, 16)
    o5 = np.full(15, 0.1)
    o5[14] = np.inf
    out["one Inf in off"] = (np.linspace(1.0, 2.0, 16), o5, 160, 16)
    return out

"""Yardstick of csrc/resample.hip (no GPU, numpy only): the taps of the 1-D linear resample restated in float32 with
the kernel's operations in the kernel's order, and the forward, the adjoint and the importance backward built from
those taps in float64.  tests/test_resample_cpu.py checks the restatement itself, tests/test_resample_kernels_gpu.py
holds the kernels to it."""
import numpy as np

F32 = np.float32
U24 = 2.0 ** -24          # unit roundoff of fp32

# (n_in, n_out): the smallest shapes at which each mechanism of the kernels can go wrong
PAIRS = [
    (7, 7),                                   # identity
    (256, 196), (49, 196), (729, 576),        # the shipped ratios
    (13, 17), (17, 13),                       # odd sizes, both directions
    (1, 5), (5, 1),                           # a single row on either side
    (1024, 3),                                # almost every adjoint row receives nothing
    (3, 1024),                                # ~340 contributors per adjoint row, the LDS table at its limit
]
BATCHES = (1, 3)
WIDTHS = (4, 36, 260)     # one vector; no multiple of 16; wider than one workgroup's 256 threads


def taps(n_in: int, n_out: int):
    """(lo int64 [n_out], hi int64 [n_out], fr float32 [n_out]): every operation a float32 operation rounded on its
    own, in the order ratio = n_in / n_out, (i + 0.5) * ratio, - 0.5, max(0, .), truncate, clamp, pos - lo."""
    i = np.arange(n_out)
    if n_in == n_out:
        return i.copy(), i.copy(), np.zeros(n_out, F32)
    ratio = F32(n_in) / F32(n_out)
    scaled = (i.astype(F32) + F32(0.5)) * ratio
    pos = np.maximum(scaled - F32(0.5), F32(0.0))
    assert ratio.dtype == F32 and scaled.dtype == F32 and pos.dtype == F32
    lo = np.minimum(pos.astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    fr = pos - lo.astype(F32)
    assert fr.dtype == F32
    return lo, hi, fr


def weights(n_in: int, n_out: int):
    """the taps as fp64 weights (w_lo, w_hi); the hi tap of a row with fr == 0 does not exist (weight 0)"""
    _, _, fr = taps(n_in, n_out)
    fr64 = fr.astype(np.float64)
    return 1.0 - fr64, fr64


def forward(x: np.ndarray, n_out: int) -> np.ndarray:
    """x [B, n_in, D] -> [B, n_out, D] in float64 (gather along the token axis)"""
    x = np.asarray(x, np.float64)
    lo, hi, _ = taps(x.shape[1], n_out)
    w_lo, w_hi = weights(x.shape[1], n_out)
    return w_lo[None, :, None] * x[:, lo, :] + w_hi[None, :, None] * x[:, hi, :]


def adjoint(g: np.ndarray, n_in: int) -> np.ndarray:
    """g [B, n_out, D] -> [B, n_in, D] in float64 (scatter-add of the same taps: written independently of forward)"""
    g = np.asarray(g, np.float64)
    n_out = g.shape[1]
    lo, hi, _ = taps(n_in, n_out)
    w_lo, w_hi = weights(n_in, n_out)
    out = np.zeros((g.shape[0], n_in, g.shape[2]))
    for i in range(n_out):
        out[:, lo[i], :] += w_lo[i] * g[:, i, :]
        if w_hi[i] != 0.0:
            out[:, hi[i], :] += w_hi[i] * g[:, i, :]
    return out


def matrix(n_in: int, n_out: int) -> np.ndarray:
    """R [n_out, n_in] float64 with forward(x) = R x"""
    lo, hi, _ = taps(n_in, n_out)
    w_lo, w_hi = weights(n_in, n_out)
    r = np.zeros((n_out, n_in))
    np.add.at(r, (np.arange(n_out), lo), w_lo)
    np.add.at(r, (np.arange(n_out), hi), w_hi)
    return r


def terms(n_in: int, n_out: int):
    """number of products that enter each element: (forward [n_out], adjoint [n_in])"""
    lo, hi, fr = taps(n_in, n_out)
    has_hi = (fr != 0).astype(np.int64)
    adj = np.zeros(n_in, np.int64)
    np.add.at(adj, lo, 1)
    np.add.at(adj, hi, has_hi)
    return 1 + has_hi, adj


def importance_bwd(g_a: np.ndarray, a: np.ndarray, imp: np.ndarray):
    """g_a, a [B, n_s], imp [B, n_t] -> (g_imp [B, n_t], bound [B, n_t]) in float64:
    v = R imp, g_v = (g_a - <a, g_a>) / sum(v), g_imp = R^T g_v; bound = sum_i w_ij |g_v[i]| for the error model"""
    g_a, a, imp = (np.asarray(z, np.float64) for z in (g_a, a, imp))
    n_s, n_t = a.shape[1], imp.shape[1]
    tot = forward(imp[:, :, None], n_s)[:, :, 0].sum(axis=1, keepdims=True)
    g_v = (g_a - (a * g_a).sum(axis=1, keepdims=True)) / tot
    return adjoint(g_v[:, :, None], n_t)[:, :, 0], adjoint(np.abs(g_v)[:, :, None], n_t)[:, :, 0]


def data(shape, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)

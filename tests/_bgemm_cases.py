"""Case tables, dispatch mirror, inputs, long-double reference and the derived bound of tests/test_bgemm_paths_gpu.py:
the fp64 batched GEMM of csrc/bgemm_f64.hip (``basd_bgemm_f64`` / ``basd_bgemm_f64_masked``) on each of its three kernels
-- the element-wise generic kernel, the pipelined fast kernel (wave-uniform 16 x 16 sub-tile skipping, sub-tile mirroring
inside the diagonal tiles of a symmetric product) and the balanced Gram kernel (off-diagonal tiles, 3 / 3 / 2 / 2
diagonal tiles, VALU strip).

``bgemm_path_of`` is a plain-Python copy of the predicate in ``basd_bgemm_f64_masked`` and must be changed together with
it; ``fast_subtile_outcomes``, ``gram_plan``, ``k_plan`` and ``tile_of_block`` copy the index arithmetic of the kernels.
They are bookkeeping -- they say which branches a case reaches, so that the tables cannot drift off the paths they are
there for (pinned by tests/test_bgemm_cases_cpu.py) -- not evidence about the kernels.

The reference is ``np.longdouble`` matmul (x87 extended; ``reference`` refuses to run where long double is no wider than
fp64).  The bound is derived, not measured: for a product accumulated in fp64 in ANY order, with or without fma,

    |c_ij - ref_ij| <= gamma_K (|op A| |op B|)_ij,     gamma_K = K u / (1 - K u),   u = 2^-53

(Higham, Accuracy and Stability of Numerical Algorithms, 3.5).  fp32 operands convert to fp64 exactly, so the bound is
the same for them; an fp32 output adds its one rounding, 2^-24 |ref_ij| (1 + gamma_K).  Where the bound is zero (a zero
row of op(A) or a zero column of op(B)) the output must be zero, of either sign.  A kernel is allowed exactly the bound:
MARGIN = 1.

In symmetric mode the kernels compute the lower triangle (whole diagonal 16 x 16 sub-tiles included) and copy it into the
upper one.  The lower triangle is therefore judged like any product.  Every element (i, j) is also judged against
ref[i, j] with gamma_K max(S_ij, S_ji) + |ref_ij - ref_ji|, which is all that can be asked of a copied element when the
operands make the product symmetric only mathematically (A = X, B = G X: the chain's s_w^T (G_t s_w)).
"""
from __future__ import annotations

import collections
import functools
import zlib

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------------------------
# constants of csrc/bgemm_f64.hip
# ------------------------------------------------------------------------------------------------------------------
TILE = 64                    # BT: output tile of a workgroup
SUBTILE = 16                 # one MFMA output; a wave owns 2 x 2 of them
KCHUNK = 16                  # BK: k extent staged per LDS buffer
KSTEP = 4                    # k extent of one v_mfma_f64_16x16x4_f64
GRAM_RMAX = 8                # strip rows the VALU path of the Gram kernel takes
STRIP_LIMIT = 65536          # bytes of dynamic LDS the strip rows may take: (n % 64) * K * 8 <= STRIP_LIMIT
XCD_DEAL = 8                 # workgroups are dealt round-robin over 8 XCDs: the grid is padded to a multiple of 8 matrices
LDS_STAGE_BYTES = 4 * KCHUNK * (TILE + 2) * 8        # the Gram kernel's two double-buffered operand tiles

F32, F64 = "f32", "f64"
NP_DTYPE = {F32: np.float32, F64: np.float64}
TORCH_DTYPE = {F32: torch.float32, F64: torch.float64}
DTYPE_CODE = {F32: 0, F64: 2}                        # BASD_DTYPE_F32 / BASD_DTYPE_F64
ITEMSIZE = {F32: 4, F64: 8}
DTYPE_TRIPLES = [(a, b, c) for a in (F32, F64) for b in (F32, F64) for c in (F64, F32)]
TRANSPOSES = [(False, False), (True, False), (False, True), (True, True)]

U64 = 2.0 ** -53
U32 = 2.0 ** -24
MARGIN = 1.0

BATCH = 3
MASK_BATCH = 11                                      # > 8 and no multiple of 8: the XCD deal wraps
MASK = {0: 5, 5: -1, 8: 1, 10: 2}                    # skip[b]; any non-zero value masks
C_PAD, C_GAP, C_GUARD = 3, 5, 64                     # ldc = N + C_PAD; c_stride = M ldc + C_GAP; elements behind the last matrix
REGIMES = ["randn", "graded", "cancel"]


# ------------------------------------------------------------------------------------------------------------------
# dispatch mirror
# ------------------------------------------------------------------------------------------------------------------
def bgemm_path_of(*, a_dtype, b_dtype, c_dtype, M, N, K, lda, ldb, a_stride, b_stride, a_off=0, b_off=0, same=False,
                  trans_a=False, trans_b=False, symmetric=False, has_skip=False) -> str:
    """"gram" | "fast" | "generic": the kernel ``basd_bgemm_f64_masked`` launches.  Strides and leading dimensions in
    elements, ``a_off`` / ``b_off``: the base addresses modulo 32 in bytes, ``same``: a and b are one pointer."""
    assert M > 0 and N > 0 and K > 0 and (not symmetric or M == N)
    assert {a_dtype, b_dtype, c_dtype} <= {F32, F64}
    aligned = (M % 4 == 0 and N % 4 == 0 and K % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and a_stride % 4 == 0
               and b_stride % 4 == 0 and a_off % 32 == 0 and b_off % 32 == 0)
    if (symmetric and same and a_dtype == b_dtype and a_stride == b_stride and lda == ldb and not trans_a and trans_b
            and c_dtype == F64 and aligned and not has_skip and M >= TILE and M % TILE <= GRAM_RMAX
            and (M % TILE) * K * 8 <= STRIP_LIMIT):
        return "gram"
    return "fast" if aligned else "generic"


def grid_blocks(batch: int, items: int) -> int:
    return (batch + XCD_DEAL - 1) // XCD_DEAL * XCD_DEAL * items


def tile_of_block(lin: int, M: int, N: int, batch: int):
    """(matrix, m0, n0) of workgroup ``lin`` of the generic and fast kernels, None for a padding workgroup"""
    tn = (N + TILE - 1) // TILE
    tiles = tn * ((M + TILE - 1) // TILE)
    mat = lin // (XCD_DEAL * tiles) * XCD_DEAL + lin % XCD_DEAL
    if mat >= batch:
        return None
    tile = (lin // XCD_DEAL) % tiles
    return mat, tile // tn * TILE, tile % tn * TILE


def fast_subtile_outcomes(M: int, N: int, symmetric: bool) -> collections.Counter:
    """what the fast kernel does with every 16 x 16 sub-tile of its grid (``need[i][j]`` and the store), and with every
    wave ("wave:all" / "wave:some" / "wave:none" of its 2 x 2 sub-tiles need the matrix cores)"""
    out = collections.Counter()
    for m0 in range(0, M, TILE):
        for n0 in range(0, N, TILE):
            if symmetric and n0 > m0:
                out["tile-above-diagonal"] += 1
                continue
            for wm in (0, 32):
                for wn in (0, 32):
                    needed = 0
                    for i in (0, 1):
                        for j in (0, 1):
                            r0, c0 = m0 + wm + i * SUBTILE, n0 + wn + j * SUBTILE
                            if r0 >= M or c0 >= N:
                                out["outside"] += 1
                                continue
                            if symmetric and m0 == n0 and c0 > r0:
                                out["above-diagonal"] += 1
                                continue
                            needed += 1
                            name = ("plain" if not symmetric else "mirrored-tile" if m0 != n0 else
                                    "mirrored-subtile" if c0 < r0 else "diagonal-subtile")
                            out[name + ("+ragged" if r0 + SUBTILE > M or c0 + SUBTILE > N else "")] += 1
                    out["wave:" + ("all" if needed == 4 else "none" if needed == 0 else "some")] += 1
    return out


def k_plan(K: int):
    """(K chunks, k steps of the last chunk) of the fast kernel's loop; the generic and Gram kernels run every chunk in
    full over zero padding"""
    nchunk = (K + KCHUNK - 1) // KCHUNK
    return nchunk, (K - (nchunk - 1) * KCHUNK + KSTEP - 1) // KSTEP


def gram_plan(n: int, K: int) -> dict:
    """work items and dynamic LDS of one matrix of the Gram kernel"""
    nt, rs = n // TILE, n % TILE
    assert nt >= 1 and rs <= GRAM_RMAX and rs * K * 8 <= STRIP_LIMIT
    return {"nt": nt, "rs": rs, "off_diagonal": nt * (nt - 1) // 2, "items": nt * (nt - 1) // 2 + nt + (1 if rs else 0),
            "strip_passes": (n + 255) // 256 if rs else 0, "lds_bytes": max(LDS_STAGE_BYTES, rs * K * 8)}


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
# inputs: "plain" (two independent operands) | "xxt" (B holds the same numbers as A = X [M, K]: C = X X^T, stored for
#         (trans_a, trans_b) = (F, T)) | "xgx" (A = X [K, M], B = G X [K, M] with G symmetric: C = X^T G X, (T, F))
# same:   a and b are ONE device buffer;  bcast: "a" | "b": that operand has one matrix and batch stride 0
# lda_pad / a_stride_pad: elements added to A's natural leading dimension / batch stride;  a_off: bytes between a 32-byte
#         boundary and A's base;  masked: the MASK problem mask, NaN operands in the masked matrices
Case = collections.namedtuple("Case", "path batch M N K ta tb dta dtb dtc sym inputs same bcast lda_pad a_stride_pad a_off "
                                      "masked")


def _c(path, M, N, K, ta=False, tb=False, dt=(F64, F64, F64), batch=BATCH, sym=False, inputs="plain", same=False,
       bcast=None, lda_pad=0, a_stride_pad=0, a_off=0, masked=False) -> Case:
    return Case(path, batch, M, N, K, ta, tb, dt[0], dt[1], dt[2], sym, inputs, same, bcast, lda_pad, a_stride_pad, a_off,
                masked)


def _xxt(path, n, K, dt=(F64, F64, F64), **kw) -> Case:
    return _c(path, n, n, K, False, True, dt, sym=True, inputs="xxt", **kw)


def _xgx(path, n, K, dt) -> Case:
    return _c(path, n, n, K, True, False, dt, sym=True, inputs="xgx")


def case_id(c: Case) -> str:
    s = f"{c.path}-{c.M}x{c.N}x{c.K}-{'T' if c.ta else 'N'}{'T' if c.tb else 'N'}-{c.dta}.{c.dtb}.{c.dtc}"
    if c.batch != BATCH:
        s += f"-b{c.batch}"
    if c.sym:
        s += "-sym-" + c.inputs + ("-same" if c.same else "")
    for flag, text in ((c.bcast, f"bcast_{c.bcast}"), (c.lda_pad, f"lda+{c.lda_pad}"),
                       (c.a_stride_pad, f"stride+{c.a_stride_pad}"), (c.a_off, f"base+{c.a_off}"), (c.masked, "masked")):
        if flag:
            s += "-" + text
    return s


F32_IN, F32_ALL, F64_F32 = (F32, F32, F64), (F32, F32, F32), (F64, F64, F32)

GENERIC_CASES = (
    [_c("generic", 1, 1, 1)]
    + [_c("generic", 65, 63, 17, ta, tb, (F32, F64, F64)) for ta, tb in TRANSPOSES]
    + [_c("generic", 70, 130, 53, ta, tb, dt) for ta, tb in TRANSPOSES for dt in (F32_IN, F64_F32)]
    + [_xxt("generic", 70, 18), _xxt("generic", 70, 18, F32_IN, same=True)])
# the aligned shape of FAST_TWIN pushed off the fast path, one arm of the alignment predicate at a time
FAST_TWIN = _c("fast", 68, 72, 20, dt=F32_IN)
KNOCKED_OFF = [_c("generic", 68, 72, 20, dt=F32_IN, lda_pad=2), _c("generic", 68, 72, 20, dt=F32_IN, a_stride_pad=2),
               _c("generic", 68, 72, 20, dt=F32_IN, a_off=16)]

FAST_CASES = (
    [_c("fast", 68, 72, 20, ta, tb, dt) for ta, tb in TRANSPOSES for dt in DTYPE_TRIPLES]
    + [_c("fast", 68, 132, K, t, t, dt) for K in (4, 16, 36) for t, dt in ((False, (F64, F64, F64)), (True, F32_IN))]
    + [_c("fast", 196, 192, 196, dt=F32_IN), _c("fast", 196, 192, 196, dt=F32_ALL)]
    + [_c("fast", 68, 72, 20, dt=(F32, F64, F64), bcast="a"), _c("fast", 68, 72, 20, dt=(F32, F64, F64), bcast="b")])
assert FAST_TWIN in FAST_CASES
BROADCAST_CASES = [c for c in FAST_CASES if c.bcast]

FAST_SYM_SIZES = [64, 68, 80, 84, 132, 196, 204]
FAST_SYM_CASES = ([_xxt("fast", n, 20) for n in FAST_SYM_SIZES] + [_xxt("fast", 196, 20, F32_IN), _xxt("fast", 68, 20, F32_ALL)])
# (f32, f32): G X rounded to fp32 is 2^-24 away from symmetric, far above gamma_K: the regime in which a kernel that
# computed the upper triangle and copied it down would show.  (f32, f64) is the chain's own form.
XGX_CASES = [_xgx("fast", 68, 20, F32_IN), _xgx("fast", 196, 20, (F32, F64, F64)), _xgx("fast", 196, 20, F32_IN)]

MASKED_CASES = [_c("generic", 70, 130, 53, dt=F32_IN, batch=MASK_BATCH, masked=True),
                _c("fast", 68, 72, 20, dt=F32_IN, batch=MASK_BATCH, masked=True),
                _xxt("fast", 196, 20, F32_IN, batch=MASK_BATCH, masked=True, same=True)]      # the _psd_eig_blocked form

GRAM_SIZES = [64, 68, 72, 132, 196, 260]
GRAM_CASES = ([_xxt("gram", n, 20, dt, same=True) for n in GRAM_SIZES for dt in (F32_IN, (F64, F64, F64))]
              + [_xxt("gram", 196, 768, F32_IN, same=True, batch=9), _xxt("gram", 68, 4, same=True)])
# both sides of the strip limit (72 x 1024: exactly 64 KiB of dynamic LDS) and of GRAM_RMAX (76: 12 strip rows)
GRAM_BOUNDARY = [_xxt("gram", 72, 1024, F32_IN, same=True), _xxt("fast", 72, 1028, F32_IN, same=True),
                 _xxt("fast", 76, 20, F32_IN, same=True)]

ALL_CASES = (GENERIC_CASES + KNOCKED_OFF + FAST_CASES + FAST_SYM_CASES + XGX_CASES + MASKED_CASES + GRAM_CASES
             + GRAM_BOUNDARY)
SAME_TENSOR_CASES = [c for c in ALL_CASES if c.same]
assert len(set(ALL_CASES)) == len(ALL_CASES)


def regimes(c: Case):
    """cancel pairs the two K halves of two independent operands"""
    return [r for r in REGIMES if r != "cancel" or (c.inputs == "plain" and c.K % 2 == 0)]


def label(c: Case) -> str:
    """the row of the margins table a case reports to"""
    return c.path + ("-sym" if c.sym and c.path != "gram" else "")      # the Gram kernel is symmetric by definition


# ------------------------------------------------------------------------------------------------------------------
# layout: where the matrices lie in the three buffers
# ------------------------------------------------------------------------------------------------------------------
Layout = collections.namedtuple("Layout", "a_shape lda a_stride a_lead a_batch b_shape ldb b_stride b_batch ldc c_stride")


def layout(c: Case) -> Layout:
    a_shape = (c.K, c.M) if c.ta else (c.M, c.K)
    b_shape = (c.N, c.K) if c.tb else (c.K, c.N)
    a_batch = 1 if c.bcast == "a" else c.batch
    b_batch = 1 if c.bcast == "b" else c.batch
    lda, ldb = a_shape[1] + c.lda_pad, b_shape[1]
    a_stride = 0 if c.bcast == "a" else a_shape[0] * lda + c.a_stride_pad
    b_stride = 0 if c.bcast == "b" else b_shape[0] * ldb
    assert c.a_off % ITEMSIZE[c.dta] == 0
    ldc = c.N + C_PAD
    return Layout(a_shape, lda, a_stride, c.a_off // ITEMSIZE[c.dta], a_batch, b_shape, ldb, b_stride, b_batch, ldc,
                  c.M * ldc + C_GAP)


def path_of(c: Case) -> str:
    lay = layout(c)
    return bgemm_path_of(a_dtype=c.dta, b_dtype=c.dtb, c_dtype=c.dtc, M=c.M, N=c.N, K=c.K, lda=lay.lda, ldb=lay.ldb,
                         a_stride=lay.a_stride, b_stride=lay.b_stride, a_off=c.a_off, b_off=0, same=c.same,
                         trans_a=c.ta, trans_b=c.tb, symmetric=c.sym, has_skip=c.masked)


def skip_mask(c: Case):
    """int32 [batch] or None"""
    if not c.masked:
        return None
    m = np.zeros(c.batch, dtype=np.int32)
    for b, v in MASK.items():
        m[b] = v
    return m


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _rounded(x, dt):
    return np.asarray(x, dtype=NP_DTYPE[dt]).astype(np.float64)


def _grades(rng, batch, n):
    """[batch, n] scales 10^U(-8, 0) with three exact zeros per matrix (none where n < 8)"""
    s = 10.0 ** rng.uniform(-8.0, 0.0, (batch, n))
    if n >= 8:
        for b in range(batch):
            s[b, rng.choice(n, 3, replace=False)] = 0.0
    return s


@functools.lru_cache(maxsize=None)
def operands(c: Case, regime: str):
    """(op(A) [a_batch, M, K], op(B) [b_batch, K, N]) as fp64 arrays whose values the operand dtypes hold exactly"""
    assert regime in regimes(c)
    lay = layout(c)
    rng = np.random.default_rng(zlib.crc32((case_id(c) + regime).encode()))
    if c.inputs == "xgx":                                                # X [K, M], G [K, K]
        x = rng.standard_normal((c.batch, c.K, c.M))
        if regime == "graded":
            x = x * _grades(rng, c.batch, c.M)[:, None, :]
        x = _rounded(x, c.dta)
        g = rng.standard_normal((c.batch, c.K, c.K))
        g = g + g.transpose(0, 2, 1)
        gx = _rounded(np.matmul(g.astype(np.longdouble), x.astype(np.longdouble)), c.dtb)
        out = np.ascontiguousarray(x.transpose(0, 2, 1)), gx
    elif c.inputs == "xxt":
        assert c.dta == c.dtb and c.M == c.N
        x = rng.standard_normal((c.batch, c.M, c.K))
        if regime == "graded":
            x = x * _grades(rng, c.batch, c.M)[:, :, None]
        x = _rounded(x, c.dta)
        out = x, np.ascontiguousarray(x.transpose(0, 2, 1))
    else:
        a = rng.standard_normal((lay.a_batch, c.M, c.K))
        b = rng.standard_normal((lay.b_batch, c.K, c.N))
        if regime == "graded":
            a = a * _grades(rng, lay.a_batch, c.M)[:, :, None]
            b = b * _grades(rng, lay.b_batch, c.N)[:, None, :]
        a, b = _rounded(a, c.dta), _rounded(b, c.dtb)
        if regime == "cancel":
            h = c.K // 2
            a[:, :, h:] = a[:, :, :h]
            b[:, h:, :] = _rounded(-(1.0 + 2.0 ** -20) * b[:, :h, :], c.dtb)
        out = a, b
    for t in out:
        t.setflags(write=False)
    return out


def stored(c: Case, which: str, op) -> torch.Tensor:
    """the flat buffer of operand ``which`` ("a" | "b") as the entry reads it: ``a_lead`` elements in front of the base,
    the matrices at their strides; every element the entry has no business reading is NaN, and so are the matrices of
    masked problems"""
    lay = layout(c)
    if which == "a":
        shape, ld, stride, lead, batch, dt, tr = lay.a_shape, lay.lda, lay.a_stride, lay.a_lead, lay.a_batch, c.dta, c.ta
    else:
        shape, ld, stride, lead, batch, dt, tr = lay.b_shape, lay.ldb, lay.b_stride, 0, lay.b_batch, c.dtb, c.tb
    mats = np.asarray(op).transpose(0, 2, 1) if tr else np.asarray(op)           # trans_x: the stored matrix is op(X)^T
    assert mats.shape == (batch,) + shape
    one = shape[0] * ld
    buf = np.full(lead + (batch - 1) * stride + one + 64, np.nan)
    mask = skip_mask(c)
    for b in range(batch):
        m = buf[lead + b * stride: lead + b * stride + one].reshape(shape[0], ld)
        if mask is None or mask[b] == 0:
            m[:, :shape[1]] = mats[b]
    return torch.from_numpy(buf).to(TORCH_DTYPE[dt])


# ------------------------------------------------------------------------------------------------------------------
# reference and bound
# ------------------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "ref S")


@functools.lru_cache(maxsize=None)
def reference(c: Case, regime: str) -> Reference:
    """long double op(A) op(B) and |op(A)| |op(B)|, both [batch, M, N]; computed once per case and regime, read-only"""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than fp64 here: no reference to judge with"
    a, b = (t.astype(np.longdouble) for t in operands(c, regime))
    ref = np.broadcast_to(np.matmul(a, b), (c.batch, c.M, c.N))
    S = np.broadcast_to(np.matmul(np.abs(a), np.abs(b)), (c.batch, c.M, c.N))
    for t in (ref, S):
        t.setflags(write=False)
    return Reference(ref, S)


def gamma(K: int):
    k = np.longdouble(K) * np.longdouble(U64)
    return k / (1 - k)


def elementwise_bound(ref, S, K: int, dtc: str, symmetric: bool = False):
    """the bound on |c - ref|, long double, the shape of ref; ``symmetric``: the form for a copied element"""
    g = gamma(K)
    if symmetric:
        rt = np.swapaxes(ref, -1, -2)
        bound = g * np.maximum(S, np.swapaxes(S, -1, -2)) + np.abs(ref - rt)
    else:
        bound = g * S
    if dtc == F32:
        bound = bound + np.longdouble(U32) * np.abs(ref) * (1 + g)
    return bound


def _ratio(c, ref, bound, where=None) -> float:
    """largest |c - ref| / bound; inf where the bound is zero and c is not, and for a NaN"""
    c = np.asarray(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(c.astype(np.longdouble) - ref)
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(c == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    if where is not None:
        q = q[..., where]
    return float(q.max(initial=0.0))


def judge(c: Case, regime: str, out, matrices=None) -> dict:
    """name -> worst err / bound of ``out`` [batch, M, N] (numpy, the output dtype) over ``matrices`` (default: those the
    mask leaves).  "elem": every element; in symmetric mode "lower" is the computed triangle under the plain bound and
    "elem" the whole matrix under the bound of a copied element."""
    r = reference(c, regime)
    mask = skip_mask(c)
    if matrices is None:
        matrices = [b for b in range(c.batch) if mask is None or mask[b] == 0]
    out, ref, S = np.asarray(out)[matrices], r.ref[matrices], r.S[matrices]
    if not c.sym:
        return {"elem": _ratio(out, ref, elementwise_bound(ref, S, c.K, c.dtc))}
    low = np.tril(np.ones((c.M, c.M), dtype=bool))
    return {"elem": _ratio(out, ref, elementwise_bound(ref, S, c.K, c.dtc, symmetric=True)),
            "lower": _ratio(out, ref, elementwise_bound(ref, S, c.K, c.dtc), where=low)}

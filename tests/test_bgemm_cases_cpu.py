"""The cases, the reference and the bound of tests/test_bgemm_paths_gpu.py can tell a right fp64 batched GEMM from a
nearly right one (no GPU needed).

tests/_bgemm_cases.py mirrors the dispatch of ``basd_bgemm_f64_masked`` and holds the case tables, the inputs, the
long-double reference and the componentwise bound.  Here: every case takes the path it names and the tables reach every
branch the kernels have (each arm of the alignment predicate, every outcome of the fast kernel's sub-tile logic, the
ragged K chunks, both sides of the Gram kernel's limits, the second pass of its strip loop, the wrap of the XCD deal);
correct fp64 products (numpy, tests/_emul.py) stay inside the bound on every case and regime; wrong ones -- an operand
rounded to fp32, fp32 accumulation, a dropped k step, a sub-tile left zero, the wrong triangle mirrored -- leave it;
and the entry's refusals, which return before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _bgemm_cases as C
from tests import _emul

_FIGURES = {}        # (what, label, output dtype, regime) -> (ratio, case id)


def _note(what, c, regime, v, worst=max):
    key = (what, C.label(c), c.dtc, regime)
    if key not in _FIGURES or worst(v, _FIGURES[key][0]) == v:
        _FIGURES[key] = (v, C.case_id(c))


def test_long_double_is_wider_than_fp64():
    assert np.finfo(np.longdouble).eps < 1e-18


# ------------------------------------------------------------------------------------------------------------------
# the mirror and the tables
# ------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    import basd_amd._native as native
    src = open(__import__("os").path.join(native.CSRC, "bgemm_f64.hip")).read()
    for text in (f"constexpr int BT = {C.TILE};", f"constexpr int BK = {C.KCHUNK};", f"constexpr int GRAM_RMAX = {C.GRAM_RMAX};",
                 f"(size_t)(M % 64) * K * 8 <= {C.STRIP_LIMIT}", "mfma_f64_16x16x4f64",
                 f"(lin / ({C.XCD_DEAL} * tiles)) * {C.XCD_DEAL} + (lin & {C.XCD_DEAL - 1})"):
        assert text in src, text
    assert C.LDS_STAGE_BYTES == 33792 and C.SUBTILE * 4 == C.TILE and C.KSTEP * 4 == C.KCHUNK


def test_every_case_takes_the_path_it_names():
    for c in C.ALL_CASES:
        assert C.path_of(c) == c.path, C.case_id(c)
    assert {c.path for c in C.ALL_CASES} == {"gram", "fast", "generic"}
    assert len({C.case_id(c) for c in C.ALL_CASES}) == len(C.ALL_CASES)
    # the knocked-off cases: the fast twin with ONE field changed
    assert C.path_of(C.FAST_TWIN) == "fast"
    changed = [{f for f in C.Case._fields if getattr(c, f) != getattr(C.FAST_TWIN, f)} for c in C.KNOCKED_OFF]
    assert changed == [{"path", "lda_pad"}, {"path", "a_stride_pad"}, {"path", "a_off"}]
    lay = [C.layout(c) for c in C.KNOCKED_OFF]
    assert lay[0].lda == 20 + 2 and lay[1].a_stride == 68 * 20 + 2 and lay[2].a_lead * 4 == 16
    # every dtype triple and transpose on the fast kernel; both outputs at the chain's largest product
    assert {(c.ta, c.tb, c.dta, c.dtb, c.dtc) for c in C.FAST_CASES if (c.M, c.N, c.K) == (68, 72, 20) and not c.bcast} == \
        {(ta, tb) + dt for ta, tb in C.TRANSPOSES for dt in C.DTYPE_TRIPLES}
    assert {c.dtc for c in C.FAST_CASES if (c.M, c.N, c.K) == (196, 192, 196)} == {C.F32, C.F64}
    assert {c.bcast for c in C.BROADCAST_CASES} == {"a", "b"}
    assert all(C.layout(c).a_stride == 0 or C.layout(c).b_stride == 0 for c in C.BROADCAST_CASES)
    # generic: one element, ragged in every dimension, more than one tile, symmetric
    assert {(c.M, c.N, c.K) for c in C.GENERIC_CASES} == {(1, 1, 1), (65, 63, 17), (70, 130, 53), (70, 70, 18)}
    # symmetric, fast, TWO buffers, both operand forms
    assert {c.M for c in C.FAST_SYM_CASES} == set(C.FAST_SYM_SIZES) and not any(c.same for c in C.FAST_SYM_CASES + C.XGX_CASES)
    assert {(c.M, c.ta, c.tb) for c in C.XGX_CASES} == {(68, True, False), (196, True, False)}
    # masked: one per kernel that takes a mask; the shared-pointer Gram form must NOT reach the Gram kernel
    assert [(c.path, c.sym, c.same) for c in C.MASKED_CASES] == [("generic", False, False), ("fast", False, False),
                                                                 ("fast", True, True)]
    assert C.path_of(C.MASKED_CASES[2]._replace(masked=False)) == "gram"
    assert [C.path_of(c) for c in C.GRAM_BOUNDARY] == ["gram", "fast", "fast"]
    assert [(c.M, c.K) for c in C.GRAM_BOUNDARY] == [(72, 1024), (72, 1028), (76, 20)]


def test_each_arm_of_the_predicates_decides():
    base = dict(a_dtype=C.F32, b_dtype=C.F32, c_dtype=C.F64, M=68, N=72, K=20, lda=20, ldb=72, a_stride=1360, b_stride=1440)
    assert C.bgemm_path_of(**base) == "fast"
    for arm in (dict(M=70), dict(N=70), dict(K=18, lda=18), dict(lda=22), dict(ldb=74), dict(a_stride=1362),
                dict(b_stride=1442), dict(a_off=16), dict(b_off=8), dict(a_off=4)):
        assert C.bgemm_path_of(**{**base, **arm}) == "generic", arm
    assert C.bgemm_path_of(**{**base, "a_off": 32, "b_off": 64, "a_stride": 0}) == "fast"
    gram = dict(a_dtype=C.F32, b_dtype=C.F32, c_dtype=C.F64, M=72, N=72, K=1024, lda=1024, ldb=1024, a_stride=72 * 1024,
                b_stride=72 * 1024, same=True, trans_b=True, symmetric=True)
    assert C.bgemm_path_of(**gram) == "gram"
    for arm in (dict(same=False), dict(symmetric=False), dict(has_skip=True), dict(c_dtype=C.F32), dict(trans_a=True),
                dict(trans_b=False), dict(M=76, N=76), dict(M=60, N=60), dict(K=1028, lda=1028, ldb=1028),
                dict(b_dtype=C.F64), dict(b_stride=72 * 1024 + 4), dict(ldb=1028)):
        assert C.bgemm_path_of(**{**gram, **arm}) == "fast", arm
    assert C.bgemm_path_of(**{**gram, "a_off": 16, "b_off": 16}) == "generic"


def test_symmetric_fast_cases_reach_every_subtile_outcome():
    sym = [c for c in C.ALL_CASES if c.path == "fast" and c.sym]
    reached = {}
    for c in sym:
        for name in C.fast_subtile_outcomes(c.M, c.N, True):
            reached.setdefault(name, set()).add(c.M)
    assert set(reached) == {"tile-above-diagonal", "outside", "above-diagonal", "mirrored-tile", "mirrored-tile+ragged",
                            "mirrored-subtile", "mirrored-subtile+ragged", "diagonal-subtile", "diagonal-subtile+ragged",
                            "wave:all", "wave:some", "wave:none"}, sorted(reached)
    assert reached["mirrored-subtile+ragged"] == {84} and reached["diagonal-subtile+ragged"] >= {68, 132, 196, 204}
    assert 64 not in reached["outside"] and 64 not in reached["tile-above-diagonal"]
    # training's shape: three full tile rows and a fourth of four rows
    o = C.fast_subtile_outcomes(196, 196, True)
    assert o["tile-above-diagonal"] == 6 and o["mirrored-tile+ragged"] == 12 and o["diagonal-subtile+ragged"] == 1
    assert o["mirrored-tile"] + o["mirrored-tile+ragged"] + o["mirrored-subtile"] + o["diagonal-subtile"] + 1 == 91
    plain = set()
    for c in C.FAST_CASES:
        plain |= set(C.fast_subtile_outcomes(c.M, c.N, False))
    assert plain == {"plain", "plain+ragged", "outside", "wave:all", "wave:some", "wave:none"}


def test_k_loops_and_gram_items_are_covered():
    fast = {C.k_plan(c.K) for c in C.ALL_CASES if c.path == "fast"}
    # one chunk ragged / full, an even and an odd number of chunks (both LDS buffers last), the chain's 196
    assert fast >= {(1, 1), (1, 4), (2, 1), (3, 1), (13, 1)}
    assert {c.K for c in C.ALL_CASES if c.path == "generic"} >= {1, 17, 18, 20, 53}
    gram = [c for c in C.ALL_CASES if c.path == "gram"]
    plans = {(c.M, c.K): C.gram_plan(c.M, c.K) for c in gram}
    assert {p["rs"] for p in plans.values()} == {0, 4, 8} and {p["strip_passes"] for p in plans.values()} == {0, 1, 2}
    assert {p["off_diagonal"] for p in plans.values()} >= {0, 1, 3, 6}
    assert plans[(260, 20)]["strip_passes"] == 2 and plans[(260, 20)]["rs"] == 4
    assert plans[(72, 1024)]["lds_bytes"] == C.STRIP_LIMIT == 65536
    assert plans[(196, 768)]["lds_bytes"] == C.LDS_STAGE_BYTES            # the strip rows fit the staging buffers
    assert any(c.K < C.KCHUNK for c in gram) and {c.dta for c in gram} == {C.F32, C.F64}
    assert max(c.batch * c.M * c.K for c in C.ALL_CASES) <= 11 * 196 * 768


def test_masked_batch_wraps_the_xcd_deal():
    assert C.MASK_BATCH > C.XCD_DEAL and C.MASK_BATCH % C.XCD_DEAL
    assert min(C.MASK) == 0 and max(C.MASK) == C.MASK_BATCH - 1 and any(b >= C.XCD_DEAL for b in C.MASK)
    assert all(v != 0 for v in C.MASK.values()) and {v for v in C.MASK.values()} >= {-1, 1}
    for c in C.MASKED_CASES:
        tiles = ((c.M + 63) // 64) * ((c.N + 63) // 64)
        blocks = C.grid_blocks(c.batch, tiles)
        assert blocks == 16 * tiles
        seen = {}
        idle = 0
        for lin in range(blocks):
            t = C.tile_of_block(lin, c.M, c.N, c.batch)
            if t is None:
                idle += 1
                continue
            seen.setdefault(t[0], set()).add(t[1:])
            assert (t[0] >= C.XCD_DEAL) == (lin >= C.XCD_DEAL * tiles)
        assert sorted(seen) == list(range(c.batch)) and all(len(v) == tiles for v in seen.values())
        assert idle == (16 - c.batch) * tiles
        assert C.skip_mask(c).tolist() == [5, 0, 0, 0, 0, -1, 0, 0, 1, 0, 2]


def test_inputs_are_what_the_regimes_say():
    c = C.FAST_TWIN
    a, b = C.operands(c, "graded")
    assert [int((np.abs(a[i]).max(axis=1) == 0).sum()) for i in range(c.batch)] == [3] * c.batch
    assert [int((np.abs(b[i]).max(axis=0) == 0).sum()) for i in range(c.batch)] == [3] * c.batch
    r = C.reference(c, "graded")
    assert int((r.S == 0).sum()) == c.batch * (3 * c.N + 3 * c.M - 9)
    row = np.abs(a).max(axis=2)
    assert float(row[row > 0].min()) < 1e-5 and float(row.max()) > 1e-2          # graded over orders of magnitude
    a, b = C.operands(c, "cancel")
    assert np.array_equal(a[:, :, 10:], a[:, :, :10]) and not np.array_equal(b[:, 10:], -b[:, :10])
    r = C.reference(c, "cancel")
    q = np.abs(r.ref) / r.S
    assert float(np.median(q)) < 2.0 ** -20 and float(q.max()) < 2.0 ** -18
    for t, dt in zip(C.operands(C.FAST_CASES[0], "randn"), (C.FAST_CASES[0].dta, C.FAST_CASES[0].dtb)):
        assert np.array_equal(t, t.astype(C.NP_DTYPE[dt]).astype(np.float64))
    # X / G X: symmetric mathematically only; with G X in fp32 the asymmetry is far above gamma_K S, in fp64 far below
    big = {}
    for c in C.XGX_CASES:
        for regime in C.regimes(c):
            r = C.reference(c, regime)
            asym = np.abs(r.ref - r.ref.transpose(0, 2, 1))
            gs = C.gamma(c.K) * r.S
            assert float(asym.max()) > 0
            big[(c.M, c.dtb, regime)] = float(np.median((asym / np.where(gs > 0, gs, 1))[gs > 0]))
    assert all((v > 1e3) == (dtb == C.F32) for (_m, dtb, _r), v in big.items()), big
    assert "cancel" not in C.regimes(C.XGX_CASES[0]) and "cancel" not in C.regimes(C.GENERIC_CASES[0])
    assert C.regimes(C.FAST_TWIN) == C.REGIMES
    # stored(): the transposes, the padding, the masked matrices
    c = C.KNOCKED_OFF[0]._replace(ta=True)
    a, _b = C.operands(c, "randn")
    buf = C.stored(c, "a", a)
    lay = C.layout(c)
    m1 = buf[lay.a_stride: lay.a_stride + c.K * lay.lda].view(c.K, lay.lda)
    assert buf.dtype == torch.float32 and np.array_equal(m1[:, :c.M].double().numpy(), a[1].T) and bool(m1[:, c.M:].isnan().all())
    c = C.MASKED_CASES[1]
    buf = C.stored(c, "b", C.operands(c, "randn")[1]).view(-1)[:c.batch * c.K * c.N].view(c.batch, -1)
    assert [bool(buf[i].isnan().all()) for i in range(c.batch)] == [bool(v) for v in C.skip_mask(c)]
    assert not bool(buf[[i for i in range(c.batch) if not C.skip_mask(c)[i]]].isnan().any())


# ------------------------------------------------------------------------------------------------------------------
# right products stay inside the bound, wrong ones leave it
# ------------------------------------------------------------------------------------------------------------------
def _cast(c, x):
    return np.asarray(x).astype(C.NP_DTYPE[c.dtc])


def _worst(c, regime, out) -> float:
    return max(C.judge(c, regime, out).values())


@pytest.mark.parametrize("c", C.ALL_CASES, ids=C.case_id)
def test_fp64_products_stay_inside_the_bound(c):
    mask = C.skip_mask(c)
    for regime in C.regimes(c):
        a, b = C.operands(c, regime)
        got = _worst(c, regime, _cast(c, np.matmul(a, b)))
        _note("numpy-fp64", c, regime, got)
        assert got <= C.MARGIN, (regime, got)
        # the emulation the CPU suite runs the loss on, fed the stored forms
        sa = torch.tensor(a.transpose(0, 2, 1) if c.ta else a).to(C.TORCH_DTYPE[c.dta])
        sb = torch.tensor(b.transpose(0, 2, 1) if c.tb else b).to(C.TORCH_DTYPE[c.dtb])
        out = _emul.bgemm_f64(sa, sb, trans_a=c.ta, trans_b=c.tb, out_dtype=C.TORCH_DTYPE[c.dtc], symmetric=c.sym,
                              skip=None if mask is None else torch.from_numpy(mask))
        assert out.dtype == C.TORCH_DTYPE[c.dtc] and tuple(out.shape) == (c.batch, c.M, c.N)
        if mask is not None:
            assert [bool(out[i].isnan().all()) for i in range(c.batch)] == [bool(v) for v in mask]
        got = _worst(c, regime, out.numpy())
        _note("emul", c, regime, got)
        assert got <= C.MARGIN, (regime, got)


def _f32(x):
    return x.astype(np.float32).astype(np.float64)


def _rounded_operand(c, a, b):
    """the fp64 operand (A if both are) rounded to fp32 on the way in"""
    return np.matmul(_f32(a), b) if c.dta == C.F64 else np.matmul(a, _f32(b))


def _f32_accumulation(c, a, b):
    """products and sums in fp32, one k at a time as a matrix core would"""
    acc = np.zeros((c.batch, c.M, c.N), dtype=np.float32)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    for k in range(c.K):
        acc = acc + a32[:, :, k:k + 1] * b32[:, k:k + 1, :]
    return acc


def _dropped_k_step(c, a, b):
    kept = (c.K - 1) // C.KSTEP * C.KSTEP
    return np.matmul(a[:, :, :kept], b[:, :kept, :])


def _zero_subtile(c, a, b):
    """the last row of sub-tiles: its last sub-tile, or in symmetric mode its first with the mirror image"""
    out = np.matmul(a, b)
    r0 = (c.M - 1) // C.SUBTILE * C.SUBTILE
    c0 = 0 if c.sym else (c.N - 1) // C.SUBTILE * C.SUBTILE
    out[:, r0:r0 + C.SUBTILE, c0:c0 + C.SUBTILE] = 0
    if c.sym:
        out[:, c0:c0 + C.SUBTILE, r0:r0 + C.SUBTILE] = 0
    return out


def _upper_mirrored(c, a, b):
    out = np.matmul(a, b)
    up = np.triu(out)
    return up + np.triu(out, 1).transpose(0, 2, 1)


def _shows(name, c, regime) -> bool:
    """can this wrong kernel leave the bound on this case at all?"""
    if name == "rounded-operand":
        # an fp32 operand is not changed; under an fp32 output the damage competes with the output's own rounding
        # unless the product cancels (|ref| << S)
        return C.F64 in (c.dta, c.dtb) and (c.dtc == C.F64 or regime == "cancel")
    if name == "f32-accumulation":
        return c.K > 1 and (c.dtc == C.F64 or regime == "cancel")
    if name == "upper-mirrored":
        return c.inputs == "xgx" and c.dtb == C.F32      # an fp64 G X is symmetric to below gamma_K S
    return True


_MUTANTS = {"rounded-operand": _rounded_operand, "f32-accumulation": _f32_accumulation, "dropped-k-step": _dropped_k_step,
            "zero-subtile": _zero_subtile, "upper-mirrored": _upper_mirrored}
_MUTANT_CASES = [c for c in C.ALL_CASES if c.batch * c.M * c.N * c.K <= 3 * 196 * 192 * 196 and c.K <= 196]


@pytest.mark.parametrize("name", list(_MUTANTS))
def test_wrong_products_leave_the_bound(name):
    shown = set()
    for c in _MUTANT_CASES:
        for regime in C.regimes(c):
            if not _shows(name, c, regime):
                continue
            a, b = (np.broadcast_to(t, (c.batch,) + t.shape[1:]) for t in C.operands(c, regime))
            got = _worst(c, regime, _cast(c, _MUTANTS[name](c, a, b)))
            _note("mutant " + name, c, regime, got, worst=min)
            assert got > C.MARGIN, (name, C.case_id(c), regime, got)
            shown.add((C.label(c), regime))
    if name == "upper-mirrored":
        assert shown == {("fast-sym", "randn"), ("fast-sym", "graded")}
        return
    want = {(lab, r) for lab in ("generic", "generic-sym", "fast", "fast-sym", "gram") for r in ("randn", "graded")}
    want |= {("fast", "cancel")} | ({("generic", "cancel")} if name != "rounded-operand" else set())
    assert shown >= want, sorted(want - shown)


def test_the_lower_triangle_is_what_catches_the_wrong_mirror():
    """under the bound of a copied element alone, a kernel that computed the upper triangle passes: the plain bound on
    the computed (lower) triangle is the check that binds the callers' contract"""
    c = C.XGX_CASES[0]
    a, b = C.operands(c, "randn")
    got = C.judge(c, "randn", _upper_mirrored(c, a, b))
    assert got["elem"] <= C.MARGIN < got["lower"]
    right = np.matmul(a, b)
    low = np.tril(right) + np.tril(right, -1).transpose(0, 2, 1)
    got = C.judge(c, "randn", low)
    assert got["elem"] <= C.MARGIN and got["lower"] <= C.MARGIN


def test_exact_zeros_are_demanded_where_the_bound_is_zero():
    c = C.FAST_TWIN
    a, b = C.operands(c, "graded")
    out = np.matmul(a, b)
    r = C.reference(c, "graded")
    i, j = np.argwhere(r.S[0] == 0)[0]
    assert out[0, i, j] == 0
    for v, ok in ((-0.0, True), (5e-324, False), (np.nan, False)):
        bad = out.copy()
        bad[0, i, j] = v
        assert (_worst(c, "graded", bad) <= C.MARGIN) == ok, v
    bad = out.copy()
    bad[1, 5, 7] = np.nan                                                  # a NaN anywhere is outside every bound
    assert _worst(c, "graded", bad) == float("inf")


def test_report_reference_figures():
    """runs after the tests above: the worst err / bound per path and regime of correct fp64 products, and the smallest
    of each wrong one, for the record (pytest -s)"""
    for (what, lab, dtc, regime), (v, where) in sorted(_FIGURES.items()):
        print(f"bgemm-f64-ref {what} {lab} ->{dtc} {regime}: {v:.3g} at {where}")


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
BASD_OK, BASD_ERR_SHAPE, BASD_ERR_DTYPE = 0, 1, 4


def _call(entries, p, q, *, dt=(0, 0, 2), batch=3, M=8, N=8, K=8, sym=0, masked=False):
    i64 = ctypes.c_int64
    args = (p, dt[0], i64(64), 8, 0, q, dt[1], i64(64), 8, 0, p, dt[2], i64(64), 8, batch, M, N, K, sym)
    if masked:
        return entries.basd_bgemm_f64_masked(*args, p, _NULL)
    return entries.basd_bgemm_f64(*args, _NULL)


@pytest.mark.parametrize("masked", [False, True])
def test_bgemm_refuses_bad_shapes_and_dtypes(entries, masked):
    """host buffers behind the pointers: nothing may be read or written through them"""
    t = torch.full((2, 4096), -7.0, dtype=torch.float64)
    p, q = ctypes.c_void_p(t[0].data_ptr()), ctypes.c_void_p(t[1].data_ptr())
    assert _call(entries, p, q, M=8, N=4, sym=1, masked=masked) == BASD_ERR_SHAPE
    assert entries.basd_last_error() == b"bgemm_f64: symmetric needs M == N"
    for K in (0, -4):
        assert _call(entries, p, q, K=K, masked=masked) == BASD_ERR_SHAPE
        assert entries.basd_last_error() == f"bgemm_f64: bad shape batch=3 K={K}".encode()
    for dt in ((1, 0, 2), (0, 1, 2), (0, 0, 1), (2, 2, 1), (3, 0, 0)):       # BASD_DTYPE_BF16 = 1 is no operand here
        assert _call(entries, p, q, dt=dt, masked=masked) == BASD_ERR_DTYPE
        assert entries.basd_last_error() == f"bgemm_f64: dtype combination a={dt[0]} b={dt[1]} c={dt[2]}".encode()
    # an empty problem is a no-op, whatever else is wrong with it
    assert _call(entries, p, q, batch=0, K=0, masked=masked) == BASD_OK
    assert _call(entries, p, q, M=0, dt=(1, 1, 1), masked=masked) == BASD_OK
    assert bool((t == -7).all())

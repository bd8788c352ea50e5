"""The weight-gradient kernels of csrc/vit_gemm.hip (register kernel KT = 4 / 8 / 12, LDS-DMA ring kernel with its
workspace + reduce and its atomic epilogue, the launcher's M % 64 tail) on every dispatch path (GPU box only).
tests/_wgrad_cases.py holds the case list and says which path each case reaches (pinned by
tests/test_wgrad_cases_cpu.py).

  1. exact accumulation into views of a flat buffer, integer regime: no tolerance at all; on the workspace entry the
     workspace is exactly as long as asked for and NaN-filled, sentinels around everything;
  2. two ring shapes back to back on one workspace;
  3. db == nullptr;
  4. the Python entry, with and without out_w / out_b;
  5. real regime against fp64, element by element, with the tolerance derived in tests/_wgrad_cases.py;
  6. refusals.

Every ring case runs through both C entries: ``basd_wgrad_bf16_ws`` (partial tiles + reduce) and ``basd_wgrad_bf16``
(fp32 atomics from the ring kernel), which the Python entry never reaches on a ring shape.
"""
import ctypes

import pytest
import torch

from tests import _wgrad_cases as C

pytestmark = pytest.mark.gpu

BASD_OK, BASD_ERR_SHAPE = 0, 1
ENTRIES = ("plain", "ws")                  # basd_wgrad_bf16, basd_wgrad_bf16_ws
PAD = 256                                  # sentinel floats before and after dw and db
SENTINEL = 0x7FC1A5A5                      # a quiet-NaN fp32 payload no kernel produces
WS_PAD, WS_BYTE = 1024, 0xA5               # sentinel bytes around the workspace
ROW_PAD = 64                               # NaN rows before and after dy and x: a row read outside [0, M) poisons dw


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    _CACHE.clear()


# one entry per kind: the inputs and references of the case under test; the previous case's are freed
_CACHE = {}


def _cached(kind, key, make):
    hit = _CACHE.get(kind)
    if hit is None or hit[0] != key:
        _CACHE.pop(kind, None)
        hit = _CACHE[kind] = (key, make())
    return hit[1]


def _rows_in_nan(t):
    """t [M, C] bf16 (CPU) -> the same rows on the GPU as a view into a buffer with 64 NaN rows before and behind"""
    buf = torch.full((t.shape[0] + 2 * ROW_PAD, t.shape[1]), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[ROW_PAD:ROW_PAD + t.shape[0]] = t.cuda()
    return buf[ROW_PAD:ROW_PAD + t.shape[0]]


def _integer_case(case):
    """dy, x (GPU, inside NaN rows), dw0, db0 (GPU) and the exact results with and without the initial values, as fp32
    (tests/test_wgrad_cases_cpu.py: they are integers below 2^24).  The reference is fp64 on the CPU."""
    def make():
        dy, x, dw0, db0 = C.integer_inputs(*case)
        raw_w, raw_b = C.reference(dy, x)
        ref_w, ref_b = raw_w + dw0.double(), raw_b + db0.double()
        for r in (ref_w, ref_b, raw_w, raw_b):
            assert torch.equal(r.float().double(), r)
        return dict(dy=_rows_in_nan(dy), x=_rows_in_nan(x), dw0=dw0.cuda(), db0=db0.cuda(), ref_w=ref_w.float().cuda(),
                    ref_b=ref_b.float().cuda(), raw_w=raw_w.float().cuda(), raw_b=raw_b.float().cuda())
    return _cached("integer", case, make)


class Flat:
    """dw [N, K] and db [N] as views into the middle of ONE fp32 buffer, as the flat gradient buffer hands them out,
    with 256 sentinel floats before, between and behind"""

    def __init__(self, N, K, dw0=None, db0=None):
        self.buf = torch.full((3 * PAD + N * K + N,), SENTINEL, dtype=torch.int32, device="cuda")
        f = self.buf.view(torch.float32)
        self.dw = f[PAD:PAD + N * K].view(N, K)
        self.db = f[2 * PAD + N * K:2 * PAD + N * K + N]
        self.guard = torch.ones_like(self.buf, dtype=torch.bool)
        if dw0 is not None:
            self.dw.copy_(dw0)
            self.guard[PAD:PAD + N * K] = False
        if db0 is not None:
            self.db.copy_(db0)
            self.guard[2 * PAD + N * K:2 * PAD + N * K + N] = False

    def assert_sentinels_untouched(self, what):
        bad = ((self.buf != SENTINEL) & self.guard).nonzero().flatten()
        assert len(bad) == 0, f"{what}: {len(bad)} sentinel floats around dw / db were written, the first at float " \
                              f"{int(bad[0])} of the flat buffer (dw starts at {PAD}, db at {2 * PAD + self.dw.numel()})"


class Workspace:
    """``nbytes`` of workspace, 16-byte aligned, NaN-filled, with sentinel bytes before and behind"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((2 * WS_PAD + nbytes,), WS_BYTE, dtype=torch.uint8, device="cuda")
        self.ws = self.buf[WS_PAD:WS_PAD + nbytes]
        assert self.ws.data_ptr() % 16 == 0
        self.fill_nan()

    def fill_nan(self):
        self.ws.view(torch.float32).fill_(float("nan"))

    def assert_sentinels_untouched(self, what):
        ok = bool((self.buf[:WS_PAD] == WS_BYTE).all()) and bool((self.buf[WS_PAD + self.nbytes:] == WS_BYTE).all())
        assert ok, f"{what}: bytes outside the {self.nbytes}-byte workspace were written"


def _call(nat, entry, dy, x, case, dw, db, ws=None, ws_ptr=None, ws_bytes=None):
    """one C call; ``ws``: a Workspace (ws entry only), or an explicit pointer / length"""
    M, N, K = case
    L, P = nat.lib(), nat._ptr
    if entry == "plain":
        return L.basd_wgrad_bf16(P(dy), P(x), ctypes.c_int64(M), N, K, P(dw), P(db), nat._stream())
    if ws_ptr is None:
        ws_ptr = ctypes.c_void_p(ws.ws.data_ptr() if ws is not None and ws.nbytes else 0)
    if ws_bytes is None:
        ws_bytes = ws.nbytes if ws is not None else 0
    return L.basd_wgrad_bf16_ws(P(dy), P(x), ctypes.c_int64(M), N, K, P(dw), P(db), ws_ptr, ctypes.c_int64(ws_bytes),
                                nat._stream())


def _need(nat, case):
    need = int(nat.lib().basd_wgrad_workspace_bytes(ctypes.c_int64(case[0]), case[1], case[2]))
    assert need == C.plan(*case).workspace_bytes and need % 16 == 0
    return need


def _assert_exact(case, what, got_w, ref_w, got_b=None, ref_b=None):
    """torch.equal, and on a mismatch the first differing (n, k), the tile and the wave it belongs to, the difference"""
    p = C.plan(*case)
    if not torch.equal(got_w, ref_w):
        bad = (got_w != ref_w).nonzero()                    # a NaN differs from everything
        n, k = (int(v) for v in bad[0])
        rows, cols = bad[:, 0], bad[:, 1]
        raise AssertionError(
            f"{what} {C.case_id(case)}: {len(bad)} of {got_w.numel()} elements of dw differ (n {int(rows.min())} .. "
            f"{int(rows.max())}, k {int(cols.min())} .. {int(cols.max())}); the first at (n {n}, k {k}): got "
            f"{float(got_w[n, k])}, exact {float(ref_w[n, k])}, difference {float(got_w[n, k]) - float(ref_w[n, k])}; "
            f"{C.locate(p, n, k)}")
    if ref_b is not None and not torch.equal(got_b, ref_b):
        bad = (got_b != ref_b).nonzero().flatten()
        n = int(bad[0])
        raise AssertionError(
            f"{what} {C.case_id(case)}: {len(bad)} of {got_b.numel()} elements of db differ; the first at n {n}: got "
            f"{float(got_b[n])}, exact {float(ref_b[n])}, difference {float(got_b[n]) - float(ref_b[n])}; "
            f"{C.locate(p, n, 0)}")


def _exact_run(nat, case, entry, bias=True, ws=None):
    """Integer regime into views of a flat buffer that already holds dw0 / db0; with ``bias=False`` db is a null
    pointer and the flat buffer's db stays sentinel-filled.  The ws entry gets a NaN-filled workspace of exactly
    ``basd_wgrad_workspace_bytes``."""
    M, N, K = case
    d = _integer_case(case)
    flat = Flat(N, K, d["dw0"], d["db0"] if bias else None)
    if entry == "ws" and ws is None:
        ws = Workspace(_need(nat, case))
    rc = _call(nat, entry, d["dy"], d["x"], case, flat.dw, flat.db if bias else None, ws)
    assert rc == BASD_OK, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    what = f"{entry} entry" + ("" if bias else ", db == nullptr")
    if bias:
        _assert_exact(case, what, flat.dw, d["ref_w"], flat.db, d["ref_b"])
    else:
        _assert_exact(case, what, flat.dw, d["ref_w"])
    flat.assert_sentinels_untouched(what)
    if entry == "ws":
        ws.assert_sentinels_untouched(what)
    return ws


# ------------------------------------------------------------------------------------------------------------------
# 1. exact accumulation, workspace discipline
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_integer_accumulation_is_exact(nat, case, entry):
    """dy integers in [-2, 2], x in [-4, 4], dw / db start from integers in [-1024, 1024]: every partial sum in any
    order is an integer below 2^24, so fp32 accumulation, the MFMA, the atomics and the reduce are exact and the result
    EQUALS dw0 + dy^T x, db0 + colsum(dy) (fp64 on the CPU), bit for bit.  A dropped or doubled row, a partial tile
    added twice or not at all, a bias added by a second k tile, an element stored to the wrong (n, k): each changes an
    integer.  dw and db are views into one larger buffer (the flat gradient buffer), the sentinels around them must
    survive; dy and x lie between NaN rows, so a row read outside [0, M) shows too.  On the workspace entry the
    workspace is exactly as long as asked for and NaN-filled: a partial tile that is read without having been written
    poisons dw, a write past its end hits the sentinels."""
    _exact_run(nat, case, entry)


# ------------------------------------------------------------------------------------------------------------------
# 2. one workspace, two shapes
# ------------------------------------------------------------------------------------------------------------------
def test_two_ring_shapes_back_to_back_on_one_workspace(nat):
    """(8192, 192, 384) with 128 slices, then (4096, 1152, 1152) with 7 on the SAME buffer, not refilled: the second
    reduce finds the first launch's partial tiles wherever it reads something its own launch did not write"""
    first, second = C.BACK_TO_BACK
    ws = Workspace(max(_need(nat, first), _need(nat, second)))
    _exact_run(nat, first, "ws", ws=ws)
    assert bool(torch.isfinite(ws.ws.view(torch.float32)[:_need(nat, first) // 4]).all())      # all of it was written
    _exact_run(nat, second, "ws", ws=ws)


# ------------------------------------------------------------------------------------------------------------------
# 3. db == nullptr
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", C.NO_BIAS_REGISTER_CASES + C.NO_BIAS_RING_CASES, ids=C.case_id)
def test_null_db_leaves_the_bias_alone(nat, case, entry):
    """db == nullptr (a Linear without bias): dw exact, and the place db has in the flat buffer keeps its sentinels"""
    _exact_run(nat, case, entry, bias=False)


def test_python_entry_without_bias(nat):
    case = C.NO_BIAS_RING_CASES[1]
    d = _integer_case(case)
    dw, db = nat.wgrad_bf16(d["dy"], d["x"], need_bias=False)
    torch.cuda.synchronize()
    assert db is None
    _assert_exact(case, "_native.wgrad_bf16(need_bias=False)", dw, d["raw_w"])


# ------------------------------------------------------------------------------------------------------------------
# 4. the Python entry
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.PYTHON_ENTRY_CASES, ids=C.case_id)
def test_python_entry_with_and_without_outputs(nat, case):
    """_native.wgrad_bf16: fresh zero-initialised outputs, and accumulation into out_w / out_b (views of a flat
    buffer), exact in the integer regime"""
    M, N, K = case
    d = _integer_case(case)
    dw, db = nat.wgrad_bf16(d["dy"], d["x"])
    torch.cuda.synchronize()
    assert dw.shape == (N, K) and db.shape == (N,) and dw.dtype == db.dtype == torch.float32
    _assert_exact(case, "_native.wgrad_bf16", dw, d["raw_w"], db, d["raw_b"])
    flat = Flat(N, K, d["dw0"], d["db0"])
    out_w, out_b = nat.wgrad_bf16(d["dy"], d["x"], out_w=flat.dw, out_b=flat.db)
    torch.cuda.synchronize()
    assert out_w is flat.dw and out_b is flat.db
    _assert_exact(case, "_native.wgrad_bf16(out_w, out_b)", flat.dw, d["ref_w"], flat.db, d["ref_b"])
    flat.assert_sentinels_untouched("_native.wgrad_bf16(out_w, out_b)")


# ------------------------------------------------------------------------------------------------------------------
# 5. real regime, per element
# ------------------------------------------------------------------------------------------------------------------
def _real_case(case):
    def make():
        dy, x = C.real_inputs(*case)
        return dict(dy=_rows_in_nan(dy), x=_rows_in_nan(x), ref=C.reference(dy, x), mag=C.magnitude(dy, x))
    return _cached("real", case, make)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_real_regime_against_fp64_elementwise(nat, case, entry):
    """x ~ N(0, 1), dy ~ N(0, 1) 10^u with u uniform in [-6, -2] per row, rounded to bf16; the reference is the fp64
    product of the rounded values (CPU).  For EVERY element

        |dw - ref| <= tol (|dy|^T |x|)[n, k]        |db - ref| <= tol (sum_m |dy|)[n]

    with tol = min(4 x 2.66e-7, M 2^-23): four times the worst ratio of the CPU emulation of the same chunk and slice
    sums over all cases (tests/_wgrad_cases.py, profiles/wgrad_margins.txt), never above the first-order bound.
    Nothing is relative to the largest output: an error confined to small elements fails.  Measured on an MI355X: the
    kernels' worst ratio over all cases and both entries is 2.7e-7 for dw and 6.0e-8 for db, 0.25 of the tolerance
    (profiles/wgrad_margins.txt has them per case)."""
    M, N, K = case
    d = _real_case(case)
    flat = Flat(N, K)
    flat.dw.zero_()
    flat.db.zero_()
    ws = Workspace(_need(nat, case)) if entry == "ws" else None
    rc = _call(nat, entry, d["dy"], d["x"], case, flat.dw, flat.db, ws)
    assert rc == BASD_OK, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    rw, rb = C.worst_ratio(flat.dw.cpu(), flat.db.cpu(), *d["ref"], *d["mag"])
    tol = C.tolerance(M)
    print(f"wgrad-margin {C.case_id(case)} {C.plan(*case).kernel} {entry} dw {rw:.3e} db {rb:.3e} tol {tol:.3e}")
    assert rw <= tol and rb <= tol, (rw, rb, tol)          # a NaN ratio fails both


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(nat):
    """BASD_ERR_SHAPE for N = 96, K = 96, N = 32 on both entries, and on the workspace entry for a ring shape with a
    null workspace, one a byte short, one misaligned by 8 bytes; BASD_OK for M = 0.  dw and db keep their sentinels."""
    L = nat.lib()
    ring = C.RING_CASES[0]
    M, N, K = ring
    d = _integer_case(ring)
    flat = Flat(1152, 1152)                                 # sentinel-filled throughout; large enough for every call
    flat.guard[:] = True
    need = _need(nat, ring)
    ws = Workspace(need + 16)

    def refused(rc, what):
        assert rc == BASD_ERR_SHAPE, (what, rc, L.basd_last_error())
        assert b"wgrad" in L.basd_last_error(), what

    for entry in ENTRIES:
        for shape in ((M, 96, K), (M, N, 96), (M, 32, K), (130, 96, 64), (130, 64, 96), (130, 32, 64)):
            refused(_call(nat, entry, d["dy"], d["x"], shape, flat.dw, flat.db, ws), (entry, shape))
        assert _call(nat, entry, d["dy"], d["x"], (0, N, K), flat.dw, flat.db, ws) == BASD_OK, entry
    base = ws.ws.data_ptr()
    refused(_call(nat, "ws", d["dy"], d["x"], ring, flat.dw, flat.db, ws_ptr=ctypes.c_void_p(0), ws_bytes=need), "null")
    refused(_call(nat, "ws", d["dy"], d["x"], ring, flat.dw, flat.db, ws_ptr=ctypes.c_void_p(base), ws_bytes=need - 1),
            "one byte short")
    refused(_call(nat, "ws", d["dy"], d["x"], ring, flat.dw, flat.db, ws_ptr=ctypes.c_void_p(base + 8), ws_bytes=need),
            "misaligned by 8 bytes")
    torch.cuda.synchronize()
    flat.assert_sentinels_untouched("refused calls")
    ws.assert_sentinels_untouched("refused calls")
    assert bool(torch.isnan(ws.ws.view(torch.float32)).all()), "a refused call wrote to the workspace"
    # the same buffers are fine with legal arguments
    assert _call(nat, "ws", d["dy"], d["x"], ring, flat.dw, flat.db, ws_ptr=ctypes.c_void_p(base), ws_bytes=need) == BASD_OK
    torch.cuda.synchronize()

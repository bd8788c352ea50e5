"""The bf16 GEMM kernels of csrc/gemm_bf16.hip (persistent ring, ring, two-stage 192 / 128 wide) at the shapes where
their schedules, K tails and ragged rows take different paths (GPU box only).  tests/_gemm_cases.py holds the case list
and says which path each case reaches (pinned by tests/test_gemm_cases_cpu.py).

  1. ``tile_run`` invariance of the persistent kernel, bitwise;
  2. every kernel against an fp64 reference, elementwise, with a derived bound;
  3. exact integer products: no tolerance at all;
  4. ragged rows: nothing written behind row M of an output, nothing read behind row M of the activations.
"""
import pytest
import torch

from tests import _gemm_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    _CACHE.clear()


# one entry per kind: the inputs (and the tile_run = 0 results) of the shape under test; the previous shape's are freed
_CACHE = {}


def _cached(kind, key, make):
    hit = _CACHE.get(kind)
    if hit is None or hit[0] != key:
        _CACHE.pop(kind, None)
        hit = _CACHE[kind] = (key, make())
    return hit[1]


def _random_inputs(shape):
    return _cached("random", shape, lambda: tuple(t.cuda() for t in C.random_inputs(*shape)))


def _sentinel(M, N):
    return torch.full((M + C.PAD, N), C.SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _gemm(nat, x, w, b, M, epilogue, tile_run):
    """basd_gemm_bf16 on the first M rows of x into a caller-owned buffer of M + 256 rows.  Every output of these tests
    is pre-filled with a NaN bit pattern the kernels never produce (torch.empty may hand back the block that held the
    previous launch's correct result, and a tile nobody multiplied would go unnoticed)."""
    N, K = w.shape
    y = _sentinel(M, N)
    rc = nat.lib().basd_gemm_bf16(nat._ptr(x), nat._ptr(w), nat._ptr(b), nat._ptr(y), M, N, K, epilogue, tile_run,
                                  nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    return y


def _run_entries(nat, inputs, M, tile_run, pre=None):
    """every entry of the GEMM on the first M rows of the inputs: basd_gemm_bf16 with epilogue 0 / 1 / 2,
    basd_gemm_bf16_gelu_fwd (both outputs) and basd_gemm_bf16_gelu_bwd (on ``pre``, default: this run's own; ``w`` is
    also its transposed fc2 weight).  Buffers of M + 256 rows."""
    x, w, b, dy = inputs
    N, K = w.shape
    L, ptr, st = nat.lib(), nat._ptr, nat._stream()
    out = {"epi0": _gemm(nat, x, w, None, M, 0, tile_run), "epi1": _gemm(nat, x, w, b, M, 1, tile_run),
           "epi2": _gemm(nat, x, w, b, M, 2, tile_run), "pre": _sentinel(M, N), "act": _sentinel(M, N),
           "dpre": _sentinel(M, N)}
    rc = L.basd_gemm_bf16_gelu_fwd(ptr(x), ptr(w), ptr(b), ptr(out["pre"]), ptr(out["act"]), M, N, K, tile_run, st)
    assert rc == 0, L.basd_last_error()
    rc = L.basd_gemm_bf16_gelu_bwd(ptr(dy), ptr(w), ptr(out["pre"] if pre is None else pre), ptr(out["dpre"]), M, N, K,
                                   tile_run, st)
    assert rc == 0, L.basd_last_error()
    torch.cuda.synchronize()
    return out


def _tail_untouched(buf, M):
    return bool((buf[M:].view(torch.int16) == C.SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------------------------
_CHUNK = 1 << 23          # elements of an fp64 reference piece: 64 MB


def _bound_ratio(y, x, w, b):
    """max over the elements of |y - ref| / (2^-8 |ref| + (K + 2) 2^-24 S) with ref = x w^T + b in fp64 from the same
    bf16 inputs and S = |x| |w|^T + |b|, in row chunks"""
    M, N = y.shape
    K = x.shape[1]
    wt = w.double().t().contiguous()
    wt_abs = wt.abs()
    bd = None if b is None else b.double()
    rows = max(1, _CHUNK // N)
    worst = 0.0
    for r0 in range(0, M, rows):
        xd = x[r0:r0 + rows].double()
        ref, S = xd @ wt, xd.abs() @ wt_abs
        if bd is not None:
            ref, S = ref + bd, S + bd.abs()
        err = (y[r0:r0 + rows].double() - ref).abs_()
        bound = ref.abs_().mul_(2.0 ** -8).add_(S, alpha=(K + 2) * 2.0 ** -24)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)     # an exact element passes a zero bound
        assert not bool(torch.isnan(ratio).any()), "NaN in the output (or read from behind row M)"
        worst = max(worst, float(ratio.max()))
    return worst


def _check_gelu_output(y, x, w, b):
    """epilogue 2 as tests/test_kernels_gpu.py::test_gemm_bf16_with_fused_epilogue checks it"""
    ref = torch.nn.functional.gelu(x.float() @ w.float().t() + b.float())
    err = (y.float() - ref).abs()
    top = float(ref.abs().max())
    assert float((err / (ref.abs() + 1e-2 * top)).max()) < 1.2e-2
    assert float(err.max()) <= 6e-3 * top


def _check_gelu_pair(pre, act, dpre, epi1, x, w, b, dy):
    """the GELU pair as tests/test_kernels_gpu.py::test_gemm_bf16_gelu_training_pair checks it; ``w`` is also the
    transposed fc2 weight of the backward"""
    ref_pre = x.float() @ w.float().t() + b.float()
    assert pre.shape == act.shape == ref_pre.shape and pre.dtype == act.dtype == torch.bfloat16
    assert float((pre.float() - ref_pre).abs().max()) <= 6e-3 * float(ref_pre.abs().max())
    del ref_pre
    ref_act = torch.nn.functional.gelu(pre.float())
    assert float((act.float() - ref_act).abs().max()) <= 4.1e-3 * float(ref_act.abs().max())
    del ref_act
    assert torch.equal(pre, epi1)                                    # same accumulation, same rounding
    p = pre.float().requires_grad_(True)
    torch.nn.functional.gelu(p).backward(dy.float() @ w.float().t())
    ref = p.grad
    err = (dpre.float() - ref).abs()
    assert dpre.shape == pre.shape
    top = float(ref.abs().max())
    assert float(err.max()) <= 6e-3 * top
    assert float((err / (ref.abs() + 1e-2 * top)).max()) < 1.2e-2


# ------------------------------------------------------------------------------------------------------------------
# 1. tile_run invariance
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.INVARIANCE_CASES, ids=C.case_id)
def test_persistent_kernel_results_do_not_depend_on_tile_run(nat, case):
    """include/basd_hip.h: "The results do not depend on it".  Which workgroup multiplies a tile, after which other
    tile, on how many workgroups per XCD and in how many chunks changes nothing in a tile's arithmetic, so every entry
    must give bitwise the tile_run = 0 result (tile_run = 0 itself: a second run of the same launch)."""
    shape, tile_run = case[:3], case[3]
    inputs = _random_inputs(shape)
    base = _cached("base", shape, lambda: _run_entries(nat, inputs, shape[0], 0))
    got = _run_entries(nat, inputs, shape[0], tile_run, pre=base["pre"])
    for name, want in base.items():
        if not torch.equal(got[name].view(torch.int16), want.view(torch.int16)):      # the rows behind M included
            bad = (got[name].view(torch.int16) != want.view(torch.int16)).nonzero()
            raise AssertionError(f"{name}: {len(bad)} elements differ from tile_run = 0, rows {int(bad[:, 0].min())} .. "
                                 f"{int(bad[:, 0].max())}, columns {int(bad[:, 1].min())} .. {int(bad[:, 1].max())}")


# ------------------------------------------------------------------------------------------------------------------
# 2. fp64 reference, elementwise
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REFERENCE_CASES, ids=C.case_id)
def test_every_kernel_against_fp64_elementwise(nat, case):
    """Epilogues 0 and 1 against ref = x w^T (+ bias) in fp64 from the same bf16 inputs, for EVERY element:

        |y - ref| <= 2^-8 |ref| + (K + 2) 2^-24 S,      S = |x| |w|^T + |bias|

    Second term: the fp32 accumulation of K exact products (a bf16 product has 16 significant bits) and the bias, in
    any order: at most K rounding errors of relative size 2^-24 on partial sums bounded by S, two more for slack on the
    second-order terms.  First term: the one rounding to bf16 -- 8 significant bits, so at most 2^-8 of the rounded
    value, which is within the second term of ref.  Nothing is relative to the largest output, so an error confined to
    small outputs or two swapped rows of equal scale fail.  Measured on an MI355X: the largest ratio of error to bound
    over all cases is 0.994 (0.89 .. 0.99 per case: the bf16 rounding of a value just above a power of two, where half
    an ulp is almost 2^-8 of the value; the accumulation term never decides).

    The GELU epilogues (2, gelu_fwd, gelu_bwd) keep the checks of tests/test_kernels_gpu.py; the saved pre-activation
    of gelu_fwd is bitwise the epilogue-1 output."""
    shape, tile_run = case[:3], case[3]
    x, w, b, dy = inputs = _random_inputs(shape)
    M = shape[0]
    out = {name: buf[:M] for name, buf in _run_entries(nat, inputs, M, tile_run).items()}
    for name, bias in (("epi0", None), ("epi1", b)):
        assert out[name].shape == (shape[0], shape[1]) and out[name].dtype == torch.bfloat16
        ratio = _bound_ratio(out[name], x, w, bias)
        print(f"gemm-bound {C.case_id(case)} {C.dispatch(*shape)} {name} ratio {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)
    _check_gelu_output(out["epi2"], x, w, b)
    _check_gelu_pair(out["pre"], out["act"], out["dpre"], out["epi1"], x, w, b, dy)


# ------------------------------------------------------------------------------------------------------------------
# 3. exact integer products
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REFERENCE_CASES, ids=C.case_id)
def test_integer_products_are_exact(nat, case):
    """x, w from {-1, 0, 1}, integer bias in [-8, 8], at most 240 non-zeros per row of w: every partial sum is an
    integer of magnitude <= 248 -- exact in fp32 in any order, and a bf16 number -- so the output EQUALS the integer
    product.  A dropped or doubled K step, a fragment from the wrong ring slot, a swapped row: each changes an integer.
    The inputs depend on the position (seeded per case, x[m, m % K] = w[n, n % K] = 1 before thinning)."""
    shape, tile_run = case[:3], case[3]
    M, N, K = shape
    x, w, b = _cached("integer", shape, lambda: tuple(t.cuda() for t in C.integer_inputs(*shape)))
    got = {"epi0": _gemm(nat, x, w, None, M, 0, tile_run), "epi1": _gemm(nat, x, w, b, M, 1, tile_run)}
    torch.cuda.synchronize()
    assert _tail_untouched(got["epi0"], M) and _tail_untouched(got["epi1"], M)
    wt = w.double().t().contiguous()
    rows = max(1, _CHUNK // N)
    for r0 in range(0, M, rows):
        xd = x[r0:r0 + rows].double()
        ref0 = xd @ wt
        assert float((xd.abs() @ wt.abs() + b.double().abs()).max()) <= 256          # the condition of exactness
        for name, ref in (("epi0", ref0), ("epi1", ref0 + b.double())):
            y = got[name][r0:min(r0 + rows, M)].double()
            if not torch.equal(y, ref):
                bad = (y != ref).nonzero()
                m, n = (int(v) for v in bad[0])
                raise AssertionError(f"{name}: {len(bad)} wrong integers in rows {r0} .. {r0 + len(y) - 1}, the first at "
                                     f"[{r0 + m}, {n}]: {float(y[m, n])} for {float(ref[m, n])}")


# ------------------------------------------------------------------------------------------------------------------
# 4. ragged rows
# ------------------------------------------------------------------------------------------------------------------
def _nan_tail(t):
    return torch.cat([t, torch.full((C.PAD, t.shape[1]), float("nan"), dtype=t.dtype, device=t.device)])


@pytest.mark.parametrize("case", C.RAGGED_CASES, ids=C.case_id)
def test_nothing_written_or_read_behind_row_M(nat, case):
    """Direct C calls on caller-owned buffers of M + 256 rows.  The outputs are pre-filled with a NaN bit pattern the
    kernels never produce: the 256 rows behind M must keep it, bit for bit.  The activation rows behind M are NaN: the
    kernels promise to re-read row M - 1 for them, so the first M rows of every output still satisfy the checks of
    part 2 (a NaN fails each of them)."""
    shape, tile_run = case[:3], case[3]
    M, N, K = shape
    x, w, b, dy = _random_inputs(shape)
    out = _run_entries(nat, (_nan_tail(x), w, b, _nan_tail(dy)), M, tile_run)
    for name, buf in out.items():
        assert buf.shape == (M + C.PAD, N) and _tail_untouched(buf, M), f"{name}: rows behind M were written"
    out = {name: buf[:M] for name, buf in out.items()}
    assert _bound_ratio(out["epi0"], x, w, None) <= 1.0
    assert _bound_ratio(out["epi1"], x, w, b) <= 1.0
    assert _bound_ratio(out["pre"], x, w, b) <= 1.0
    _check_gelu_output(out["epi2"], x, w, b)
    _check_gelu_pair(out["pre"], out["act"], out["dpre"], out["epi1"], x, w, b, dy)

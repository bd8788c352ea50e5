"""The widened Procrustes backward (row-tiled residual product, 257 <= n <= 1024 and n % 4 != 0) on a CPU-only machine:
the predicate of the binding, the argument checks of the C entries (they return before anything touches a device) and
the CPU restatement of the contract (tests/_pbwd_emul.py) against fp64, so the yardstick of the GPU tests is itself
pinned."""
import ctypes
import os

import pytest
import torch

from tests import _pbwd_emul

BASD_ERR_SHAPE = 1


@pytest.fixture(scope="module")
def lib():
    import basd_amd._native as native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


@pytest.mark.parametrize("n,d_s,d_t,want", [
    (576, 192, 768, True), (729, 192, 768, True), (1024, 192, 1024, True), (54, 48, 80, True), (257, 192, 384, True),
    (260, 64, 80, True), (320, 384, 384, True), (196, 192, 768, True), (16, 32, 64, True), (4, 16, 16, True),
    (1028, 192, 768, False), (1025, 192, 768, False), (3, 16, 16, False), (576, 192, 760, False), (576, 192, 8, False),
    (320, 380, 384, False),      # token side: the student product needs d_s % 16 == 0 as well
    (576, 190, 768, False)])     # feature side: the row kernel needs d_s % 4 == 0
def test_procrustes_bwd_supported(n, d_s, d_t, want):
    import basd_amd._native as native
    assert native.procrustes_bwd_supported(n, d_s, d_t) is want


def _side(lib, n, d, batch=2, fac=4096, w=4096, out=4096):
    p = ctypes.c_void_p
    return lib.basd_procrustes_bwd_side(p(fac), p(w), p(4096), p(4096), batch, n, d, p(out), 0, p(4096), p(0))


def test_side_entry_refuses_bad_shapes_and_names_the_limit(lib):
    for n, d in [(1028, 768), (1025, 768), (3, 768), (576, 760), (576, 8), (729, 0)]:
        assert _side(lib, n, d) == BASD_ERR_SHAPE, (n, d)
        msg = lib.basd_last_error()
        assert b"procrustes_bwd_side" in msg and b"1024" in msg, msg
    # whole-matrix kernels (n <= 256, n % 4 == 0) load the factor 16 bytes wide; the row-tiled form needs 4-byte alignment
    assert _side(lib, 196, 768, fac=4100) == BASD_ERR_SHAPE
    assert _side(lib, 576, 768, fac=4098) == BASD_ERR_SHAPE
    assert _side(lib, 576, 768, w=4100) == BASD_ERR_SHAPE and _side(lib, 576, 768, out=4104) == BASD_ERR_SHAPE


def test_whole_entry_refuses_1028_rows(lib):
    p = ctypes.c_void_p(4096)
    need = lib.basd_procrustes_bwd_workspace_bytes(2, 1028)
    assert need == 2 * 2 * 1028 * 4
    rc = lib.basd_procrustes_bwd(p, p, p, p, p, p, 2, 1028, 192, 768, p, 0, p, p, p, ctypes.c_int64(need), ctypes.c_void_p(0))
    assert rc == BASD_ERR_SHAPE and b"1024" in lib.basd_last_error()


def test_empty_batch_is_a_no_op(lib):
    assert _side(lib, 576, 768, batch=0) == 0
    assert lib.basd_procrustes_bwd_workspace_bytes(3, 729) == 2 * 3 * 729 * 4


def _inputs(batch, n, d_s, d_t, seed):
    g = torch.Generator().manual_seed(seed)
    s_w = torch.randn(batch, n, d_s, generator=g)
    t_w = torch.randn(batch, n, d_t, generator=g)
    a = torch.rand(batch, n, generator=g) + 0.1
    a = a / a.sum(-1, keepdim=True)
    gl = torch.randn(batch, generator=g)
    a_t = torch.randn(batch, n, n, generator=g) / n ** 0.5
    fac_s = torch.randn(batch, n, n, generator=g) / n ** 0.5 if n <= d_s else torch.randn(batch, n, d_s, generator=g)
    return s_w, t_w, a, gl, fac_s, a_t


def test_emulation_against_fp64_at_576_rows():
    """The split product's error is bounded from the number formats: hi keeps 8 significant bits, mid the next 8, so
    |x - hi - mid| <= 2^-18 |x|; the three kept products therefore miss a term of fac W by at most
    (2^-18 + 2^-18 + 2^-18 [the dropped mid x mid]) |fac| |W| = 3 x 2^-18 |fac| |W|, and K = n fp32 additions add a
    rounding error that grows like sqrt(K) 2^-24 |fac| |W| (2^-23 allowed here).  The bound is applied per row in the
    Frobenius norm, scaled like the output; the element-wise fp32 epilogue adds 4 ulp of the result."""
    n, d_t = 576, 768
    s_w, t_w, a, gl, fac_s, a_t = _inputs(2, n, 192, d_t, seed=576)
    g_s, g_t, g_a = _pbwd_emul.procrustes_bwd(s_w, t_w, a, gl, fac_s, a_t, torch.float32)
    want_s, want_t, want_a = _pbwd_emul.reference_f64(s_w, t_w, a, gl, fac_s, a_t)
    unit = 3 * 2.0 ** -18 + n ** 0.5 * 2.0 ** -23
    row_bound = unit * (a_t.double().abs() @ t_w.double().abs()).norm(dim=-1)            # [batch, n]
    c = (2.0 * gl.double()).abs().view(-1, 1) * a.double().sqrt()
    bound = float((c * row_bound).norm()) + 4 * 2.0 ** -24 * float(want_t.norm())
    err = float((g_t.double() - want_t).norm())
    rel_t = err / float(want_t.norm())
    rel_s = float((g_s.double() - want_s).norm() / want_s.norm())
    rel_a = float((g_a.double() - want_a).norm() / want_a.norm())
    print(f"emulation vs fp64 at n = 576: g_t {rel_t:.3e} (bound {bound / float(want_t.norm()):.3e}), g_s {rel_s:.3e}, "
          f"g_a {rel_a:.3e}")
    assert 0.0 < err <= bound, (err, bound)
    # feature side: the student residual is element-wise fp32 (a subtraction and a product: 2 ulp at most)
    assert rel_s <= 2 * 2.0 ** -24, rel_s
    # the row dots sum d_s + d_t products of the residual in fp32 on top of the product's error; <R, W> does not
    # cancel for these inputs (<W, W> dominates), so their relative error stays below the product bound's scale
    assert rel_a <= unit * float((a_t.double().abs() @ t_w.double().abs()).norm() / (t_w.double() - a_t.double() @ t_w.double()).norm()), rel_a
    # and the split matters: one bf16 product (hi x hi only) is two orders of magnitude worse
    hi_only = _pbwd_emul.split(a_t)[0] @ _pbwd_emul.split(t_w)[0]
    assert float((hi_only.double() - a_t.double() @ t_w.double()).norm()) > 50 * float(
        (_pbwd_emul.prod3(a_t, t_w).double() - a_t.double() @ t_w.double()).norm())


def test_emulation_token_side_and_bf16_output():
    s_w, t_w, a, gl, fac_s, a_t = _inputs(2, 48, 64, 80, seed=48)
    g_s, g_t, g_a = _pbwd_emul.procrustes_bwd(s_w, t_w, a, gl, fac_s, a_t, torch.bfloat16)
    want_s, want_t, want_a = _pbwd_emul.reference_f64(s_w, t_w, a, gl, fac_s, a_t)
    assert g_s.dtype == torch.bfloat16 and g_t.dtype == torch.float32 and g_a.shape == a.shape
    assert float((g_s.double() - want_s).norm() / want_s.norm()) < 2.0 ** -8          # one bf16 rounding per element
    assert float((g_t.double() - want_t).norm() / want_t.norm()) < 3e-5
    out, rowdot = _pbwd_emul.procrustes_bwd_side(fac_s, s_w, a, gl)
    assert torch.equal(out.to(torch.bfloat16), g_s)
    assert float((rowdot.double() - (2 * gl.double()).view(-1, 1) * ((s_w.double() - fac_s.double() @ s_w.double()) * s_w.double()).sum(-1)).abs().max()) < 1e-3


def test_nested_library_gemm_recorders_keep_their_own_sets():
    """a step recorded from outside runs the trainer's own recorder inside it: leaving the inner block (equal, empty
    set) must not take the outer recorder off the list"""
    from basd_amd.losses import _ops
    with _ops.record_library_gemms() as outer:
        with _ops.record_library_gemms() as inner:
            pass
        _ops.note_library_gemm("after the inner block")
    assert outer == {"after the inner block"} and inner == set()
    assert not _ops._GEMM_RECORDERS

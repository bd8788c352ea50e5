"""The Procrustes backward for 257 <= n <= 1024 student tokens (and n % 4 != 0) on the row-tiled residual-product kernel
(csrc/procrustes_bwd.hip, procrustes_bwd_side_tiled_kernel with row tiles): the C entries against fp64 with the CPU restatement of the
contract (tests/_pbwd_emul.py) as the yardstick, reproducibility, bounds, the autograd path and a 384 px training step.

Yardstick: the kernel and the restatement compute the same three bf16 products with fp32 accumulation and may differ in
the order of the fp32 additions only, so the kernel's error against fp64 has to stay within 2x the restatement's error
on the same tensors (rel-L2 of g_t, g_s, g_a; max-abs of g_t over max |want|).  Every test prints its figures before it
asserts; DESIGN.md section 5e holds the restatement's own errors against fp64 (CPU).  The kernel's figures have not been
recorded from an MI355X run yet."""
import ctypes
import os
import time

import pytest
import torch

from tests import _pbwd_emul

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
LIB_BMM = "Procrustes backward: fp32 bmm (A_t t_w)"


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


def _white_inputs(batch, n, d_s, d_t):
    """the construction of test_procrustes_bwd_entry_matches_the_unfused_chain (tests/test_kernels_gpu.py)"""
    g = torch.Generator().manual_seed(batch * 1000 + n)
    s_w = torch.randn(batch, n, d_s, generator=g)
    t_w = torch.randn(batch, n, d_t, generator=g)
    a = torch.rand(batch, n, generator=g) + 0.1
    a = (a / a.sum(-1, keepdim=True)).contiguous()
    gl = torch.randn(batch, generator=g)
    a_t = torch.randn(batch, n, n, generator=g) / n ** 0.5
    token_side = n <= d_s
    fac_s = (torch.randn(batch, n, n, generator=g) / n ** 0.5) if token_side else torch.randn(batch, n, d_s, generator=g)
    return s_w, t_w, a, gl, fac_s, a_t


def _errors(got, want):
    g_s, g_t, g_a = (x.detach().cpu().double() for x in got)
    want_s, want_t, want_a = want
    return {"g_t": float((g_t - want_t).norm() / want_t.norm()),
            "g_s": float((g_s - want_s).norm() / want_s.norm()),
            "g_a": float((g_a - want_a).norm() / want_a.norm()),
            "g_t max": float((g_t - want_t).abs().max() / want_t.abs().max())}


def _check_against_the_emulation(nat, label, cpu_inputs, s_dtype):
    dev_inputs = [x.cuda() for x in cpu_inputs]
    got = nat.procrustes_bwd(*dev_inputs, s_dtype)
    torch.cuda.synchronize()
    s_w, t_w = cpu_inputs[0], cpu_inputs[1]
    assert got[0].dtype == s_dtype and got[1].dtype == torch.float32
    assert got[0].shape == s_w.shape and got[1].shape == t_w.shape and got[2].shape == s_w.shape[:2]
    for x in got:
        assert bool(torch.isfinite(x.float()).all())
    want = _pbwd_emul.reference_f64(*cpu_inputs)
    kern = _errors(got, want)
    emul = _errors(_pbwd_emul.procrustes_bwd(*cpu_inputs, s_dtype), want)
    ratios = {k: kern[k] / emul[k] for k in kern}
    print(f"\n{label}: " + "; ".join(f"{k} kernel {kern[k]:.3e} emulation {emul[k]:.3e} ratio {ratios[k]:.3f}" for k in kern))
    for k in kern:
        assert kern[k] <= 2.0 * emul[k], (label, k, kern[k], emul[k])
    return got


@pytest.mark.parametrize("batch,n,d_s,d_t,s_dtype", [
    (3, 576, 192, 768, torch.bfloat16), (2, 729, 192, 768, torch.float32), (2, 1024, 192, 1024, torch.bfloat16),
    (2, 260, 64, 80, torch.float32), (3, 257, 192, 384, torch.float32), (2, 54, 48, 80, torch.float32),
    (2, 320, 384, 384, torch.bfloat16),       # token side past 256 rows: both sides on the row-tiled kernel
    (2, 130, 144, 96, torch.float32)])        # token side, n % 4 != 0, two row tiles
def test_entry_against_fp64_within_twice_the_emulation(nat, batch, n, d_s, d_t, s_dtype):
    """basd_procrustes_bwd at shapes that used to return BASD_ERR_SHAPE (n > 256, n % 4 != 0), feature and token side"""
    _check_against_the_emulation(nat, f"n={n} d_s={d_s} d_t={d_t} {s_dtype}", _white_inputs(batch, n, d_s, d_t), s_dtype)


def _side(nat, fac, w, a, gl, out, rowdot, out_dtype):
    batch, n, d = w.shape
    code = nat.DTYPE_F32 if out_dtype == torch.float32 else nat.DTYPE_BF16
    p = ctypes.c_void_p
    rc = nat.lib().basd_procrustes_bwd_side(p(fac.data_ptr()), p(w.data_ptr()), p(a.data_ptr()), p(gl.data_ptr()), batch, n,
                                            d, p(out.data_ptr()), code, p(rowdot.data_ptr()), nat._stream())
    nat._check(rc, "basd_procrustes_bwd_side")


def test_side_entry_alone_on_the_token_side_form(nat):
    """basd_procrustes_bwd_side is generic: fac [n, n] at n = 320, d = 384 (the student side of a token-side step)"""
    batch, n, d = 2, 320, 384
    _, _, a, gl, _, _ = _white_inputs(batch, n, d, d)
    g = torch.Generator().manual_seed(320)
    w = torch.randn(batch, n, d, generator=g)
    fac = torch.randn(batch, n, n, generator=g) / n ** 0.5
    out = torch.empty(batch, n, d, device="cuda")
    rowdot = torch.empty(batch, n, device="cuda")
    _side(nat, fac.cuda(), w.cuda(), a.cuda(), gl.cuda(), out, rowdot, torch.float32)
    torch.cuda.synchronize()
    r = w.double() - fac.double() @ w.double()
    c2 = (2.0 * gl.double()).view(-1, 1)
    want_out, want_dot = (c2 * a.double().sqrt()).unsqueeze(-1) * r, c2 * (r * w.double()).sum(-1)
    e_out, e_dot = _pbwd_emul.procrustes_bwd_side(fac, w, a, gl)
    rel = lambda x, y: float((x.double().cpu() - y).norm() / y.norm())
    print(f"\nside n=320 d=384: out kernel {rel(out, want_out):.3e} emulation {rel(e_out, want_out):.3e}; "
          f"rowdot kernel {rel(rowdot, want_dot):.3e} emulation {rel(e_dot, want_dot):.3e}")
    assert rel(out, want_out) <= 2.0 * rel(e_out, want_out)
    assert rel(rowdot, want_dot) <= 2.0 * rel(e_dot, want_dot)


def _trained_inputs(batch=2, n=576, d_s=192, d_t=768, rank=192, exact_rows=64):
    """Inputs that look like a trained network's instead of white noise: 8 massive-activation channels of t_w (|mean|
    1e2 x their spread), an importance with 90 % of its mass on 5 % of the rows, and a_t = an orthogonal projector of
    rank 192 plus 1e-3 noise.  The projector is the identity on 64 (scattered) rows and a random rank-128 projector on
    the others, so P = a_t t_w cancels t_w on those 64 rows down to the noise: the residual there is 1e-3 of its
    operands, which is where a split product loses relative accuracy."""
    g = torch.Generator().manual_seed(384)
    s_w = torch.randn(batch, n, d_s, generator=g)
    t_w = torch.randn(batch, n, d_t, generator=g)
    ch = torch.randperm(d_t, generator=g)[:8]
    t_w[:, :, ch] += 100.0 * torch.where(torch.rand(8, generator=g) < 0.5, -1.0, 1.0)
    heavy = n // 20
    a = torch.empty(batch, n)
    for b in range(batch):
        perm = torch.randperm(n, generator=g)
        hi, lo = torch.rand(heavy, generator=g) + 0.5, torch.rand(n - heavy, generator=g) + 0.5
        a[b, perm[:heavy]] = 0.9 * hi / hi.sum()
        a[b, perm[heavy:]] = 0.1 * lo / lo.sum()
    gl = torch.randn(batch, generator=g)
    a_t = torch.zeros(batch, n, n)
    for b in range(batch):
        perm = torch.randperm(n, generator=g)
        q = torch.linalg.qr(torch.randn(n - exact_rows, rank - exact_rows, generator=g, dtype=torch.float64))[0]
        proj = torch.zeros(n, n, dtype=torch.float64)
        proj[:exact_rows, :exact_rows] = torch.eye(exact_rows, dtype=torch.float64)
        proj[exact_rows:, exact_rows:] = q @ q.t()
        a_t[b] = proj[perm][:, perm].float()
    a_t += 1e-3 * torch.randn(batch, n, n, generator=g)
    fac_s = torch.randn(batch, n, d_s, generator=g)
    return s_w, t_w, a.contiguous(), gl, fac_s, a_t.contiguous()


def test_trained_network_statistics_at_576_tokens(nat):
    inputs = _trained_inputs()
    s_w, t_w, a, gl, fac_s, a_t = inputs
    # the construction does what it says
    assert float(a.sort(dim=-1, descending=True).values[:, :576 // 20].sum(-1).min()) > 0.89
    r = t_w.double() - a_t.double() @ t_w.double()
    ratio = r.norm(dim=-1) / t_w.double().norm(dim=-1)
    assert int((ratio < 0.1).sum()) >= 2 * 64 and float(ratio.max()) > 0.5
    _check_against_the_emulation(nat, "trained statistics n=576", inputs, torch.float32)


def test_two_calls_are_bitwise_equal(nat):
    inputs = [x.cuda() for x in _white_inputs(3, 576, 192, 768)]
    first = nat.procrustes_bwd(*inputs, torch.bfloat16)
    second = nat.procrustes_bwd(*inputs, torch.bfloat16)
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    # and at n % 4 != 0 (4-byte factor loads)
    inputs = [x.cuda() for x in _white_inputs(2, 729, 192, 768)]
    first, second = nat.procrustes_bwd(*inputs, torch.float32), nat.procrustes_bwd(*inputs, torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])


def test_1028_rows_are_refused(nat):
    inputs = [x.cuda() for x in _white_inputs(1, 1028, 192, 32)]
    with pytest.raises(nat.BasdNativeError, match="1024"):
        nat.procrustes_bwd(*inputs, torch.float32)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_masked_last_tile_writes_nothing_past_row_n(nat, out_dtype):
    """n = 729: the sixth row tile holds 89 valid rows and the K tail 25 columns.  The outputs sit between guard bands of
    NaN in one allocation each; the bands stay NaN, every row below n is written."""
    batch, n, d, guard = 2, 729, 768, 160
    _, _, a, gl, _, _ = _white_inputs(batch, n, 192, d)
    g = torch.Generator().manual_seed(729)
    w = torch.randn(batch, n, d, generator=g)
    fac = torch.randn(batch, n, n, generator=g) / n ** 0.5
    out_all = torch.full((batch * n + 2 * guard, d), float("nan"), dtype=out_dtype, device="cuda")
    dot_all = torch.full((batch * n + 2 * guard,), float("nan"), device="cuda")
    out, rowdot = out_all[guard:guard + batch * n], dot_all[guard:guard + batch * n]
    _side(nat, fac.cuda(), w.cuda(), a.cuda(), gl.cuda(), out, rowdot, out_dtype)
    torch.cuda.synchronize()
    for band in (out_all[:guard], out_all[guard + batch * n:], dot_all[:guard], dot_all[guard + batch * n:]):
        assert bool(torch.isnan(band.float()).all())
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(rowdot).all())
    e_out, e_dot = _pbwd_emul.procrustes_bwd_side(fac, w, a, gl, out_dtype)
    assert torch.allclose(out.float().cpu().view(batch, n, d), e_out.float(), rtol=1e-2 if out_dtype == torch.bfloat16 else 1e-4,
                          atol=1e-5 * float(e_out.float().abs().max()))
    assert torch.allclose(rowdot.cpu().view(batch, n), e_dot, rtol=1e-4, atol=1e-5 * float(e_dot.abs().max()))


def test_autograd_at_576_tokens_against_the_library_path_and_fp64(nat):
    """functional.procrustes at B = 2, N = 576, D_s = 192, D_t = 768: gradients of the fused path against (a) the
    library path (PROCRUSTES_BWD_FUSED = False) and (b) fp64 autograd of oracle.basd_oracle.procrustes on the CPU.  The
    fused path's rel-L2 distance to (b) may be at most 1.5x the library path's, or within the 5e-4 the goldens allow."""
    import basd_amd.losses.functional as F
    from basd_amd.losses import _ops
    from oracle import basd_oracle as O
    _ops.set_ops(None)
    g = torch.Generator().manual_seed(576)
    s = torch.randn(2, 576, 192, generator=g)
    t = torch.randn(2, 576, 768, generator=g)
    imp = torch.rand(2, 576, generator=g) + 0.05
    seed = torch.tensor([0.7, -1.3])

    def grads(fn, dev, dtype):
        xs = [x.to(dev, dtype).requires_grad_(True) for x in (s, t, imp)]
        (fn(*xs) * seed.to(dev, dtype)).sum().backward()
        return [x.grad.detach().cpu().double() for x in xs]

    want = grads(O.procrustes, "cpu", torch.float64)
    assert F.PROCRUSTES_BWD_FUSED
    with _ops.record_library_gemms() as seen:
        fused = grads(F.procrustes, "cuda", torch.float32)
    assert LIB_BMM not in seen, seen
    F.PROCRUSTES_BWD_FUSED = False
    try:
        with _ops.record_library_gemms() as seen:
            library = grads(F.procrustes, "cuda", torch.float32)
    finally:
        F.PROCRUSTES_BWD_FUSED = True
    assert LIB_BMM in seen
    for name, f, l, w in zip(("s", "t", "imp"), fused, library, want):
        d_f, d_l = float((f - w).norm() / w.norm()), float((l - w).norm() / w.norm())
        print(f"\ngrad {name}: fused vs fp64 {d_f:.3e}, library vs fp64 {d_l:.3e}, fused vs library {float((f - l).norm() / l.norm()):.3e}")
        assert d_f <= max(1.5 * d_l, 5e-4), (name, d_f, d_l)


def _make_preset(student, teacher, batch, img, patch, extra=()):
    """the helper of tests/test_long_sequence_step_gpu.py"""
    from basd_amd.config import load_config
    from basd_amd.train import SyntheticLoader, build
    torch.manual_seed(0)
    cfg = load_config(CFG, None, [f"data.batch_size={batch}", "data.dataset=synthetic", f"model.student_preset={student}",
                                  f"basd.teacher_model_name={teacher}", f"model.vit.img_size={img}",
                                  f"model.vit.patch_size={patch}", "model.drop_path_rate=0.0"] + list(extra))
    trainer, _ = build(cfg, device="cuda")
    trainer.use_mixup = False
    trainer.optimizer.train()
    trainer.model.train()
    b = next(iter(SyntheticLoader(batch, img, cfg.model.num_classes, 1, "cuda", seed=5)))
    return trainer, b


def test_384px_step_keeps_the_procrustes_backward_off_the_library():
    """the img384-T577 preset (576 patch tokens), one strict-mode train_step: the loss backward's largest product no
    longer reports a library fp32 bmm"""
    import basd_amd.losses._ops as O
    trainer, b = _make_preset("deit_tiny_patch16_224", "vit_base_patch16_224", 2, 384, 16)
    assert trainer.model.pos_embed.shape[1] == 577
    O.FALLBACKS.clear()
    O.set_strict(True)
    t0 = time.perf_counter()
    try:
        with O.record_library_gemms() as seen:
            loss, _ = trainer.train_step(b)
            trainer.check_health()
    finally:
        O.set_strict(False)
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    print(f"\n384 px step: {took:.1f} s, library GEMM sites {sorted(seen)}")
    assert float(loss) == float(loss)
    assert not O.FALLBACKS, dict(O.FALLBACKS)
    assert LIB_BMM not in seen, sorted(seen)
    assert took < 120.0, took                  # one step at batch 2, first-launch set-up included

"""The Procrustes backward with N_t != N_s on the entries of csrc/resample.hip: no library GEMM on the way back to the
caller's teacher tokens and importance, the gradients of an fp64 restatement, capturable, and reachable from the C
entries alone.  Shapes: B = 2, D_s = 32, D_t = 48, N_s = 16 against N_t = 16 (nothing to resample), 25 (down) and
9 (up); the inputs are built the way oracle/synth.py builds the fixtures (planted teacher rank, decaying student
spectrum, softmax attention)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, N_S, D_S, D_T = 2, 16, 32, 48
GRAD_TOL = 2e-4           # the project's bound for token gradients on gapped-spectrum inputs (rel-L2 against fp64)


@pytest.fixture(autouse=True)
def _native():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    native.lib()
    _ops.set_ops(None)
    yield native


def _inputs(n_t: int, seed: int = 3):
    from oracle import basd_oracle as O
    from oracle.synth import Shape, make_inputs
    shape = Shape(B=B, N_s=N_S, N_t=n_t, D_s=D_S, D_t=D_T, L_t=1, H=2, C=10, E=1)
    inputs = make_inputs(shape, seed=seed)
    s = inputs["student_tokens"][inputs["token_layers"][0]]
    t = inputs["teacher_tokens"][0]
    imp = O.importance_from_attention(inputs["teacher_attns"][0], True)
    return s.contiguous(), t.contiguous(), imp.contiguous(), torch.tensor([1.0, -0.5])


def _restated(s, t, imp):
    """relational.py's attention-weighted Procrustes value per sample, with F.interpolate for both resamples"""
    n_s = s.shape[1]
    if t.shape[1] != n_s:
        t = F.interpolate(t.transpose(1, 2), size=n_s, mode="linear", align_corners=False).transpose(1, 2)
        imp = F.interpolate(imp.unsqueeze(1), size=n_s, mode="linear", align_corners=False).squeeze(1)
    w = (imp / imp.sum(dim=-1, keepdim=True)).unsqueeze(-1)
    s_c = s - (w * s).sum(dim=1, keepdim=True)
    t_c = t - (w * t).sum(dim=1, keepdim=True)
    s_w, t_w = w.sqrt() * s_c, w.sqrt() * t_c
    nuc = torch.linalg.svdvals(s_w.transpose(1, 2) @ t_w).sum(dim=-1)
    return (s_w * s_w).sum(dim=(1, 2)) + (t_w * t_w).sum(dim=(1, 2)) - 2.0 * nuc


@functools.lru_cache(maxsize=None)
def _reference(n_t: int):
    s, t, imp, gl = _inputs(n_t)
    leaves = [z.double().clone().requires_grad_(True) for z in (s, t, imp)]
    val = _restated(*leaves)
    (val * gl.double()).sum().backward()
    return val.detach(), [z.grad for z in leaves]


def _device_grads(n_t: int, seed: int = 3):
    from basd_amd.losses import functional as BF
    s, t, imp, gl = _inputs(n_t, seed)
    leaves = [z.cuda().requires_grad_(True) for z in (s, t, imp)]
    val = BF.procrustes(*leaves)
    (val * gl.cuda()).sum().backward()
    torch.cuda.synchronize()
    return val.detach(), [z.grad for z in leaves]


def _rel(got, want) -> float:
    return float((got.double().cpu() - want).norm() / want.norm())


def test_backward_reaches_no_library_gemm():
    from basd_amd.losses import _align_token_count
    from basd_amd.losses._ops import record_library_gemms
    seen = {}
    for n_t in (16, 25, 9):
        with record_library_gemms() as rec:
            _device_grads(n_t)
        seen[n_t] = set(rec)
    assert seen[25] <= seen[16] and seen[9] <= seen[16], seen
    assert not seen[16], seen
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(B, 25, D_T, device="cuda").to(dtype).requires_grad_(True)
        with record_library_gemms() as rec:
            out = _align_token_count(x, N_S)
            out.float().square().sum().backward()
        torch.cuda.synchronize()
        assert set(rec) <= seen[16], rec
        assert out.shape == (B, N_S, D_T) and out.dtype == dtype and x.grad.shape == x.shape


@pytest.mark.parametrize("n_t", [16, 25, 9])
def test_gradients_against_fp64(n_t, monkeypatch, _native):
    """The entries and, on the same inputs, the torch chain they replace (``resample_supported`` set aside), both held
    to the same bound: a failure of the first alone is the kernels', a failure of both is the input's."""
    want = _reference(n_t)[1]
    val, got = _device_grads(n_t)
    monkeypatch.setattr(_native, "resample_supported", None)
    val_chain, got_chain = _device_grads(n_t)
    monkeypatch.undo()
    assert torch.equal(val, val_chain)
    errs = {}
    for name, g, gc, w in zip(("s", "t", "imp"), got, got_chain, want):
        errs[name] = (_rel(g, w), _rel(gc, w))
        print(f"N_t = {n_t}: d/d{name} rel-L2 entries {errs[name][0]:.3g}, torch chain {errs[name][1]:.3g}")
    for name, (e_new, e_chain) in errs.items():
        assert e_chain <= GRAD_TOL, (name, "torch chain", e_chain)
        assert e_new <= GRAD_TOL, (name, "entries", e_new)


def test_align_token_count_values(_native):
    from basd_amd.losses import _align_token_count
    from tests import _resample_cases as C
    x = torch.from_numpy(C.data((B, 25, D_T), seed=11))
    g = torch.from_numpy(C.data((B, N_S, D_T), seed=12))
    xd = x.cuda().requires_grad_(True)
    out = _align_token_count(xd, N_S)
    out.backward(g.cuda())
    torch.cuda.synchronize()
    assert torch.equal(out, _native.resample_tokens(x.cuda(), N_S))
    assert torch.equal(xd.grad, _native.resample_tokens_adjoint(g.cuda(), 25))
    torch.testing.assert_close(out.double().cpu(), torch.from_numpy(C.forward(x.numpy(), N_S)), rtol=0, atol=1e-5)
    torch.testing.assert_close(xd.grad.double().cpu(), torch.from_numpy(C.adjoint(g.numpy(), 25)), rtol=0, atol=1e-5)


def test_captured_backward_is_bit_equal_to_eager():
    from basd_amd.losses import functional as BF
    n_t = 25
    s, t, imp, gl = _inputs(n_t)
    leaves = [z.cuda().requires_grad_(True) for z in (s, t, imp)]
    gl = gl.cuda()

    def step():
        for z in leaves:
            z.grad = None
        val = BF.procrustes(*leaves)
        (val * gl).sum().backward()
        return val

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for z in leaves:
        z.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # one stream: the graph has no parallel branches
        val_g = step()
    for seed in (5, 6):
        fresh = _inputs(n_t, seed)[:3]
        with torch.no_grad():
            for z, new in zip(leaves, fresh):
                z.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        val_e, want = _device_grads(n_t, seed)
        assert torch.equal(val_g.detach(), val_e), seed
        for name, z, w in zip(("s", "t", "imp"), leaves, want):
            assert torch.equal(z.grad, w), (seed, name)


@pytest.mark.parametrize("n_t", [16, 25, 9])
def test_c_only_sequence_reproduces_autograd(n_t, _native):
    """prep -> fwd -> bwd -> basd_resample_tokens_adjoint + basd_procrustes_importance_bwd through the raw wrappers:
    bit for bit the gradients of the Python path.  With equal counts the Python path keeps its three fp32 pointwise
    launches for the importance, so there the entry (fp64, rounded once) is held to their error instead: the fp32 dot
    of N_s terms, the subtraction and the division, (N_s + 3) 2^-24 (|g_a| + sum |a g_a|) / tot per element."""
    from basd_amd.losses import functional as BF
    val, want = _device_grads(n_t)
    s, t, imp, gl = (z.cuda() for z in _inputs(n_t))
    s_w, t_w, a, tr = _native.procrustes_prep(s, t, imp)
    nuc, fac_s, a_t = _native.procrustes_fwd(s_w, t_w, BF.PCHOL_TOL)
    g_s, g_t, g_a = _native.procrustes_bwd(s_w, t_w, a, gl, fac_s, a_t, torch.float32)
    g_imp = _native.procrustes_importance_bwd(g_a, a, imp)
    if n_t != N_S:
        g_t = _native.resample_tokens_adjoint(g_t, n_t)
    torch.cuda.synchronize()
    assert torch.equal(tr[:, 0] + tr[:, 1] - 2.0 * nuc, val)
    for name, got, w in zip(("s", "t"), (g_s, g_t), want):
        assert got.shape == w.shape and torch.equal(got, w), name
    if n_t != N_S:
        assert torch.equal(g_imp, want[2])
    else:
        ga, ad, tot = g_a.double(), a.double(), imp.double().sum(-1, keepdim=True)
        tol = (N_S + 3) * 2.0 ** -24 * (ga.abs() + (ad * ga).abs().sum(-1, keepdim=True)) / tot
        assert bool(((g_imp.double() - want[2].double()).abs() <= tol).all())

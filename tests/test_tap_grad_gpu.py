"""The two entries of csrc/tap_grad.hip on the GPU: the selector's token gradient per element against fp64 (with the
torch chain it replaces held to the same bound), the tap scatter bit for bit against autograd's bf16 chain, and one
c1-sized train step with the new path on and forced off."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5), (2, 67), (5, 64)]        # B, N: rows = 15 (part of one wave), 134, 320 (two tiles, ragged second)
GUARD = 3                                  # sentinel rows behind every output tensor
SENTINEL = -7.0


def _tokens(e, b, n, d, kind, gen):
    """E CLS-stripped bf16 views of [B, N + 1, D] buffers whose CLS rows hold 1e4 (a read outside the view shows in
    the mean); kind "offset": column mean 30, standard deviation 1 (the centring cancels the leading digits)"""
    views = []
    for _ in range(e):
        buf = torch.randn(b, n + 1, d, generator=gen, device="cuda") + (30.0 if kind == "offset" else 0.0)
        buf[:, 0, :] = 1e4
        views.append(buf.bfloat16()[:, 1:, :])
    return views


def _weights(e, d, gen):
    """non-symmetric, entries of magnitude 1 and 1e-3 mixed"""
    w = torch.randn(e, d, d, generator=gen, device="cuda")
    small = torch.rand(e, d, d, generator=gen, device="cuda") < 0.5
    return torch.where(small, w * 1e-3, w).contiguous()


def _torch_chain(s, w):
    """the lines of _SelectorWeightsFn.backward that the entry replaces"""
    sf = s.float().reshape(-1, s.shape[-1])
    row = -(sf.mean(dim=0, keepdim=True) @ w)
    return torch.addmm(row, sf, w).reshape(s.shape).to(s.dtype)


def _check_against_fp64(y, s, w, what):
    d = s.shape[-1]
    s64 = s.double().reshape(-1, d)
    w64 = w.double()
    mean = s64.mean(dim=0, keepdim=True)
    y64 = (s64 - mean) @ w64
    # one bf16 ulp (double rounding at a tie) + twice the fp32 accumulation bound: the centring is s W - mean W
    bound = 2.0 ** -8 * y64.abs() + d * 2.0 ** -23 * ((s64.abs() + mean.abs()) @ w64.abs())
    err = (y.double().reshape(-1, d) - y64).abs()
    worst = float((err / bound).max())
    print(f"{what}: max |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def _run_selector_case(d, e, b, n):
    import basd_amd._native as native
    gen = torch.Generator(device="cuda").manual_seed(1000 * d + 10 * e + n)
    for kind in ("centred", "offset"):
        toks = _tokens(e, b, n, d, kind, gen)
        w = _weights(e, d, gen)
        raw = [torch.full((b * n + GUARD, d), SENTINEL, dtype=torch.bfloat16, device="cuda") for _ in range(e)]
        outs = [r[:b * n].view(b, n, d) for r in raw]
        got = native.selector_token_grad(toks, w, out=outs)
        torch.cuda.synchronize()
        for i in range(e):
            assert got[i].data_ptr() == outs[i].data_ptr()
            assert bool((raw[i][b * n:] == SENTINEL).all()), "rows behind the output were written"
            _check_against_fp64(outs[i], toks[i], w[i], f"kernel D={d} E={e} B={b} N={n} {kind} tap {i}")
            _check_against_fp64(_torch_chain(toks[i], w[i]), toks[i], w[i], f"torch chain D={d} {kind} tap {i}")
            assert bool((toks[i]._base[:, 0, :] == 1e4).all())


@pytest.mark.parametrize("b,n", SHAPES)
@pytest.mark.parametrize("e", [1, 3])
@pytest.mark.parametrize("d", [192, 384])
def test_selector_token_grad_against_fp64(d, e, b, n):
    _run_selector_case(d, e, b, n)


def test_selector_token_grad_against_fp64_at_768():
    _run_selector_case(768, 3, 2, 67)


def test_selector_token_grad_takes_contiguous_tokens_and_many_tiles():
    """contiguous [B, N, D] tokens (batch stride N D) and more (tap, tile) items than workgroups: 3 x 89 > 256, so
    workgroups walk several tiles and some of them cross from one tap into the next"""
    import basd_amd._native as native
    gen = torch.Generator(device="cuda").manual_seed(7)
    b, n, d = 115, 197, 192
    toks = [(torch.randn(b, n, d, generator=gen, device="cuda") + 3.0 * i).bfloat16() for i in range(3)]
    w = _weights(3, d, gen)
    got = native.selector_token_grad(toks, w)
    for i in range(3):
        _check_against_fp64(got[i], toks[i], w[i], f"contiguous tap {i}")


@pytest.mark.parametrize("absent", ["none", "g_out", "g_a", "g_b"])
@pytest.mark.parametrize("offset", [1, 0])
@pytest.mark.parametrize("b,n", SHAPES)
def test_tap_grad_scatter_is_bit_equal_to_autograds_chain(b, n, offset, absent):
    import basd_amd._native as native
    gen = torch.Generator(device="cuda").manual_seed(100 * n + 10 * offset + len(absent))
    for d in (64, 192):
        t = n + offset
        g_out = torch.randn(b, t, d, generator=gen, device="cuda").bfloat16() if absent != "g_out" else None
        g_a = torch.randn(b, n, d, generator=gen, device="cuda").bfloat16() if absent != "g_a" else None
        g_b = (3.0 * torch.randn(b, n, d, generator=gen, device="cuda")).bfloat16() if absent != "g_b" else None
        tok = g_a + g_b if (g_a is not None and g_b is not None) else (g_a if g_a is not None else g_b)
        want = F.pad(tok, (0, 0, offset, 0))
        if g_out is not None:
            want = g_out + want
        got = native.tap_grad_scatter(g_out, g_a, g_b, (b, t, d), offset)
        assert got.dtype == torch.bfloat16 and got.shape == (b, t, d)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (d, absent, offset)


# ---------------------------------------------------------------------------------------------------------------------
CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")

# Two runs of one build differ by this much in relative L2 (bench.py's docstring: parameters 2e-3); the flat gradient of
# this step measured smaller on the parent commit (docstring of the test), so the docstring's figure stands.
RUN_TO_RUN = 2e-3


def _one_step(captured: bool):
    """-> (loss, flat gradient) of the first train step of a freshly built c1-sized trainer"""
    from basd_amd.config import load_config
    from basd_amd.train import SyntheticLoader, build
    torch.manual_seed(0)
    cfg = load_config(CFG, "basd_cifar100", ["data.batch_size=4", "model.drop_path_rate=0.0"])
    trainer, _ = build(cfg, device="cuda")
    trainer.use_mixup = False
    trainer.optimizer.train()
    trainer.model.train()
    batch = next(iter(SyntheticLoader(4, 32, 100, 1, "cuda", seed=5)))
    if captured:
        assert trainer.enable_graph(batch), trainer.graph_error
    grads = []
    step = trainer.optimizer.step

    def snapshot():
        grads.append(trainer.flat.grad.clone())
        return step()
    trainer.optimizer.step = snapshot
    loss, _ = trainer.train_step(batch)
    torch.cuda.synchronize()
    trainer.check_health()
    return loss.detach().clone(), grads[0]


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_one_step_fused_against_fallback(captured, monkeypatch):
    """One c1-sized step (width 192, 32 px, patch 4, batch 4) with the two entries on and with both forced off through
    their ``*_supported`` predicates: the loss is bit-equal (the forward is untouched), the flat gradient agrees to
    2 x the run-to-run distance of one build.

    Measured on an MI355X (profiles/tap_grad_ab.txt): the losses were equal to the bit; the flat gradients were
    4.72e-08 (eager) and 4.73e-08 (captured) apart in relative L2.  Two runs of the parent commit on the same inputs
    were 3.4e-08 .. 4.1e-08 apart (losses equal to the bit), which is below the 2e-3 of bench.py's docstring, so the
    bound is 2 x 2e-3."""
    import basd_amd._native as native
    calls = {"grad": 0, "scatter": 0}
    real_grad, real_scatter = native.selector_token_grad, native.tap_grad_scatter
    monkeypatch.setattr(native, "selector_token_grad",
                        lambda *a, **k: (calls.__setitem__("grad", calls["grad"] + 1), real_grad(*a, **k))[1])
    monkeypatch.setattr(native, "tap_grad_scatter",
                        lambda *a, **k: (calls.__setitem__("scatter", calls["scatter"] + 1), real_scatter(*a, **k))[1])
    loss_on, grad_on = _one_step(captured)
    assert calls["grad"] >= 1 and calls["scatter"] >= 1, calls        # the step took the new path
    used = dict(calls)
    monkeypatch.setattr(native, "selector_token_grad_supported", lambda d: False)
    monkeypatch.setattr(native, "tap_grad_scatter_supported", lambda d: False)
    loss_off, grad_off = _one_step(captured)
    assert calls == used, "the forced-off step still called the new entries"
    rel = float((grad_on - grad_off).norm() / grad_off.norm())
    print(f"captured={captured}: loss on {float(loss_on)!r} off {float(loss_off)!r}, flat gradient rel L2 {rel:.3e}")
    assert torch.equal(loss_on, loss_off)
    assert rel <= 2 * RUN_TO_RUN, rel

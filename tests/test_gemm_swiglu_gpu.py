"""basd_gemm_bf16_swiglu (csrc/gemm_bf16.hip, EPI 8): the w12 GEMM of a SwiGLU MLP with the gate in its epilogue, on both
kernels the entry can reach (GPU box only).

The entry launches the persistent ring kernel where ``pring_cus_per_xcd(M, 2 H) == 32 and K >= 192`` and the ring kernel
for every other shape (tests/_gemm_cases.py mirrors the launcher).  Cases (M, H, K):
  * ring:  (300, 128, 64)   one column tile, ONE K step, a full and a ragged row block;
           (300, 256, 64)   two column tiles;
           (300, 128, 320)  five K steps: the ring's prologue, steady state and tail;
  * pring: (3841, 2048, 192)  the smallest M that selects it at this width (16 row blocks, one tile per workgroup), the
                              smallest K it takes, M % 256 == 1;
           (5889, 2048, 192)  24 row blocks: workgroups that multiply a second tile behind an epilogue (the counted wait
                              on the epilogue's 8 stores), which is also where ``tile_run`` changes the launch.

Yardstick (DESIGN "Evaluation precision", the rule for a reordered fp32 computation): the contract evaluated in fp64 on
the same bf16 inputs; the kernel's largest error and its relative L2 error against it may be at most TWICE those of a
plain torch fp32 emulation of the contract (fp32 matmul, fp32 bias add, fp32 silu * x2, one rounding to bf16).
"""
import pytest
import torch
import torch.nn.functional as F

from tests import _gemm_cases as C

pytestmark = pytest.mark.gpu

CASES = {(300, 128, 64): "ring", (300, 256, 64): "ring", (300, 128, 320): "ring",
         (3841, 2048, 192): "pring", (5889, 2048, 192): "pring"}
GUARD = 4096                     # elements in front of the output
TAIL = 8                         # rows behind M
BASD_ERR_SHAPE = 1
ZERO_ROW = 1


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    _INPUTS.clear()


_INPUTS = {}


def _inputs(case):
    """bf16 inputs from a fixed seed (hub layout: rows 0 .. H - 1 of w12 are the gated half) with pre-activations of
    standard deviation 3 (beyond +-8 on both sides: the sigmoid saturates) and one all-zero row of x; the fp64 contract
    and the fp32 emulation's errors against it.  Built once per case and shared, never modified."""
    if case not in _INPUTS:
        M, H, K = case
        g = torch.Generator().manual_seed(1_000_003 * M + 1009 * H + K)
        x = torch.randn(M, K, generator=g).bfloat16()
        x[ZERO_ROW] = 0
        w12 = (3.0 * torch.randn(2 * H, K, generator=g) / K ** 0.5).bfloat16()
        b12 = torch.randn(2 * H, generator=g).bfloat16()
        a = x.double() @ w12.double().t() + b12.double()
        a1, a2 = a.chunk(2, dim=-1)
        assert float(a1.max()) >= 8.0 and float(a1.min()) <= -8.0
        ref = a1 / (1.0 + torch.exp(-a1)) * a2
        e1, e2 = (x.float() @ w12.float().t() + b12.float()).chunk(2, dim=-1)
        emul = (F.silu(e1) * e2).bfloat16()
        _INPUTS[case] = dict(x=x.cuda(), w12=w12.cuda(), b12=b12.cuda(), ref=ref, emul_err=_errors(emul, ref))
    return _INPUTS[case]


def _errors(y, ref):
    d = y.double().cpu() - ref
    return float(d.abs().max()), float(d.norm() / ref.norm())


def _swiglu(nat, inp, case, tile_run=0, bias=True):
    """the C entry on the packed operands, the output between a guard frame and TAIL sentinel rows -> [M, H]"""
    M, H, K = case
    wp, bp = nat.swiglu_pack(inp["w12"], inp["b12"])
    buf = torch.full((GUARD + (M + TAIL) * H,), C.SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    y = buf[GUARD:GUARD + M * H]
    rc = nat.lib().basd_gemm_bf16_swiglu(nat._ptr(inp["x"]), nat._ptr(wp), nat._ptr(bp if bias else None), nat._ptr(y),
                                         M, H, K, tile_run, nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    bits = buf.view(torch.int16)
    assert bool((bits[:GUARD] == C.SENTINEL).all()), "written in front of the output"
    assert bool((bits[GUARD + M * H:] == C.SENTINEL).all()), "rows behind M were written"
    assert not bool((y.view(torch.int16) == C.SENTINEL).any()), "an element of the output was not written"
    return y.view(M, H)


def test_cases_reach_both_kernels():
    for (M, H, K), kernel in CASES.items():
        pring = C.pring_cus_per_xcd(M, 2 * H) == 32 and K >= 192
        assert ("pring" if pring else "ring") == kernel, (M, H, K)
        assert M % C.GBM != 0 and M > C.GBM                         # a full and a ragged row block
    # the smallest M that selects the persistent kernel at N = 4096
    assert C.pring_cus_per_xcd(3840, 4096) < 32 and C.pring_cus_per_xcd(3841, 4096) == 32
    # a workgroup of the larger case multiplies two tiles
    assert max(C.schedule(5889, 4096, 192).tiles_per_workgroup) == 2


@pytest.mark.parametrize("case", list(CASES), ids=C.case_id)
def test_gate_against_fp64_like_the_fp32_emulation(nat, case):
    """Measured on an MI355X: profiles/gemm_swiglu_margins.txt (kernel error / emulation error: 1.00 for the largest
    error -- the bf16 rounding decides -- and 1.00 for rel-L2)."""
    inp = _inputs(case)
    y = _swiglu(nat, inp, case)
    assert bool(torch.isfinite(y.float()).all())
    got, emul = _errors(y, inp["ref"]), inp["emul_err"]
    print(f"gemm-swiglu-margin {C.case_id(case)} {CASES[case]}: max err {got[0]:.4e} (emulation {emul[0]:.4e}, ratio "
          f"{got[0] / emul[0]:.3f}), rel-L2 {got[1]:.4e} (emulation {emul[1]:.4e}, ratio {got[1] / emul[1]:.3f})")
    assert got[0] <= 2.0 * emul[0] and got[1] <= 2.0 * emul[1], (got, emul)
    # the all-zero row: the gate of the two biases alone
    b1, b2 = inp["b12"].double().cpu().chunk(2)
    want = (b1 / (1.0 + torch.exp(-b1)) * b2).bfloat16()
    assert torch.equal(y[ZERO_ROW].cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("case", [(300, 256, 64), (5889, 2048, 192)], ids=C.case_id)
def test_without_a_bias(nat, case):
    inp = _inputs(case)
    y = _swiglu(nat, inp, case, bias=False)
    a1, a2 = (inp["x"].double().cpu() @ inp["w12"].double().cpu().t()).chunk(2, dim=-1)
    ref = a1 / (1.0 + torch.exp(-a1)) * a2
    e1, e2 = (inp["x"].float().cpu() @ inp["w12"].float().cpu().t()).chunk(2, dim=-1)
    got, emul = _errors(y, ref), _errors((F.silu(e1) * e2).bfloat16(), ref)
    assert got[0] <= 2.0 * emul[0] and got[1] <= 2.0 * emul[1], (got, emul)
    assert not bool(y[ZERO_ROW].float().abs().any())


@pytest.mark.parametrize("case", [(300, 256, 64), (3841, 2048, 192), (5889, 2048, 192)], ids=C.case_id)
def test_tile_run_does_not_change_a_bit(nat, case):
    inp = _inputs(case)
    want = _swiglu(nat, inp, case, tile_run=0)
    for tile_run in (1, -16):
        got = _swiglu(nat, inp, case, tile_run=tile_run)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), tile_run


def test_large_preactivations_saturate_without_overflow(nat):
    """x scaled by 32 (exact in bf16): gated pre-activations beyond +-200, where exp2 overflows to +inf (the result is
    -0 or a tiny negative times x2, not NaN) or underflows to 0 (the result is x1 * x2)."""
    case = (300, 256, 64)
    inp = _inputs(case)
    big = dict(inp, x=(inp["x"].float() * 32.0).bfloat16())
    y = _swiglu(nat, big, case).cpu()
    a1, a2 = (big["x"].double().cpu() @ inp["w12"].double().cpu().t() + inp["b12"].double().cpu()).chunk(2, dim=-1)
    assert float(a1.max()) >= 200.0 and float(a1.min()) <= -200.0
    assert bool(torch.isfinite(y.float()).all())
    assert float(y[a1 <= -100.0].float().abs().max()) <= 1e-30
    ref = torch.where(a1 < -700.0, torch.zeros_like(a1), a1 / (1.0 + torch.exp(-a1.clamp_min(-700.0))) * a2)
    e1, e2 = (big["x"].float().cpu() @ inp["w12"].float().cpu().t() + inp["b12"].float().cpu()).chunk(2, dim=-1)
    got, emul = _errors(y, ref), _errors((F.silu(e1) * e2).bfloat16(), ref)
    assert got[0] <= 2.0 * emul[0] and got[1] <= 2.0 * emul[1], (got, emul)


@pytest.mark.parametrize("H,K", [(192, 64), (128, 96), (64, 64), (128, 0)])
def test_unsupported_shapes_are_refused_before_the_launch(nat, H, K):
    z = torch.zeros(512 * 512, dtype=torch.bfloat16, device="cuda")
    y = torch.full((300 * 256,), C.SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    rc = nat.lib().basd_gemm_bf16_swiglu(nat._ptr(z), nat._ptr(z), nat._ptr(z), nat._ptr(y), 300, H, K, 0, nat._stream())
    torch.cuda.synchronize()
    assert rc == BASD_ERR_SHAPE and b"gemm_bf16_swiglu" in nat.lib().basd_last_error()
    assert bool((y.view(torch.int16) == C.SENTINEL).all()), "a refused call wrote to y"
    assert not nat.gemm_swiglu_supported(H, K)


def test_wrapper_is_the_entry(nat):
    case = (300, 256, 64)
    inp = _inputs(case)
    wp, bp = nat.swiglu_pack(inp["w12"], inp["b12"])
    got = nat.gemm_bf16_swiglu(inp["x"].view(3, 100, 64), wp, bp)
    assert got.shape == (3, 100, 256)
    assert torch.equal(got.view(300, 256).view(torch.int16), _swiglu(nat, inp, case).view(torch.int16))
    # and it is the unfused composition up to the extra rounding of w12's output
    x1, x2 = nat.gemm_bf16(inp["x"], inp["w12"], inp["b12"]).chunk(2, dim=-1)
    plain = (F.silu(x1) * x2).float()
    rel = float((got.view(300, 256).float() - plain).norm() / plain.norm())
    assert 0.0 < rel < 2e-2, rel

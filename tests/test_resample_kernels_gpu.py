"""The three entries of csrc/resample.hip against the fp64 restatement of tests/_resample_cases.py.

Bounds (derived from the arithmetic, not measured).  An output element is a chain of c FMAs / products over its c terms
(tests/_resample_cases.terms) of fp32 values g_i with weights w in {1 - fr, fr}: fr is exact, 1 - fr carries one
rounding, the first term passes through c roundings, so |err| <= (c + 1) u S + O(u^2) with u = 2^-24 and
S = sum |w_ij| |g_i|; the tests hold (c + 2) u S.  A bf16 output adds its own rounding, held at 2^-8 |result|.
The importance backward is computed in fp64 and rounded once: 2 u sum_i w_ij |g_v[i]| plus the smallest fp32
denormal.  Every output lives inside a larger buffer pre-filled with NaN between two canary margins."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _resample_cases as C

pytestmark = pytest.mark.gpu

U24 = C.U24
MARGIN = 64               # canary elements on either side (a multiple of 16 bytes for both dtypes)
CANARY = 12345.0
ERR_SHAPE = 1             # BASD_ERR_SHAPE of include/basd_hip.h


@pytest.fixture(autouse=True)
def _native():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    native.lib()
    _ops.set_ops(None)
    yield native


def _framed(shape, dtype, shift: int):
    """a NaN-filled tensor of ``shape`` inside a canary-framed flat buffer; ``shift`` elements past 16-byte alignment"""
    n = int(np.prod(shape))
    flat = torch.full((2 * MARGIN + n + shift,), CANARY, dtype=dtype, device="cuda")
    view = flat[MARGIN + shift:MARGIN + shift + n]
    view.fill_(float("nan"))
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (shift * flat.element_size()) % 16
    return flat, view.view(shape)


def _frame_intact(flat, shape, shift: int) -> bool:
    n = int(np.prod(shape))
    edge = torch.cat([flat[:MARGIN + shift], flat[MARGIN + shift + n:]])
    return bool((edge == CANARY).all())


def _shifted_input(x: torch.Tensor, shift: int) -> torch.Tensor:
    flat = torch.zeros(x.numel() + shift, dtype=x.dtype, device="cuda")
    flat[shift:].copy_(x.reshape(-1))
    return flat[shift:].view(x.shape)


def _check_tokens(native, n_in, n_out, batch, d, dtype, adjoint: bool, shift: int = 0):
    what = f"{'adjoint' if adjoint else 'forward'} {n_in} -> {n_out}, batch {batch}, d {d}, {dtype}, shift {shift}"
    n_src, n_dst = (n_out, n_in) if adjoint else (n_in, n_out)
    x = torch.from_numpy(C.data((batch, n_src, d), seed=n_in * 4099 + n_out * 7 + d + batch)).to(dtype)
    x64 = x.double().numpy()
    if adjoint:
        want, scale, c = C.adjoint(x64, n_in), C.adjoint(np.abs(x64), n_in), C.terms(n_in, n_out)[1]
    else:
        want, scale, c = C.forward(x64, n_out), C.forward(np.abs(x64), n_out), C.terms(n_in, n_out)[0]
    tol = (c[None, :, None] + 2) * U24 * scale
    if dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * np.abs(want)
    run = native.resample_tokens_adjoint if adjoint else native.resample_tokens
    xd = _shifted_input(x.cuda(), shift)
    outs = []
    for _ in range(2):
        flat, out = _framed((batch, n_dst, d), dtype, shift)
        run(xd, n_dst, out=out)
        torch.cuda.synchronize()
        assert _frame_intact(flat, out.shape, shift), what
        outs.append(out.clone())
    got = outs[0].double().cpu().numpy()
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} elements left unwritten"
    if adjoint:
        assert (got[:, c == 0, :] == 0).all(), what
    over = np.abs(got - want) - tol
    assert (over <= 0).all(), f"{what}: over the bound by {float(over.max()):.3g} at {np.unravel_index(over.argmax(), over.shape)}"
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), f"{what}: two runs differ"


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("n_in,n_out", C.PAIRS)
def test_tokens_against_fp64(_native, n_in, n_out, adjoint):
    for batch in C.BATCHES:
        for d in C.WIDTHS:
            for dtype in (torch.float32, torch.bfloat16):
                _check_tokens(_native, n_in, n_out, batch, d, dtype, adjoint)


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("n_in,n_out", C.PAIRS)
def test_tokens_with_the_base_offset_by_four_bytes(_native, n_in, n_out, adjoint):
    """input and output 4 bytes past a 16-byte boundary: the one-element fp32 path and the two-element bf16 path"""
    _check_tokens(_native, n_in, n_out, 3, 36, torch.float32, adjoint, shift=1)
    _check_tokens(_native, n_in, n_out, 3, 36, torch.bfloat16, adjoint, shift=2)


def test_bf16_vector_paths(_native):
    """bf16 with d % 8 != 0 takes 8-byte accesses from an aligned base (d = 4, 36, 260 above).  Here the others:
    d % 8 == 0 from an aligned base (16 bytes), from a base 8 bytes past alignment (8 bytes), and a base 2 bytes past
    alignment (single elements)."""
    for adjoint in (False, True):
        for n_in, n_out in ((13, 17), (17, 13), (3, 1024)):
            _check_tokens(_native, n_in, n_out, 3, 40, torch.bfloat16, adjoint)
        _check_tokens(_native, 17, 13, 3, 40, torch.bfloat16, adjoint, shift=4)
        _check_tokens(_native, 13, 17, 3, 36, torch.bfloat16, adjoint, shift=1)


@pytest.mark.parametrize("n_t,n_s", C.PAIRS)
def test_importance_backward_against_fp64(_native, n_t, n_s):
    for batch in C.BATCHES:
        what = f"importance backward n_t {n_t}, n_s {n_s}, batch {batch}"
        rng = np.random.default_rng(n_t * 131 + n_s + batch)
        imp = (rng.random((batch, n_t)) + 0.1).astype(np.float32)
        g_a = rng.standard_normal((batch, n_s)).astype(np.float32)
        v = C.forward(imp[:, :, None], n_s)[:, :, 0]
        a = (v / v.sum(axis=1, keepdims=True)).astype(np.float32)          # what the prep kernel hands on, as fp32
        want, scale = C.importance_bwd(g_a, a, imp)
        tol = 2 * U24 * scale + 2.0 ** -149
        dev = [torch.from_numpy(np.ascontiguousarray(z)).cuda() for z in (g_a, a, imp)]
        outs = []
        for _ in range(2):
            flat, out = _framed((batch, n_t), torch.float32, 0)
            _native.procrustes_importance_bwd(*dev, out=out)
            torch.cuda.synchronize()
            assert _frame_intact(flat, out.shape, 0), what
            outs.append(out.clone())
        got = outs[0].double().cpu().numpy()
        assert not np.isnan(got).any(), what
        over = np.abs(got - want) - tol
        assert (over <= 0).all(), f"{what}: over the bound by {float(over.max()):.3g}"
        assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), f"{what}: two runs differ"


def test_error_paths_launch_nothing(_native):
    """n = 0, n = 1025, d = 6 and a NULL pointer: BASD_ERR_SHAPE, a message, and the output as it was.  Every pointer
    that is passed is a real allocation large enough for the nearest valid shape: nothing here could fault."""
    lib = _native.lib()
    x = torch.zeros(2 * 1024 * 8, dtype=torch.float32, device="cuda")
    out = torch.full((2 * 1024 * 8,), CANARY, dtype=torch.float32, device="cuda")
    p, null, st = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(0), _native._stream()
    po = ctypes.c_void_p(out.data_ptr())
    bad_tokens = [
        dict(n_in=0), dict(n_out=0), dict(n_in=1025), dict(n_out=1025), dict(d=6), dict(d=0), dict(batch=0),
        dict(x=null), dict(out=null),
    ]
    for entry in (lib.basd_resample_tokens, lib.basd_resample_tokens_adjoint):
        for kw in bad_tokens:
            a = dict(x=p, dtype=0, batch=2, n_in=16, n_out=8, d=8, out=po)
            a.update(kw)
            rc = entry(a["x"], a["dtype"], a["batch"], a["n_in"], a["n_out"], a["d"], a["out"], st)
            assert rc == ERR_SHAPE and lib.basd_last_error(), kw
    for kw in (dict(n_s=0), dict(n_t=0), dict(n_s=1025), dict(n_t=1025), dict(batch=0), dict(g_a=null), dict(a=null),
               dict(imp=null), dict(out=null)):
        a = dict(g_a=p, a=p, imp=p, batch=2, n_s=16, n_t=8, out=po)
        a.update(kw)
        rc = lib.basd_procrustes_importance_bwd(a["g_a"], a["a"], a["imp"], a["batch"], a["n_s"], a["n_t"], a["out"], st)
        assert rc == ERR_SHAPE and lib.basd_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    assert not _native.resample_supported(0, 8, 8, torch.float32) and not _native.resample_supported(8, 1025, 8, torch.float32)
    assert not _native.resample_supported(8, 8, 6, torch.float32) and not _native.resample_supported(8, 8, 8, torch.float64)
    assert _native.resample_supported(1, 1024, 4, torch.bfloat16)

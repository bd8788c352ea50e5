"""The fp64 batched GEMM of csrc/bgemm_f64.hip -- the generic kernel, the pipelined fast kernel (plain and symmetric, with
and without a problem mask) and the balanced Gram kernel -- per element against a long-double reference on every dispatch
path (GPU box only).  tests/_bgemm_cases.py holds the cases, the inputs, the reference and the DERIVED bound
(|c - ref| <= gamma_K |op A| |op B|, plus one fp32 rounding for an fp32 output; margin 1), and says which kernel a case
reaches; tests/test_bgemm_cases_cpu.py pins that and proves that the bound rejects nearly right kernels.

The C entries are called directly, so that the path is the one named.  Every output is a caller-owned buffer with
ldc = N + 3, five elements between the matrices and 64 behind the last, pre-filled with a NaN pattern no kernel produces:
inside M x N nothing of it may be left, outside it every bit must be.  Operand buffers hold NaN wherever the entry has no
business reading (leading-dimension padding, gaps between matrices, the matrices of masked problems).

With ``pytest -s`` the worst err / bound per path and regime is printed when the module is done; profiles/bgemm_f64_margins.txt
keeps one run's table."""
import ctypes

import pytest
import torch

from tests import _bgemm_cases as C

pytestmark = pytest.mark.gpu

POISON_F32 = 0x7FC00D1E
POISON_F64 = 0x7FF8000000D1E5ED

_WORST = {}          # (path label, output dtype, regime, what) -> (largest err / bound, case)


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    for (lab, dtc, regime, what), (v, where) in sorted(_WORST.items()):
        print(f"bgemm-f64-worst {lab} ->{dtc} {regime} {what}: {v:.4f} at {where}")


def _poisoned(n, dtype):
    if dtype == torch.float32:
        return torch.full((n,), POISON_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n,), POISON_F64, dtype=torch.int64, device="cuda").view(torch.float64)


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _poison_of(t):
    return {torch.float32: POISON_F32, torch.float64: POISON_F64}[t.dtype]


def _untouched(t) -> bool:
    return bool((_bits(t) == _poison_of(t)).all())


def _same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _direct(nat, c, regime):
    """one direct call of the entry on the case's buffers -> (out [batch, M, N] on the CPU, device operands (a, b))"""
    lay = C.layout(c)
    opa, opb = C.operands(c, regime)
    a_buf = C.stored(c, "a", opa).cuda()
    a = a_buf[lay.a_lead:]
    b = a if c.same else C.stored(c, "b", opb).cuda()
    assert a.data_ptr() % 32 == c.a_off and b.data_ptr() % 32 == (c.a_off if c.same else 0)
    if c.same:                                       # one buffer serves as both operands: their layouts must agree
        assert (lay.a_shape, lay.lda, lay.a_stride) == (lay.b_shape, lay.ldb, lay.b_stride)
    dtc = C.TORCH_DTYPE[c.dtc]
    out = _poisoned(c.batch * lay.c_stride + C.C_GUARD, dtc)
    mask = C.skip_mask(c)
    skip = None if mask is None else torch.from_numpy(mask).cuda()
    i64, lib = ctypes.c_int64, nat.lib()
    args = (_ptr(a), C.DTYPE_CODE[c.dta], i64(lay.a_stride), lay.lda, int(c.ta), _ptr(b), C.DTYPE_CODE[c.dtb],
            i64(lay.b_stride), lay.ldb, int(c.tb), _ptr(out), C.DTYPE_CODE[c.dtc], i64(lay.c_stride), lay.ldc, c.batch,
            c.M, c.N, c.K, int(c.sym))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if skip is None:
        rc = lib.basd_bgemm_f64(*args, stream)
    else:
        rc = lib.basd_bgemm_f64_masked(*args, _ptr(skip), stream)
    assert rc == 0, lib.basd_last_error()
    torch.cuda.synchronize()
    host = out.cpu()
    # what must not be written: the padding columns, the gap behind every matrix, the guard, masked problems
    assert _untouched(host[c.batch * lay.c_stride:]), "written behind the last matrix"
    mats = []
    for m in range(c.batch):
        slot = host[m * lay.c_stride:(m + 1) * lay.c_stride]
        if mask is not None and mask[m]:
            assert _untouched(slot), f"masked matrix {m} was written"
            mats.append(torch.full((c.M, c.N), float("nan"), dtype=dtc))
            continue
        assert _untouched(slot[c.M * lay.ldc:]), f"the gap behind matrix {m} was written"
        block = slot[:c.M * lay.ldc].view(c.M, lay.ldc)
        assert _untouched(block[:, c.N:]), f"padding columns of matrix {m} were written"
        inside = block[:, :c.N].contiguous()
        assert not bool((_bits(inside) == _poison_of(inside)).any()), f"poison left inside matrix {m}"
        assert not bool(torch.isnan(inside).any()), f"NaN in matrix {m}"
        mats.append(inside)
    return torch.stack(mats), (a, b)


def _judge(c, regime, out):
    """"product": the elements a kernel computes (all of them, or the lower triangle in symmetric mode) under the plain
    bound; "copied": the whole symmetric matrix under the bound of a copied element (1.0000 by construction where the
    operands are symmetric in exact arithmetic only and the asymmetry dwarfs gamma_K S)"""
    got = C.judge(c, regime, out.numpy())
    got = {"product": got["lower"], "copied": got["elem"]} if c.sym else {"product": got["elem"]}
    print(f"bgemm-f64-bound {C.case_id(c)} {regime} " + " ".join(f"{k} {v:.4f}" for k, v in sorted(got.items())))
    for what, v in got.items():
        key = (C.label(c) + ("-masked" if c.masked else ""), c.dtc, regime, what)
        if v >= _WORST.get(key, (-1.0, None))[0]:
            _WORST[key] = (v, C.case_id(c))
    assert max(got.values()) <= C.MARGIN, (C.case_id(c), regime, got)
    if c.sym and c.inputs == "xxt":
        assert _same_bits(out, out.transpose(1, 2)), "X X^T is not bitwise symmetric"


def _check(nat, c):
    assert C.path_of(c) == c.path
    for regime in C.regimes(c):
        out, _ops = _direct(nat, c, regime)
        _judge(c, regime, out)


@pytest.mark.parametrize("c", C.GENERIC_CASES, ids=C.case_id)
def test_generic_kernel(nat, c):
    _check(nat, c)


@pytest.mark.parametrize("c", C.FAST_CASES, ids=C.case_id)
def test_fast_kernel(nat, c):
    _check(nat, c)


@pytest.mark.parametrize("c", C.KNOCKED_OFF + [C.FAST_TWIN], ids=C.case_id)
def test_aligned_shape_knocked_off_the_fast_path(nat, c):
    """one arm of the alignment predicate each (lda, batch stride, base address) and the plain fast twin: every one against
    the reference, not against each other"""
    lay = C.layout(c)
    assert (lay.lda % 4, lay.a_stride % 4, c.a_off) in ((2, 0, 0), (0, 2, 0), (0, 0, 16), (0, 0, 0))
    _check(nat, c)


@pytest.mark.parametrize("c", C.FAST_SYM_CASES, ids=C.case_id)
def test_fast_kernel_symmetric_two_buffers(nat, c):
    """the sub-tile logic and the mirror of the diagonal tiles at ragged sizes: training reaches it through
    bgemm_f64(s_w, h, trans_a=True, symmetric=True) and the masked pair products only"""
    _check(nat, c)


@pytest.mark.parametrize("c", C.XGX_CASES, ids=C.case_id)
def test_fast_kernel_symmetric_in_exact_arithmetic_only(nat, c):
    """C = X^T (G X): the lower triangle is the product, the upper one its copy"""
    _check(nat, c)


@pytest.mark.parametrize("c", C.MASKED_CASES, ids=C.case_id)
def test_problem_mask(nat, c):
    """batch 11 (the XCD deal wraps), NaN operands behind the mask: masked outputs stay poison bit for bit, the others are
    judged like any product"""
    _check(nat, c)


@pytest.mark.parametrize("c", C.GRAM_CASES + C.GRAM_BOUNDARY, ids=C.case_id)
def test_gram_kernel_and_its_limits(nat, c):
    _check(nat, c)


@pytest.mark.parametrize("c", C.BROADCAST_CASES + C.SAME_TENSOR_CASES, ids=C.case_id)
def test_wrapper_equals_the_direct_call(nat, c):
    """_native.bgemm_f64 with a batch-1 operand (batch stride 0) and with one tensor as both operands (the pointer test
    of the Gram dispatch): bit for bit what the direct call gives"""
    regime = "graded"
    lay = C.layout(c)
    assert c.lda_pad == c.a_stride_pad == c.a_off == 0
    direct, (a, b) = _direct(nat, c, regime)
    ta = a[:lay.a_batch * lay.a_shape[0] * lay.lda].view(lay.a_batch, *lay.a_shape)
    tb = ta if c.same else b[:lay.b_batch * lay.b_shape[0] * lay.ldb].view(lay.b_batch, *lay.b_shape)
    mask = C.skip_mask(c)
    skip = None if mask is None else torch.from_numpy(mask).cuda()
    got = nat.bgemm_f64(ta, tb, trans_a=c.ta, trans_b=c.tb, out_dtype=C.TORCH_DTYPE[c.dtc], symmetric=c.sym, skip=skip)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (c.batch, c.M, c.N) and got.dtype == C.TORCH_DTYPE[c.dtc]
    live = [m for m in range(c.batch) if mask is None or not mask[m]]
    assert _same_bits(got.cpu()[live], direct[live])

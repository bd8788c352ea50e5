"""The small fused kernels at the two ends of a training step -- ce_rows_kernel + ce_uwso_finish_kernel
(csrc/ce_uwso.hip), angle_weights_kernel, selector_bwd_seed_kernel + symmetrise_store_kernel, flag_if_exceeds_kernel
(csrc/selector.hip), sf_adamw_kernel and lerp_kernel (csrc/optim.hip) -- per element against fp64 at the shapes where
their strided loops, grid caps and switches can go wrong (GPU box only).  tests/_head_cases.py holds the cases, the
inputs, the fp64 references and the derived bounds, and says which regime a case reaches (pinned by
tests/test_head_cases_cpu.py, which also holds an fp32 torch chain of every formula to half of the same bounds).

The C entries are called directly on caller-owned buffers that hold a known pattern before the launch, with 64 guard
elements behind each (on both sides of the optimizer's slices): the guards must come back bit for bit.  One test
function per kernel family and one per family's refusals, so that a family can be taken out alone."""
import ctypes

import pytest
import torch

from tests import _head_cases as H

pytestmark = pytest.mark.gpu

_WORST = {}          # (kernel, output) -> (largest err / bound, case): printed when the module is done (pytest -s)
BASD_OK, BASD_ERR_SHAPE = 0, 1
G = H.GUARD


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    for (kernel, name), (v, where) in sorted(_WORST.items()):
        print(f"head-worst {kernel} {name}: {v:.4f} at {where}")


@pytest.fixture(autouse=True)
def _clean_status_word(nat):
    """the device health word is sticky by design: start every test from a clean one"""
    nat.status_word("cuda").zero_()
    yield


def _note(kernel, got, where):
    for name, v in got.items():
        print(f"head-bound {where} {name} {v:.4f}")
        if v >= _WORST.get((kernel, name), (-1.0, None))[0]:
            _WORST[(kernel, name)] = (v, where)
    for name, v in got.items():
        assert v <= 1.0, (kernel, where, name, v)


def _healthy(nat):
    assert int(nat.status_word("cuda").item()) == 0


def _owned(n, dtype=torch.float32):
    """a caller-owned output of n elements and its G guard elements, all holding the known pattern; and a copy"""
    pre = H.guard_fill(n + G, dtype).cuda()
    return pre.clone(), pre


def _bits(t):
    return t.view(torch.int32)


def _cuda(t):
    return None if t is None else t.cuda()


def _last_error(nat) -> str:
    return nat.lib().basd_last_error().decode()


# ----------------------------------------------------------------------------------------------------------------------
# cross-entropy / UW-SO head
# ----------------------------------------------------------------------------------------------------------------------
def _ce_call(nat, logits, soft, labels, B, C, smoothing, geo, row, dl, out4):
    return nat.lib().basd_ce_uwso(nat._ptr(logits), nat._ptr(soft), nat._ptr(labels), B, C, smoothing, nat._ptr(geo),
                                  nat._ptr(row), nat._ptr(dl), nat._ptr(out4), nat._stream())


@pytest.mark.parametrize("case", H.CE_CASES, ids=H.ce_id)
def test_ce_uwso_against_fp64(nat, case):
    """row_loss, dlogits and the four scalars of basd_ce_uwso per element; two calls are bit-identical (no atomics)"""
    B, C = case.B, case.C
    logits, soft, labels, geo = (_cuda(t) for t in H.ce_inputs(case))
    ref = H.CERef(logits, soft, labels, case.smoothing, geo)
    geo1 = None if geo is None else geo.reshape(1)
    runs = []
    for _ in range(2):
        bufs = [_owned(n) for n in (B, B * C, 4)]
        rc = _ce_call(nat, logits, soft, labels, B, C, case.smoothing, geo1, *(b for b, _p in bufs))
        assert rc == BASD_OK, _last_error(nat)
        torch.cuda.synchronize()
        for (b, pre), n in zip(bufs, (B, B * C, 4)):
            assert torch.equal(_bits(b[n:]), _bits(pre[n:])), "written behind a buffer"
        runs.append([b[:n] for (b, _p), n in zip(bufs, (B, B * C, 4))])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), "two calls differ"
    row, dl, out4 = runs[0]
    _healthy(nat)
    _note("ce_uwso", ref.ratios(row, dl.view(B, C), out4), H.ce_id(case))


def test_ce_uwso_refusals(nat):
    """neither or both kinds of target, a missing output: an error before any launch; an empty batch: a no-op"""
    B, C = 3, 5
    logits, soft = torch.randn(B, C).cuda(), torch.rand(B, C).cuda()
    labels = torch.zeros(B, dtype=torch.int64).cuda()
    (row, prow), (dl, pdl), (out4, pout) = _owned(B), _owned(B * C), _owned(4)
    assert _ce_call(nat, logits, None, None, B, C, 0.1, None, row, dl, out4) == BASD_ERR_SHAPE
    assert "exactly one of soft_targets" in _last_error(nat)
    assert _ce_call(nat, logits, soft, labels, B, C, 0.1, None, row, dl, out4) == BASD_ERR_SHAPE
    for missing in range(3):
        outs = [row, dl, out4]
        outs[missing] = None
        assert _ce_call(nat, logits, soft, None, B, C, 0.1, None, *outs) == BASD_ERR_SHAPE
        assert "are required" in _last_error(nat)
    assert _ce_call(nat, logits, soft, None, 0, C, 0.1, None, row, dl, out4) == BASD_OK
    assert _ce_call(nat, logits, soft, None, B, 0, 0.1, None, row, dl, out4) == BASD_OK
    torch.cuda.synchronize()
    assert torch.equal(_bits(row), _bits(prow)) and torch.equal(_bits(dl), _bits(pdl)) and torch.equal(_bits(out4), _bits(pout))
    _healthy(nat)


# ----------------------------------------------------------------------------------------------------------------------
# angle weights, forward
# ----------------------------------------------------------------------------------------------------------------------
def _aw_call(nat, sig, sw, lt, E, L, D, unnorm, d2, pre, w, coef):
    return nat.lib().basd_angle_weights(nat._ptr(sig), nat._ptr(sw), nat._ptr(lt), E, L, D, int(unnorm), nat._ptr(d2),
                                        nat._ptr(pre), nat._ptr(w), nat._ptr(coef), nat._stream())


@pytest.mark.parametrize("case", H.AW_CASES, ids=H.aw_id)
def test_angle_weights_against_fp64(nat, case):
    """d2, pre, the softmax weights and coef of basd_angle_weights per element; coef is exactly 0 where the clamp or a
    floor is active; a rank-0 layer gives the NaN pattern of the fp64 reference"""
    E, L, D = case.E, case.L, case.D
    sig, sw, lt = (t.cuda() for t in H.aw_inputs(case))
    ref = H.AWRef(sig, sw, lt, case.unnorm)
    sizes = (E * L, E * L, E * L, E * L * D)
    bufs = [_owned(n) for n in sizes]
    rc = _aw_call(nat, sig, sw, lt, E, L, D, case.unnorm, *(b for b, _p in bufs))
    assert rc == BASD_OK, _last_error(nat)
    torch.cuda.synchronize()
    for (b, pre), n in zip(bufs, sizes):
        assert torch.equal(_bits(b[n:]), _bits(pre[n:])), "written behind a buffer"
    d2, pre, w, coef = (b[:n] for (b, _p), n in zip(bufs, sizes))
    _healthy(nat)
    _note("angle_weights", ref.ratios(d2.view(E, L), pre.view(E, L), w.view(E, L), coef.view(E, L, D),
                                      nan_ok=case.ranks == "rank0"), H.aw_id(case))


def test_angle_weights_refusals(nat):
    """more layers than the kernel's table, no directions: an error; no extraction points: a no-op that writes nothing"""
    sig, sw, lt = torch.rand(2 * 65 * 4).cuda(), torch.rand(65 * 4).cuda(), torch.zeros(2).cuda()
    bufs = [_owned(2 * 65 * 4) for _ in range(4)]
    outs = [b for b, _p in bufs]
    assert _aw_call(nat, sig, sw, lt, 2, H.AW_MAX_L + 1, 4, True, *outs) == BASD_ERR_SHAPE
    assert "angle_weights: L=65" in _last_error(nat)
    assert _aw_call(nat, sig, sw, lt, 2, 3, 0, True, *outs) == BASD_ERR_SHAPE
    assert "D=0" in _last_error(nat)
    assert _aw_call(nat, sig, sw, lt, 0, 3, 4, True, *outs) == BASD_OK
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(b), _bits(p)) for b, p in bufs)
    _healthy(nat)


# ----------------------------------------------------------------------------------------------------------------------
# angle weights, backward
# ----------------------------------------------------------------------------------------------------------------------
WS_FILL, WS_GUARD = 0xA5, 4096


def _workspace(nbytes):
    """(buffer, offset): buffer[offset : offset + nbytes] starts 8 bytes behind a 256-byte boundary, WS_GUARD bytes of
    the fill follow it"""
    raw = torch.full((256 + 8 + nbytes + WS_GUARD,), WS_FILL, dtype=torch.uint8, device="cuda")
    off = (8 - raw.data_ptr()) % 256
    assert (raw.data_ptr() + off) % 256 == 8
    return raw, off


def _ab_call(nat, inp, E, L, D, Ds, g_lt, w_tok, ws_ptr, ws_bytes):
    p = nat._ptr
    return nat.lib().basd_angle_weights_bwd(
        p(inp["g_w"]), p(inp["g_pre_out"]), p(inp["wts"]), p(inp["d2"]), p(inp["log_temp"]), p(inp["t_seed"]),
        p(inp["v_s"]), p(inp["lam_s"]), p(inp["proj_s"]), E, L, D, Ds, p(g_lt), p(w_tok), ctypes.c_void_p(ws_ptr),
        ctypes.c_int64(ws_bytes), nat._stream())


@pytest.mark.parametrize("case", H.AB_CASES, ids=H.ab_id)
def test_angle_weights_bwd_against_fp64(nat, case):
    """g_log_temp and w_tok of basd_angle_weights_bwd per element, on a workspace of exactly the stated size whose base
    is 8 bytes off a 256-byte boundary; w_tok is bitwise symmetric (h + h^T in fp64 commutes)"""
    E, L, D, Ds = case.E, case.L, case.D, case.Ds
    inp = {k: _cuda(v) for k, v in H.ab_inputs(case).items()}
    ref = H.ABRef(**inp)
    need = int(nat.lib().basd_angle_weights_bwd_workspace_bytes(E, D, Ds))
    assert need == H.ab_launch(E, L, D, Ds).ws_bytes
    raw, off = _workspace(need)
    (g_lt, plt), (w_tok, ptok) = _owned(E), _owned(E * Ds * Ds)
    rc = _ab_call(nat, inp, E, L, D, Ds, g_lt, w_tok, raw.data_ptr() + off, need)
    assert rc == BASD_OK, _last_error(nat)
    torch.cuda.synchronize()
    assert bool((raw[:off] == WS_FILL).all()) and bool((raw[off + need:] == WS_FILL).all()), "written outside the workspace"
    assert torch.equal(_bits(g_lt[E:]), _bits(plt[E:])) and torch.equal(_bits(w_tok[E * Ds * Ds:]), _bits(ptok[E * Ds * Ds:]))
    w = w_tok[:E * Ds * Ds].view(E, Ds, Ds)
    assert torch.equal(w, w.transpose(1, 2)), "w_tok is not bitwise symmetric"
    _healthy(nat)
    _note("angle_weights_bwd", ref.ratios(g_lt[:E], w), H.ab_id(case))


def test_angle_weights_bwd_refusals(nat):
    """a workspace one byte short, no workspace, more layers than the kernel's table: an error, nothing written"""
    case = H.ABCase(2, 3, 48, 16, True, (0.0, 0.5))
    E, L, D, Ds = case.E, case.L, case.D, case.Ds
    inp = {k: _cuda(v) for k, v in H.ab_inputs(case).items()}
    need = H.ab_workspace_bytes(E, D, Ds)
    raw, off = _workspace(need)
    (g_lt, plt), (w_tok, ptok) = _owned(E), _owned(E * Ds * Ds)
    assert _ab_call(nat, inp, E, L, D, Ds, g_lt, w_tok, raw.data_ptr() + off, need - 1) == BASD_ERR_SHAPE
    assert f"workspace of {need - 1} bytes, need {need}" in _last_error(nat)
    assert _ab_call(nat, inp, E, L, D, Ds, g_lt, w_tok, 0, need) == BASD_ERR_SHAPE
    assert "workspace" in _last_error(nat)
    assert _ab_call(nat, inp, E, H.AW_MAX_L + 1, D, Ds, g_lt, w_tok, raw.data_ptr() + off, need) == BASD_ERR_SHAPE
    assert "angle_weights_bwd: L=65" in _last_error(nat)
    torch.cuda.synchronize()
    assert bool((raw == WS_FILL).all()) and torch.equal(_bits(g_lt), _bits(plt)) and torch.equal(_bits(w_tok), _bits(ptok))
    _healthy(nat)


# ----------------------------------------------------------------------------------------------------------------------
# health-word flag
# ----------------------------------------------------------------------------------------------------------------------
def _flag_call(nat, values, n, tol, bit, status):
    return nat.lib().basd_flag_if_exceeds_f64(nat._ptr(values), ctypes.c_int64(n), tol, bit, nat._ptr(status), nat._stream())


@pytest.mark.parametrize("n", H.FLAG_SIZES)
def test_flag_if_exceeds_on_an_own_status_buffer(nat, n):
    """one offender (the next double above tol, NaN, +inf) at the first / last index and on both sides of the
    grid-stride wrap ORs exactly its bit into a word that holds 0x5A0; tol itself, -inf and -0.0 leave the word"""
    base = H.flag_clean(n).cuda()
    status = torch.full((1 + G,), H.STATUS_PRE, dtype=torch.int32, device="cuda")
    want = status.clone()
    assert _flag_call(nat, base, n, H.FLAG_TOL, 0x40, status) == BASD_OK
    assert torch.equal(status, want), "a value <= tol raised the flag"
    for kind, (value, bit) in H.FLAG_KINDS.items():
        for pos in H.flag_positions(n):
            v = base.clone()
            v[pos] = value
            status.fill_(H.STATUS_PRE)
            assert _flag_call(nat, v, n, H.FLAG_TOL, bit, status) == BASD_OK
            want[0] = H.STATUS_PRE | bit
            assert torch.equal(status, want), (kind, pos, hex(int(status[0])))
    _healthy(nat)                                       # the shared word was never the target


def test_flag_if_exceeds_noops_and_wrapper(nat):
    """n = 0 and a null status launch nothing; through the wrapper a NaN surfaces as the LinAlgError and clears"""
    bad = torch.tensor([0.5, float("nan"), 0.1], dtype=torch.float64, device="cuda")
    status = torch.full((1 + G,), H.STATUS_PRE, dtype=torch.int32, device="cuda")
    assert _flag_call(nat, bad, 0, 1.0, 2, status) == BASD_OK
    assert _flag_call(nat, bad, 3, 1.0, 2, None) == BASD_OK
    torch.cuda.synchronize()
    assert bool((status == H.STATUS_PRE).all())
    _healthy(nat)
    nat.flag_if_exceeds(bad, 1.0, nat.STATUS_NONFINITE)
    with pytest.raises(torch.linalg.LinAlgError, match="non-finite"):
        nat.check_status()
    nat.check_status()                                  # cleared by the failed check
    _healthy(nat)


# ----------------------------------------------------------------------------------------------------------------------
# Schedule-Free AdamW step and lerp
# ----------------------------------------------------------------------------------------------------------------------
def _sliced(t):
    """t [n] as the middle of a buffer with G guard elements on both sides: (buffer, its copy, the slice)"""
    n = t.numel()
    buf = H.guard_fill(n + 2 * G).cuda()
    buf[G:G + n] = t.cuda()
    return buf, buf.clone(), buf[G:G + n]


def _guards_intact(buf, pre, n):
    return torch.equal(_bits(buf[:G]), _bits(pre[:G])) and torch.equal(_bits(buf[G + n:]), _bits(pre[G + n:]))


@pytest.mark.parametrize("case", H.AD_CASES, ids=H.ad_id)
def test_sf_adamw_step_against_fp64(nat, case):
    """y, z and v of basd_sf_adamw_step per element (v carries a per-index signature: an element skipped or updated
    twice is off by a thousand bounds), g and the guards on both sides of every slice bit for bit"""
    n = case.n
    ins = H.ad_inputs(case)
    (by, py, y), (bg, pg, g), (bz, pz, z), (bv, pv, v) = (_sliced(t) for t in ins)
    ref = H.ADRef(y, g, z, v, case)
    assert y.data_ptr() % 16 == 0
    nat.sf_adamw_step(y, g, z, v, **H.ad_kwargs(case))
    torch.cuda.synchronize()
    assert all(_guards_intact(b, p, n) for b, p in ((by, py), (bg, pg), (bz, pz), (bv, pv))), "written outside a slice"
    assert torch.equal(_bits(bg), _bits(pg)), "the gradient was written"
    _healthy(nat)
    _note("sf_adamw", ref.ratios(y, z, v), H.ad_id(case))


def test_sf_adamw_step_refuses_misaligned_buffers(nat):
    n = 1027
    bufs = [_sliced(t) for t in H.ad_inputs(H.ADCase(n + 1, 0.25, 0.3, 0.05))]
    f = ctypes.c_double
    for bad in range(4):
        ptrs = [nat._ptr(s[1:] if i == bad else s[:n]) for i, (_b, _p, s) in enumerate(bufs)]
        assert ptrs[bad].value % 16 == 4
        rc = nat.lib().basd_sf_adamw_step(*ptrs, ctypes.c_int64(n), f(3e-3), f(0.9), f(0.999), f(1e-8), f(0.05), f(0.25),
                                          f(0.3), nat._stream())
        assert rc == BASD_ERR_SHAPE and "16-byte aligned" in _last_error(nat)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(b), _bits(p)) for b, p, _s in bufs)
    _healthy(nat)


@pytest.mark.parametrize("case", H.LP_CASES, ids=H.lp_id)
def test_lerp_against_fp64(nat, case):
    """y of basd_lerp per element; w = 0 leaves y bit for bit; z and the guards untouched"""
    n = case.n
    (by, py, y), (bz, pz, z) = (_sliced(t) for t in H.lp_inputs(case))
    ref = H.LPRef(y, z, case.w)
    nat.lerp_(y, z, case.w)
    torch.cuda.synchronize()
    assert _guards_intact(by, py, n) and torch.equal(_bits(bz), _bits(pz)), "written outside y"
    if case.w == 0.0:
        assert torch.equal(_bits(by), _bits(py))
    _healthy(nat)
    _note("lerp", ref.ratios(y), H.lp_id(case))

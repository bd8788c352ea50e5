"""The bf16 attention kernels at the logit statistics of a trained ViT (tests/_attn_regimes.py: attention sinks at the CLS
token, in a late key tile and in two tiles, one-hot rows, all-equal rows, logits of std 14), each C entry called
directly, against fp64 on the same bf16 inputs.  The bounds are the ones the project's tests already use; the
backward's dQ / dK are compared as tests/_attn_regimes.py::BWD_CHECKS says, and the CPU module checks that table."""
import ctypes

import pytest
import torch

from tests import _attn_regimes as R
from tests.test_attention_long_gpu import _long_bwd, _long_fwd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


@pytest.fixture(autouse=True)
def _clean_status_word(nat):
    nat.status_word("cuda").zero_()
    yield


def _short_fwd(nat, qkv, H, hd, scale, cls=False, lse=False):
    B, T = qkv.shape[0], qkv.shape[1]
    out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
    c = torch.empty(B, H, T - 1, dtype=torch.float32, device="cuda") if cls else None
    l = torch.empty(B, H, T, dtype=torch.float32, device="cuda") if lse else None
    nat._check(nat.lib().basd_attention_fwd_bf16(nat._ptr(qkv), B, T, H, hd, ctypes.c_float(scale), nat._ptr(out),
                                                 nat._ptr(c), nat._ptr(l), nat._stream()), "fwd")
    return out, (c.sum(1) if cls else None), l


def _short_qmean(nat, qkv, H, hd, scale):
    B, T = qkv.shape[0], qkv.shape[1]
    out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
    m = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    nat._check(nat.lib().basd_attention_fwd_qmean_bf16(nat._ptr(qkv), B, T, H, hd, ctypes.c_float(scale),
                                                       nat._ptr(out), nat._ptr(m), nat._stream()), "fwd_qmean")
    return out, m.sum(1)


def _short_bwd(nat, qkv, out, dout, lse, H, hd, scale):
    B, T = qkv.shape[0], qkv.shape[1]
    dqkv = torch.empty_like(qkv)
    nat._check(nat.lib().basd_attention_bwd_bf16(nat._ptr(qkv), nat._ptr(out), nat._ptr(dout), nat._ptr(lse), B, T, H,
                                                 hd, ctypes.c_float(scale), nat._ptr(dqkv), nat._stream()), "bwd")
    return dqkv


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t.float()).all())


def _inputs(B, T, H, hd, regime):
    seed = R.seed_of(B, T, H, hd, regime)
    return R.sink_qkv(B, T, H, hd, regime=regime, seed=seed).cuda(), R.dout_for(B, T, H, hd, seed).cuda()


def _check_cls_tap(tap, qkv, H, hd, scale):
    """the CLS-row contract (bf16-rounded logits) on every key a kernel cannot round either way"""
    ref, exact, amb, _, _, _ = R.cls_ref(qkv, H, hd, scale)
    assert tap.shape == ref.shape and tap.dtype == torch.float32
    _finite(tap)
    assert float(amb.double().mean()) <= R.AMBIGUOUS_SHARE
    ok = ~amb
    t = tap.double()
    print(f"  CLS tap: worst |err| on unambiguous keys {float((t - ref)[ok].abs().max()):.2e}")
    assert torch.allclose(t[ok], ref[ok], rtol=2e-2, atol=1e-6)
    assert float((t - exact).abs().max()) <= 1.5 * float((ref - exact).abs().max()) + 1e-6


def _check_fwd(nat, family, B, T, H, hd, regime):
    qkv, _ = _inputs(B, T, H, hd, regime)
    scale = hd ** -0.5
    if family == "short":
        out, cls, lse = _short_fwd(nat, qkv, H, hd, scale, cls=True, lse=True)
        plain, _, _ = _short_fwd(nat, qkv, H, hd, scale)
        out_q, qm = _short_qmean(nat, qkv, H, hd, scale)
    else:
        out, lse, cls, qm = _long_fwd(nat, qkv, H, hd, scale, cls=True, qmean=True)
        plain, _, _, _ = _long_fwd(nat, qkv, H, hd, scale, lse=False)
        out_q = out
    logits, p, ref, ref_lse = R.fwd_ref(qkv, H, hd, scale)
    _finite(out, plain, out_q, lse, qm)
    err = float((out.double() - ref).abs().max())
    bound = 2e-2 * float(ref.abs().max()) + 1e-3
    lse_err = (lse.double() - ref_lse).abs()
    lse_use = float((lse_err / R.lse_bound(logits)).max())
    qm_ref = p.mean(dim=(1, 2))
    qm_use = float(((qm.double() - qm_ref).abs() / (1e-8 + 2e-5 * qm_ref.abs())).max())
    print(f"{family} {regime} T={T} hd={hd}: out {err / bound:.3f} of bound, LSE {lse_use:.3f} of bound "
          f"(worst {float(lse_err.max()):.2e}), query mean {qm_use:.3f} of tolerance")
    assert err < bound
    assert torch.equal(out, plain) and torch.equal(out, out_q)     # the taps do not change the output
    assert lse_use <= 1.0
    assert qm.shape == (B, T)
    assert torch.allclose(qm.double(), qm_ref, rtol=2e-5, atol=1e-8)
    assert torch.allclose(qm.sum(-1), torch.ones(B, device="cuda"), atol=1e-5)
    _check_cls_tap(cls, qkv, H, hd, scale)
    nat.check_status()


@pytest.mark.parametrize("regime", R.SHORT_REGIMES)
@pytest.mark.parametrize("B,T,H,hd", R.SHORT_FWD)
def test_short_forward_in_regime(nat, B, T, H, hd, regime):
    """basd_attention_fwd_bf16 (plain; LSE + CLS tap) and basd_attention_fwd_qmean_bf16"""
    _check_fwd(nat, "short", B, T, H, hd, regime)


@pytest.mark.parametrize("regime", R.LONG_REGIMES)
@pytest.mark.parametrize("B,T,H,hd", R.LONG_FWD)
def test_long_forward_in_regime(nat, B, T, H, hd, regime):
    """basd_attention_fwd_long_bf16: plain, and LSE + CLS tap + query-mean tap"""
    _check_fwd(nat, "long", B, T, H, hd, regime)


@pytest.mark.parametrize("regime", R.SHORT_REGIMES)
@pytest.mark.parametrize("B,T,H,hd", R.CLS_IMPORTANCE)
def test_cls_importance_in_regime(nat, B, T, H, hd, regime):
    """basd_cls_importance_bf16 (T <= 320) and the long CLS-row kernel (T > 320, basd_attention_fwd_long_bf16 without
    an output), the entries nat.cls_importance dispatches to"""
    qkv, _ = _inputs(B, T, H, hd, regime)
    scale = hd ** -0.5
    if T <= 320:
        imp = torch.empty(B, T - 1, dtype=torch.float32, device="cuda")
        nat._check(nat.lib().basd_cls_importance_bf16(nat._ptr(qkv), B, T, H, hd, ctypes.c_float(scale), nat._ptr(imp),
                                                       nat._stream()), "cls_importance")
    else:
        c = torch.empty(B, H, T - 1, dtype=torch.float32, device="cuda")
        nat._check(nat.lib().basd_attention_fwd_long_bf16(nat._ptr(qkv), B, T, H, hd, ctypes.c_float(scale),
                                                          nat._ptr(None), nat._ptr(c), nat._ptr(None), nat._ptr(None),
                                                          nat._stream()), "fwd_long cls")
        imp = c.sum(1)
    print(f"cls_importance {regime} T={T} hd={hd}")
    _check_cls_tap(imp, qkv, H, hd, scale)
    nat.check_status()


def _check_bwd(nat, family, B, T, H, hd, regime):
    qkv, dout = _inputs(B, T, H, hd, regime)
    scale = hd ** -0.5
    if family == "short":
        out, _, lse = _short_fwd(nat, qkv, H, hd, scale, lse=True)
        dqkv = _short_bwd(nat, qkv, out, dout, lse, H, hd, scale)
        cap = R.CAP_SHORT
    else:
        out, lse, _, _ = _long_fwd(nat, qkv, H, hd, scale)
        dqkv = _long_bwd(nat, qkv, out, dout, lse, H, hd, scale)
        dqkv2 = _long_bwd(nat, qkv, out, dout, lse, H, hd, scale)
        assert torch.equal(dqkv, dqkv2)                 # dQ partials added in key-block order: bitwise reproducible
        cap = R.CAP_LONG
    _finite(out, lse, dqkv)
    gq, gk, gv = R.dqkv_parts(dqkv, H, hd)
    aq, ak, av, mq, mk = R.bwd_a_ref(qkv, out, dout, H, hd, scale)     # given the kernel's own bf16 O
    xq, xk, xv = R.bwd_autograd(qkv, dout, H, hd, scale)
    checks = R.BWD_CHECKS[regime]
    figs = {"dV vs autograd": R.rel(gv, xv), "dV vs (a)": R.rel(gv, av),
            "dQ (a) / magnitude": R.rel(gq, aq, mq), "dK (a) / magnitude": R.rel(gk, ak, mk)}
    if family in checks["a_result"]:
        figs.update({"dQ (a) / result": R.rel(gq, aq), "dK (a) / result": R.rel(gk, ak)})
    if family in checks["b"]:
        figs.update({"dQ vs autograd": R.rel(gq, xq), "dK vs autograd": R.rel(gk, xk)})
    print(f"{family} bwd {regime} T={T} hd={hd}: " + ", ".join(f"{n} {e:.2e}" for n, e in figs.items()))
    for name, e in figs.items():
        assert e < cap, (name, e)
    nat.check_status()


@pytest.mark.parametrize("regime", R.SHORT_REGIMES)
@pytest.mark.parametrize("B,T,H,hd", R.SHORT_BWD)
def test_short_backward_in_regime(nat, B, T, H, hd, regime):
    """basd_attention_bwd_bf16 on the output and LSE of basd_attention_fwd_bf16"""
    _check_bwd(nat, "short", B, T, H, hd, regime)


@pytest.mark.parametrize("regime", R.LONG_REGIMES)
@pytest.mark.parametrize("B,T,H,hd", R.LONG_BWD)
def test_long_backward_in_regime(nat, B, T, H, hd, regime):
    """basd_attention_bwd_long_bf16 on the output and LSE of basd_attention_fwd_long_bf16"""
    _check_bwd(nat, "long", B, T, H, hd, regime)

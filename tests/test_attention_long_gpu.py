"""Long-sequence attention kernels (csrc/attention_long.hip) against an fp64 restatement on the same bf16 inputs, the
overlap with the short kernels at T = 197, and the dispatch of ``_native`` (short kernels wherever they apply)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# LSE: about 3x the worst |error| over seeds 0-2 of the forward cases below (measured on the MI355X: 1.06e-6, T = 1024)
LSE_ATOL = 3.2e-6
# dqkv rel-L2 per Q / K / V slice vs fp64 autograd: about 3x the worst over seeds 0-2 (measured 2.41e-3, dV, T 577 hd 80)
BWD_REL = 7.5e-3


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    native.lib()
    return native


def _qkv(B, T, H, hd, seed, amp=1.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, 3 * H * hd, generator=g) * amp).to(torch.bfloat16).cuda()


def _long_fwd(nat, qkv, H, hd, scale, cls=False, qmean=False, lse=True):
    B, T = qkv.shape[0], qkv.shape[1]
    out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
    l = torch.empty(B, H, T, dtype=torch.float32, device="cuda") if (lse or qmean) else None
    c = torch.empty(B, H, T - 1, dtype=torch.float32, device="cuda") if cls else None
    m = torch.empty(B, H, T, dtype=torch.float32, device="cuda") if qmean else None
    nat._check(nat.lib().basd_attention_fwd_long_bf16(nat._ptr(qkv), B, T, H, hd, ctypes.c_float(scale), nat._ptr(out),
                                                      nat._ptr(c), nat._ptr(m), nat._ptr(l), nat._stream()), "fwd_long")
    return out, l, (c.sum(1) if cls else None), (m.sum(1) if qmean else None)


def _long_bwd(nat, qkv, out, dout, lse, H, hd, scale):
    B, T = qkv.shape[0], qkv.shape[1]
    ws = torch.empty(int(nat.lib().basd_attention_bwd_long_workspace_bytes(B, T, H, hd)), dtype=torch.uint8,
                     device="cuda")
    dqkv = torch.empty_like(qkv)
    nat._check(nat.lib().basd_attention_bwd_long_bf16(nat._ptr(qkv), nat._ptr(out), nat._ptr(dout), nat._ptr(lse), B, T,
                                                      H, hd, ctypes.c_float(scale), nat._ptr(dqkv), nat._ptr(ws),
                                                      ctypes.c_int64(ws.numel()), nat._stream()), "bwd_long")
    return dqkv


def _ref(qkv, H, hd, scale):
    B, T = qkv.shape[0], qkv.shape[1]
    x = qkv.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).double()
    q, k, v = x[0], x[1], x[2]
    logits = (q @ k.transpose(-1, -2)) * scale
    p = logits.softmax(dim=-1)
    return q, k, p, (p @ v).transpose(1, 2).reshape(B, T, H * hd), torch.logsumexp(logits, dim=-1)


FWD = [(2, 1, 3, 64), (2, 225, 3, 64), (3, 257, 3, 64), (2, 257, 12, 80), (2, 300, 2, 64), (2, 300, 3, 80),
       (2, 577, 12, 64), (1, 577, 2, 80), (1, 1024, 3, 64), (1, 1024, 2, 80), (2, 197, 2, 80)]


def errors_fwd(nat, B, T, H, hd, seed):
    """-> (out error / bound, worst |LSE error|, CLS tap, query-mean tap results) of one forward case"""
    qkv = _qkv(B, T, H, hd, seed * 7919 + T * 7 + H + hd)
    scale = hd ** -0.5
    out, lse, cls, qm = _long_fwd(nat, qkv, H, hd, scale, cls=T >= 2, qmean=True)
    q, k, p, ref, ref_lse = _ref(qkv, H, hd, scale)
    err = float((out.double() - ref).abs().max())
    bound = 2e-2 * float(ref.abs().max()) + 1e-3
    return qkv, (out, lse, cls, qm), (q, k, p, ref, ref_lse), err / bound, float((lse.double() - ref_lse).abs().max())


@pytest.mark.parametrize("B,T,H,hd", FWD)
def test_long_forward_output_lse_and_taps(nat, B, T, H, hd):
    qkv, (out, lse, cls, qm), (q, k, p, ref, ref_lse), rel, lse_err = errors_fwd(nat, B, T, H, hd, 0)
    assert out.shape == (B, T, H * hd) and out.dtype == torch.bfloat16
    assert rel < 1.0, rel                                # max error < 2e-2 max|ref| + 1e-3
    assert lse_err < LSE_ATOL, lse_err
    scale = hd ** -0.5
    if T >= 2:
        logits = (q[:, :, :1] @ k.transpose(-2, -1)).float()
        want = (logits.to(torch.bfloat16).float() * scale).softmax(dim=-1)[:, :, 0, 1:].mean(dim=1)
        assert cls.shape == (B, T - 1)
        assert torch.allclose(cls, want, rtol=2e-2, atol=1e-6)
    want = p.mean(dim=(1, 2))
    assert qm.shape == (B, T) and qm.dtype == torch.float32
    assert torch.allclose(qm.double(), want, rtol=2e-5, atol=1e-8)
    assert torch.allclose(qm.sum(-1), torch.ones(B, device="cuda"), atol=1e-5)
    # the taps do not change the output; the query-mean tap is bitwise reproducible
    out2, _, _, qm2 = _long_fwd(nat, qkv, H, hd, scale, qmean=True)
    assert torch.equal(out, out2) and torch.equal(qm, qm2)


def errors_bwd(nat, B, T, H, hd, seed):
    """-> ({slice: rel-L2 vs fp64 autograd}, first dqkv, second dqkv) of one backward case"""
    g = torch.Generator().manual_seed(seed * 104729 + B * 1000 + T + hd)
    qkv = (torch.randn(B, T, 3 * H * hd, generator=g) * 0.8).bfloat16().cuda()
    dout = torch.randn(B, T, H * hd, generator=g).bfloat16().cuda()
    scale = hd ** -0.5
    out, lse, _, _ = _long_fwd(nat, qkv, H, hd, scale)
    dqkv = _long_bwd(nat, qkv, out, dout, lse, H, hd, scale)
    dqkv2 = _long_bwd(nat, qkv, out, dout, lse, H, hd, scale)
    x = qkv.double().reshape(B, T, 3, H, hd).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = (((q @ k.transpose(-1, -2)) * scale).softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, H * hd)
    o.backward(dout.double())
    ref = x.grad.reshape(B, T, 3, H * hd)
    got = dqkv.double().reshape(B, T, 3, H * hd)
    rel = {}
    for i, name in enumerate("qkv"):
        den = float(ref[:, :, i].norm())
        # T = 1: dQ and dK vanish (one key); what is left is the fp32 rounding of dP - delta, measured absolutely
        rel[name] = float((got[:, :, i] - ref[:, :, i]).norm()) / (den if den > 0 else 1.0)
    return rel, dqkv, dqkv2


BWD = [(2, 225, 3, 64), (2, 257, 3, 64), (2, 257, 2, 80), (1, 577, 3, 64), (1, 577, 2, 80), (2, 197, 2, 80),
       (1, 1024, 2, 64), (2, 1, 2, 80)]


@pytest.mark.parametrize("B,T,H,hd", BWD)
def test_long_backward_matches_fp64_autograd(nat, B, T, H, hd):
    rel, dqkv, dqkv2 = errors_bwd(nat, B, T, H, hd, 0)
    print(f"T={T} hd={hd}: rel-L2 {rel}")
    for name, e in rel.items():
        assert e < BWD_REL, (name, e)
    # dQ partials are added in key-block order (no atomics): bitwise reproducible
    assert torch.equal(dqkv, dqkv2)


def test_long_entries_agree_with_the_short_kernels_at_t197(nat):
    """T = 197, hd 64: both kernel families apply; same contracts up to the bf16 rounding of P"""
    B, T, H, hd = 4, 197, 3, 64
    scale = hd ** -0.5
    qkv = _qkv(B, T, H, hd, 11, amp=0.8)
    out_s, imp_s, lse_s = nat.attention_fwd(qkv, H, hd, scale, want_importance=True, want_lse=True)
    out_l, lse_l, cls_l, _ = _long_fwd(nat, qkv, H, hd, scale, cls=True)
    assert float((out_s.float() - out_l.float()).abs().max()) < 1e-2 * float(out_s.float().abs().max())
    assert torch.allclose(lse_s, lse_l, rtol=0, atol=1e-5)
    assert torch.allclose(cls_l, imp_s, rtol=2e-2, atol=1e-6)
    # same arithmetic as basd_cls_importance_bf16 (fp32 dot in d order, bf16 rounding), sums in another order
    assert torch.allclose(cls_l, nat.cls_importance(qkv, H, hd, scale), rtol=1e-5, atol=1e-8)
    _, imp_q = nat.attention_fwd(qkv, H, hd, scale, want_importance=True, query_mean=True)
    _, _, _, qm_l = _long_fwd(nat, qkv, H, hd, scale, qmean=True)
    assert torch.allclose(qm_l, imp_q, rtol=1e-4, atol=1e-8)
    dout = torch.randn(B, T, H * hd, device="cuda").bfloat16()
    d_s = nat.attention_bwd(qkv, out_s, dout, lse_s, H, hd, scale)
    d_l = _long_bwd(nat, qkv, out_s, dout, lse_s, H, hd, scale)
    a, b = d_s.float().reshape(B, T, 3, -1), d_l.float().reshape(B, T, 3, -1)
    for i in range(3):
        assert float((a[:, :, i] - b[:, :, i]).norm() / a[:, :, i].norm()) < 5e-3, "qkv"[i]


class _Spy:
    def __init__(self, monkeypatch, lib, names):
        self.calls = []
        for name in names:
            fn = getattr(lib, name)

            def spy(*args, _fn=fn, _name=name):
                self.calls.append(_name)
                return _fn(*args)
            monkeypatch.setattr(lib, name, spy)


def test_dispatch_keeps_the_short_kernels(nat, monkeypatch):
    """c1 to c5 shapes stay on the short entries; only shapes they refuse reach the long ones"""
    names = ("basd_attention_fwd_bf16", "basd_attention_fwd_qmean_bf16", "basd_attention_bwd_bf16",
             "basd_cls_importance_bf16", "basd_attention_fwd_long_bf16", "basd_attention_bwd_long_bf16")
    spy = _Spy(monkeypatch, nat.lib(), names)

    def run(T, H, hd, **kw):
        spy.calls.clear()
        qkv = _qkv(2, T, H, hd, T + hd, amp=0.8)
        res = nat.attention_fwd(qkv, H, hd, hd ** -0.5, **kw)
        return qkv, res, list(spy.calls)

    assert run(197, 3, 64, want_importance=True)[2] == ["basd_attention_fwd_bf16"]
    assert run(197, 3, 64, want_importance=True, query_mean=True)[2] == ["basd_attention_fwd_qmean_bf16"]
    assert run(257, 2, 80, want_importance=True)[2] == ["basd_attention_fwd_bf16"]
    assert run(272, 2, 64, want_lse=True)[2] == ["basd_attention_fwd_bf16"]
    assert run(273, 2, 64, want_lse=True)[2] == ["basd_attention_fwd_long_bf16"]
    assert run(577, 2, 80, want_importance=True, query_mean=True)[2] == ["basd_attention_fwd_long_bf16"]
    for T, hd, want in [(197, 64, "basd_attention_bwd_bf16"), (224, 64, "basd_attention_bwd_bf16"),
                        (225, 64, "basd_attention_bwd_long_bf16"), (197, 80, "basd_attention_bwd_long_bf16")]:
        qkv, (out, _, lse), _ = run(T, 2, hd, want_lse=True)
        spy.calls.clear()
        nat.attention_bwd(qkv, out, torch.randn_like(out), lse, 2, hd, hd ** -0.5)
        assert spy.calls == [want], (T, hd, spy.calls)
    for T, want in [(320, "basd_cls_importance_bf16"), (321, "basd_attention_fwd_long_bf16")]:
        qkv = _qkv(2, T, 2, 64, T)
        spy.calls.clear()
        imp = nat.cls_importance(qkv, 2, 64, 0.125)
        assert spy.calls == [want] and imp.shape == (2, T - 1)
        tot = imp.sum(-1)                                  # the CLS row without its first key
        assert bool(((tot > 0) & (tot <= 1 + 1e-5)).all())

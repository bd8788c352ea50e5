"""The attention-regime inputs of tests/test_attention_regimes_gpu.py, checked without a GPU on the same seeds: every
regime is what it claims (on its fp64 reference), the CLS-tap reference has few keys that a kernel could round either
way, and every backward comparison the GPU test makes leaves the kernel room under its cap -- the reference floor of
the end-to-end comparison (b), and an emulation of the kernel's fp32 dP - delta and bf16 dS for (a)."""
import pytest
import torch

from tests import _attn_regimes as R


def _cases(shapes, regimes):
    return [(*s, r) for s in shapes for r in regimes]


REGIME_CASES = sorted(set(_cases(R.SHORT_FWD + R.SHORT_BWD, R.SHORT_REGIMES) +
                          _cases(R.LONG_FWD + R.LONG_BWD, R.LONG_REGIMES) +
                          _cases(R.CLS_IMPORTANCE, R.SHORT_REGIMES)))
CLS_CASES = sorted(set(_cases(R.SHORT_FWD, R.SHORT_REGIMES) + _cases(R.LONG_FWD, R.LONG_REGIMES) +
                       _cases(R.CLS_IMPORTANCE, R.SHORT_REGIMES)))
BWD_CASES = [(*c, "short") for c in _cases(R.SHORT_BWD, R.SHORT_REGIMES)] + \
            [(*c, "long") for c in _cases(R.LONG_BWD, R.LONG_REGIMES)]


@pytest.mark.parametrize("B,T,H,hd,regime", REGIME_CASES)
def test_regime_is_what_it_claims(B, T, H, hd, regime):
    qkv = R.sink_qkv(B, T, H, hd, regime=regime, seed=R.seed_of(B, T, H, hd, regime))
    assert qkv.shape == (B, T, 3 * H * hd) and qkv.dtype == torch.bfloat16
    logits, p, _, _ = R.fwd_ref(qkv, H, hd, hd ** -0.5)
    kind, s = R.REGIMES[regime]
    pmax = p.amax(dim=-1)
    arg = p.argmax(dim=-1)
    rng = logits.amax(dim=-1) - logits.amin(dim=-1)
    print(f"{regime} T={T} hd={hd}: mean max P {float(pmax.mean()):.4f}, logit std {float(logits.std()):.2f}, "
          f"max range {float(rng.max()):.1f}")
    if kind == "gauss":
        assert float(pmax.mean()) < 0.1 and float(rng.max()) < 20
    elif kind == "flat":
        assert bool((logits[:, 0::2] == 0).all()) and bool((p[:, 0::2] == 1.0 / T).all())
        assert float(logits[:, 1::2].abs().max()) > 0                 # the odd heads are Gaussian
    elif kind == "hot":
        assert 10 <= float(logits.std()) <= 16 and float(rng.min()) >= 40
    else:
        sinks = R.sink_positions(kind, T)
        if kind == "cls":
            assert bool((arg == 0).all())
            if s >= 30:
                assert float(pmax.mean()) >= 0.999
            else:
                # the rest of the row grows with T: the mean row maximum of P is about 0.85 on the 224-px grids
                # (T <= 257) and falls to about 0.5 at T = 1024
                assert float(pmax.mean()) >= (0.8 if T <= 257 else 0.45)
        elif kind in ("late_last", "late_tile"):
            j = sinks[0]
            assert j >= R.KB and bool((arg == j).all())
            # the row maximum appears only in the tile of the sink, tens of logits above the earlier tiles: the long
            # forward's rescale factor exp(m_run - m_new) is at most e^-15 < 2^-21 there (about e^-25 on average)
            t0 = R.KB * (j // R.KB)
            gap = logits[..., j] - logits[..., :t0].amax(dim=-1)
            assert float(gap.min()) >= 15 and float(pmax.mean()) >= 0.999
        else:
            j1, j2 = sinks
            assert j1 // R.KB != j2 // R.KB
            pair = p[..., j1] + p[..., j2]
            assert float(pair.mean()) >= 0.99
            # both sinks carry mass: the second tile's maximum is within a few logits of the first's
            assert float(torch.minimum(p[..., j1], p[..., j2]).mean()) >= 0.01


@pytest.mark.parametrize("B,T,H,hd,regime", CLS_CASES)
def test_cls_tap_reference_is_unambiguous(B, T, H, hd, regime):
    """few keys whose bf16 logit a kernel may round the other way, and none of them able to move the other keys"""
    qkv = R.sink_qkv(B, T, H, hd, regime=regime, seed=R.seed_of(B, T, H, hd, regime))
    ref, exact, amb, amb_logit, p_r, ulp = R.cls_ref(qkv, H, hd, hd ** -0.5)
    share = float(amb.double().mean())
    # one ulp at an ambiguous logit moves every probability of its row by about P * ulp: at most 1/20 of the 2e-2
    # tolerance of the other keys
    influence = float((p_r * ulp * amb_logit).max())
    print(f"{regime} T={T} hd={hd}: ambiguous share {share:.4f}, influence {influence:.2e}")
    assert share <= R.AMBIGUOUS_SHARE
    assert influence <= 1e-3


@pytest.mark.parametrize("B,T,H,hd,regime,family", BWD_CASES)
def test_backward_references_leave_room(B, T, H, hd, regime, family):
    """the table R.BWD_CHECKS holds for this case: what the GPU test asserts leaves the kernel room under its cap"""
    cap = R.CAP_SHORT if family == "short" else R.CAP_LONG
    seed = R.seed_of(B, T, H, hd, regime)
    qkv = R.sink_qkv(B, T, H, hd, regime=regime, seed=seed)
    dout = R.dout_for(B, T, H, hd, seed)
    scale = hd ** -0.5
    _, _, o, _ = R.fwd_ref(qkv, H, hd, scale)
    o_b = o.to(torch.bfloat16)                                # the rounding of O that no kernel avoids
    dq, dk, dv, mq, mk = R.bwd_a_ref(qkv, o_b, dout, H, hd, scale)
    # emulation of the kernels: fp32 dP - delta, bf16 dS (the exact fp64 values rounded)
    q, k, v = R.split(qkv, H, hd)
    p = ((q @ k.transpose(-1, -2)) * scale).softmax(dim=-1)
    og = o_b.double().reshape(B, T, H, hd).transpose(1, 2)
    do = dout.double().reshape(B, T, H, hd).transpose(1, 2)
    d32 = ((do @ v.transpose(-1, -2)).float() - (do * og).sum(-1, keepdim=True).float()).double()
    ds = (scale * p * d32).to(torch.bfloat16).double()
    eq, ek = ds @ k, ds.transpose(-1, -2) @ q
    checks = R.BWD_CHECKS[regime]
    figs = {"q/mag": R.rel(eq, dq, mq), "k/mag": R.rel(ek, dk, mk)}
    if family in checks["a_result"]:
        figs.update({"q/res": R.rel(eq, dq), "k/res": R.rel(ek, dk)})
    if family in checks["b"]:
        aq, ak, av = R.bwd_autograd(qkv, dout, H, hd, scale)
        figs.update({"floor q": R.rel(dq, aq), "floor k": R.rel(dk, ak), "floor v": R.rel(dv, av)})
    print(f"{regime} T={T} hd={hd}: " + ", ".join(f"{n} {e:.2e}" for n, e in figs.items()))
    for name, e in figs.items():
        assert e <= (cap / 2 if name.startswith("floor") else cap / 4), (name, e)

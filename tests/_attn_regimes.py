"""Attention inputs with the logit statistics of a trained ViT (attention sinks, one-hot rows, tens of logits), the fp64
references the regime tests compare the bf16 attention kernels with, and the table of which backward comparisons each
regime supports.  Shared by tests/test_attention_regimes_cpu.py (the inputs really are what they claim; the references
leave the kernels room under the caps) and tests/test_attention_regimes_gpu.py (the kernels against the references).

Construction (all in fp64, rounded to bf16 once): qkv ~ N(0, 0.8^2).  A sink of strength s adds a * u to every query
and to the key of one token, u a unit vector per head, a = sqrt(s) * hd^(1/4): every query's scaled logit against that
key rises by about a^2 * scale = s."""
import math

import torch

BASE_STD = 0.8
HOT_VAR = 14.0                     # `hot`: q, k ~ N(0, 14) -> scale * q.k has std 14 (any hd)
SINK_LATE = 30.0                   # strength of the late and the paired sinks
KB = 64                            # keys per tile of the long forward (csrc/attention_long.hip)

# regime -> (kind, strength)
REGIMES = {
    "gauss": ("gauss", 0.0),
    "flat": ("flat", 0.0),             # q = 0 in the even heads: all logits 0, exact ties, P = 1 / T
    "cls_sink8": ("cls", 8.0),
    "cls_sink30": ("cls", 30.0),
    "cls_sink80": ("cls", 80.0),
    "late_last": ("late_last", SINK_LATE),   # the last token (inside a ragged last tile when T % 64 != 0)
    "late_tile": ("late_tile", SINK_LATE),   # the last key of the last full 64-key tile before the final tile
    "two_sinks": ("two", SINK_LATE),         # token 1 and the last token: different 64-key tiles, equal strength
    "hot": ("hot", 0.0),
}

# The short kernels see the whole row at once: late_tile adds nothing to late_last there.
SHORT_REGIMES = [r for r in REGIMES if r != "late_tile"]
LONG_REGIMES = list(REGIMES)

# Shapes (B, T, H, hd), B * H <= 8
SHORT_FWD = [(2, 197, 2, 64), (2, 257, 2, 80), (2, 272, 2, 64)]
SHORT_BWD = [(2, 65, 2, 64), (2, 97, 2, 64), (2, 197, 2, 64), (2, 224, 2, 64)]
LONG_FWD = [(2, 273, 2, 64), (2, 273, 2, 80), (1, 577, 2, 64), (1, 577, 2, 80), (1, 1024, 2, 64), (1, 1024, 2, 80)]
LONG_BWD = LONG_FWD + [(2, 197, 2, 80)]
# basd_cls_importance_bf16 (T <= 320) and the long CLS-row kernel (T > 320) on both sides of the switch
CLS_IMPORTANCE = [(2, 197, 2, 64), (2, 320, 2, 64), (2, 321, 2, 64), (1, 577, 2, 80)]

# rel-L2 caps the project already has: short backward (test_kernels_gpu.py::test_attention_bwd_matches_autograd) and
# long backward (test_attention_long_gpu.py::BWD_REL)
CAP_SHORT = 1.5e-2
CAP_LONG = 7.5e-3

# Backward comparisons per regime and kernel family ("short": basd_attention_bwd_bf16, cap CAP_SHORT; "long":
# basd_attention_bwd_long_bf16, cap CAP_LONG).  dV is compared in every regime (vs fp64 autograd and vs the reference
# of (a)), and so are dQ / dK by
#   (a) the entry's own contract (fp64 FA2 backward given the kernel's bf16 O), error over the magnitude of the
#       computation ||scale (P o (|dP| + |delta|)) |K|||.
# The table lists the families that also get
#   "a_result": the error of (a) over the result's norm: only where dS is not a cancellation residue (a one-hot row's
#       dS is O(2^-24 hd) of its terms, so its error relative to the result has no bound) and where the emulation of
#       the kernels' fp32 dP - delta / bf16 dS stays under a quarter of the cap.  s = 8 measures 1.4e-3 .. 2.2e-3: under
#       a quarter of the short cap, not of the long one (moved off for "long");
#   "b": dQ / dK end to end against fp64 autograd: only where the reference floor (the rounding of O to bf16 that no
#       kernel avoids) is at most half the cap.  Not at s >= 8 (floor 7e-3 .. 1); `hot` (logit std 14, top
#       probability about 0.85) has a floor of 4.5e-3 .. 6.0e-3: under half the short cap, not the long one.
BWD_CHECKS = {
    "gauss": {"a_result": ("short", "long"), "b": ("short", "long")},
    "flat": {"a_result": ("short", "long"), "b": ("short", "long")},
    "cls_sink8": {"a_result": ("short",), "b": ()},
    "cls_sink30": {"a_result": (), "b": ()},
    "cls_sink80": {"a_result": (), "b": ()},
    "late_last": {"a_result": (), "b": ()},
    "late_tile": {"a_result": (), "b": ()},
    "two_sinks": {"a_result": (), "b": ()},
    "hot": {"a_result": ("short", "long"), "b": ("short",)},
}

# LSE: the existing absolute bound (test_attention_long_gpu.py::LSE_ATOL, measured at |LSE| <~ 7) plus 16 fp32 ulps of
# the row's largest |logit| (fp32 accumulation of exact bf16 products over hd <= 80 terms, and the fmaf)
LSE_ATOL = 3.2e-6
LSE_LOGIT_ULPS = 2.0 ** -20
# CLS tap: a logit within a relative 2^-20 of a bf16 rounding midpoint may round either way in the kernel's fp32 sum
AMBIGUOUS_REL = 2.0 ** -20
AMBIGUOUS_SHARE = 0.01


def seed_of(B, T, H, hd, regime, salt=0):
    return (((B * 1009 + T) * 131 + H) * 97 + hd) * 31 + list(REGIMES).index(regime) + 7919 * salt


def sink_positions(kind, T):
    if kind == "cls":
        return [0]
    if kind == "late_last":
        return [T - 1]
    if kind == "late_tile":
        return [KB * ((T - 1) // KB) - 1]
    if kind == "two":
        return [1, T - 1]
    return []


def sink_qkv(B, T, H, hd, *, regime, seed):
    """-> bf16 qkv [B, T, 3 * H * hd] (CPU) of the named regime"""
    kind, s = REGIMES[regime]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 3, H, hd, generator=g, dtype=torch.float64) * BASE_STD
    u = torch.randn(H, hd, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    if kind == "flat":
        x[:, :, 0, 0::2] = 0.0
    elif kind == "hot":
        x[:, :, :2] *= math.sqrt(HOT_VAR) / BASE_STD
    elif s > 0:
        a = math.sqrt(s) * hd ** 0.25
        x[:, :, 0] += a * u
        for j in sink_positions(kind, T):
            assert 0 <= j < T
            x[:, j, 1] += a * u
    return x.reshape(B, T, 3 * H * hd).to(torch.bfloat16)


def dout_for(B, T, H, hd, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randn(B, T, H * hd, generator=g).to(torch.bfloat16)


def split(qkv, H, hd):
    """bf16 qkv [B, T, 3 H hd] -> fp64 q, k, v [B, H, T, hd] (same device)"""
    B, T = qkv.shape[0], qkv.shape[1]
    x = qkv.double().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def fwd_ref(qkv, H, hd, scale):
    """-> (scaled logits [B, H, T, T], P, out [B, T, H hd], LSE [B, H, T]) in fp64"""
    B, T = qkv.shape[0], qkv.shape[1]
    q, k, v = split(qkv, H, hd)
    logits = (q @ k.transpose(-1, -2)) * scale
    p = logits.softmax(dim=-1)
    return logits, p, (p @ v).transpose(1, 2).reshape(B, T, H * hd), torch.logsumexp(logits, dim=-1)


def lse_bound(logits):
    return LSE_ATOL + LSE_LOGIT_ULPS * logits.abs().amax(dim=-1)


def near_bf16_midpoint(x):
    """True where x (fp64) lies within a relative AMBIGUOUS_REL of a midpoint between two bf16 neighbours"""
    _, e = torch.frexp(x)                                      # |x| = m 2^e, m in [0.5, 1): bf16 spacing 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    t = x.abs() / ulp
    dist = (t - t.floor() - 0.5).abs() * ulp
    return dist <= AMBIGUOUS_REL * x.abs()


def cls_ref(qkv, H, hd, scale):
    """The CLS-row tap's contract: softmax over bf16(q_0 . k_t) * scale, head-averaged, without key 0.
    -> (ref [B, T-1], exact [B, T-1] (no rounding), ambiguous keys [B, T-1], ambiguous logits [B, H, T], P of the
    rounded row [B, H, T], one bf16 ulp of every scaled logit [B, H, T])"""
    q, k, _ = split(qkv, H, hd)
    raw = (q[:, :, :1] @ k.transpose(-1, -2))[:, :, 0]         # [B, H, T], exact (bf16 products, fp64 sum)
    rounded = raw.to(torch.bfloat16).double()
    p_r = (rounded * scale).softmax(dim=-1)
    ref = p_r[:, :, 1:].mean(dim=1)
    exact = (raw * scale).softmax(dim=-1)[:, :, 1:].mean(dim=1)
    amb_logit = near_bf16_midpoint(raw)
    _, e = torch.frexp(raw)
    ulp = torch.ldexp(torch.ones_like(raw), e - 8) * scale
    return ref, exact, amb_logit.any(dim=1)[:, 1:], amb_logit, p_r, ulp


def bwd_a_ref(qkv, o_given, dout, H, hd, scale):
    """fp64 FA2 backward of the entry's contract, given the (kernel's) bf16 O and dO:
    -> (dq, dk, dv, magnitude of dq, magnitude of dk), each [B, H, T, hd]"""
    B, T = qkv.shape[0], qkv.shape[1]
    q, k, v = split(qkv, H, hd)
    p = ((q @ k.transpose(-1, -2)) * scale).softmax(dim=-1)
    og = o_given.double().reshape(B, T, H, hd).transpose(1, 2)
    do = dout.double().reshape(B, T, H, hd).transpose(1, 2)
    delta = (do * og).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - delta)
    w = scale * p * (dp.abs() + delta.abs())
    return (scale * ds @ k, scale * ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do,
            w @ k.abs(), w.transpose(-1, -2) @ q.abs())


def bwd_autograd(qkv, dout, H, hd, scale):
    """fp64 autograd of softmax(Q K^T scale) V -> dq, dk, dv [B, H, T, hd]"""
    B, T = qkv.shape[0], qkv.shape[1]
    x = qkv.double().reshape(B, T, 3, H, hd).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = (((q @ k.transpose(-1, -2)) * scale).softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, H * hd)
    o.backward(dout.double())
    return tuple(x.grad[:, :, i].transpose(1, 2) for i in range(3))


def dqkv_parts(dqkv, H, hd):
    """kernel dqkv [B, T, 3 H hd] -> fp64 dq, dk, dv [B, H, T, hd]"""
    B, T = dqkv.shape[0], dqkv.shape[1]
    x = dqkv.double().reshape(B, T, 3, H, hd)
    return tuple(x[:, :, i].transpose(1, 2) for i in range(3))


def rel(a, b, den=None):
    return float((a - b).norm() / (b if den is None else den).norm())

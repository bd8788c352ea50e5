"""Cases, launcher mirrors, inputs, fp64 references and bounds of tests/test_head_kernels_gpu.py: the small fused kernels
at the two ends of a training step -- the cross-entropy / UW-SO head (csrc/ce_uwso.hip), the selector's angle weights
and their backward and the health-word flag (csrc/selector.hip), the flat Schedule-Free AdamW step and the lerp
(csrc/optim.hip).  No GPU is used here.

Per family: namedtuple cases with a readable id; seeded CPU generators of fp32 inputs (the CPU pin and the GPU test see
the same bits); a plain-Python mirror of the HOST launch arithmetic (grid, trips of every strided loop, tails), so that
a case can say which regime it reaches (pinned by tests/test_head_cases_cpu.py); an fp64 reference written from the
formula in the kernel's header comment, on the fp32 input values; a per-element bound built from that reference's own
intermediate magnitudes (results are err / bound, asserted <= 1 on the GPU); and, where tests/_emul.py has none, an
fp32 torch chain of the same formula, which tests/test_head_cases_cpu.py holds to err / bound <= 0.5.

The leading constants K_* were set on the CPU, never on a kernel: the worst err / bound of the fp32 chain over all
cases of the family at K = 1 is noted next to each, and K is the next "round" number that puts it at or below 0.5 (a
factor two for the kernels' other summation order and their fused multiply-adds).
"""
from __future__ import annotations

import collections
import math

import torch

U = 2.0 ** -24             # unit roundoff of fp32
V = 2.0 ** -53             # of fp64
TINY = 2.0 ** -126         # smallest normal fp32: what a flushed or denormal result can be off by, whatever its size
EPS32 = 2.0 ** -23         # torch.finfo(float32).eps, the clamp of the reference code
GUARD = 64                 # elements behind (optimizer: on both sides of) every caller-owned buffer
STATUS_PRE = 0x5A0         # what a test-owned status buffer holds before a flag launch

# launch constants, once, with their source lines
CE_LANES = 256             # ce_uwso.hip:36 ff., :64 (``c += 256``, ``b += 256``)
CE_SCALE_UNROLL = 256 * 8  # ce_uwso.hip:99 (elements per workgroup the scaling grid is sized for)
CE_SCALE_CAP = 1024        # ce_uwso.hip:100
AW_LANES = 256             # selector.hip:39, :42, :122 (``m += 256``, ``a += 256``), :132, :180 (symmetrise blocks)
AW_MAX_L = 64              # selector.hip:30, :80, :101, :151
FLAG_CAP = 256             # selector.hip:201 (workgroups of 256 lanes)
OPT_LANES = 256            # optim.hip:129, :142
OPT_CAP = 2048             # optim.hip:130, :143


def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b


def f32(x: float) -> float:
    """x rounded to fp32, as a Python double: what a float argument or a (float) cast of the C entry holds"""
    return float(torch.tensor(x, dtype=torch.float64).float())


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1_000_003 + int(k) + 29) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, nan_ok: bool = False) -> float:
    """max |got - ref| / bound in fp64; an exact element passes a zero bound; a NaN fails, unless ``nan_ok``: then the
    NaN pattern of ``got`` must equal that of ``ref`` and those positions are left out"""
    got, ref = got.double().reshape(-1), ref.reshape(-1)
    bound = bound.reshape(-1)
    if nan_ok:
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), "NaN pattern differs from the fp64 reference"
        keep = ~torch.isnan(ref)
        got, ref, bound = got[keep], ref[keep], bound[keep]
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    assert not bool(torch.isnan(q).any()), "NaN in an output"
    return float(q.max()) if q.numel() else 0.0


def guard_fill(n: int, dtype=torch.float32) -> torch.Tensor:
    """a known pattern no kernel result equals: what outputs and their guards hold before a launch"""
    return (-777.0 - (torch.arange(n) % 13).double()).to(dtype)


# ======================================================================================================================
# cross-entropy / UW-SO head (csrc/ce_uwso.hip)
# ======================================================================================================================
# target: hard | soft | sums (soft rows that sum to 1, 0.5, 2 and an exact one-hot given as soft)
# geo: None | float;  margin: 0 | 30 | 100 (one class ``margin`` above all others);  right: the confident class is the
# label on EVERY row (with smoothing 0 and margin 100 the cross-entropy itself is below eps)
CECase = collections.namedtuple("CECase", "B C target smoothing geo margin right")


def _ce(B, C, target="hard", smoothing=0.1, geo=3.7, margin=0, right=False):
    return CECase(B, C, target, smoothing, geo, margin, right)


def ce_id(c: CECase) -> str:
    s = f"{c.B}x{c.C}-{c.target}-s{c.smoothing}-geo{c.geo}"
    return s + (f"-margin{c.margin}" if c.margin else "") + ("-right" if c.right else "")


CE_CLASSES = [1, 2, 63, 255, 256, 257, 1000]
CE_BATCHES = [1, 255, 256, 257, 600]
CE_GEO = [None, 3.7, 1e6, 1e-9, 0.0]
CE_CAP_CASES = [_ce(2048, 1024, "soft"), _ce(2049, 1024, "hard")]
CE_CLAMP_CASE = _ce(64, 100, "hard", 0.0, 3.7, 100, True)
CE_CASES = ([_ce(5, C, t, s) for C in CE_CLASSES for t, s in (("hard", 0.1), ("soft", 0.0))]
            + [_ce(B, 10, t, s) for B in CE_BATCHES for t, s in (("hard", 0.0), ("soft", 0.1))]
            + CE_CAP_CASES
            + [_ce(4, 37, "sums", s) for s in (0.0, 0.1)] + [_ce(8, 300, "sums", 0.1)]
            + [_ce(64, C, t, 0.1, 3.7, m) for m in (30, 100) for C in (100, 1000) for t in ("hard", "soft")]
            + [_ce(64, 100, "hard", 0.0, 3.7, 100)]
            + [_ce(7, 10, t, 0.1, geo) for geo in CE_GEO for t in ("hard", "soft")]
            + [CE_CLAMP_CASE, CE_CLAMP_CASE._replace(geo=1e-9), CE_CLAMP_CASE._replace(geo=None)])

CELaunch = collections.namedtuple("CELaunch", "class_trips idle_lanes row_trips grid scale_trips last_trip cap")


def ce_launch(B: int, C: int) -> CELaunch:
    """basd_ce_uwso: ce_rows_kernel on B workgroups (class loops of ceil(C / 256) trips; ``idle_lanes`` have no class at
    all), ce_uwso_finish_kernel on min(ceil(B C / 2048), 1024) workgroups: the row_loss sum takes ceil(B / 256) trips,
    the scaling loop ceil(B C / (256 grid)) (8 where the grid is not capped), its last one ``last_trip`` elements"""
    n = B * C
    grid = min(_ceil(n, CE_SCALE_UNROLL), CE_SCALE_CAP)
    per = grid * CE_LANES
    limit = CE_SCALE_CAP * CE_SCALE_UNROLL
    return CELaunch(_ceil(C, CE_LANES), max(0, CE_LANES - C), _ceil(B, CE_LANES), grid, _ceil(n, per),
                    n - (_ceil(n, per) - 1) * per, "below" if n < limit else "at" if n == limit else "above")


def ce_inputs(case: CECase):
    """(logits [B, C] fp32, soft [B, C] fp32 | None, labels [B] int64 | None, geo 0-d fp32 | None).  Hard labels: row 0
    has label 0, row 1 label C - 1.  margin: one class per row ``margin`` above all others (the target on even rows,
    another class on odd rows unless ``right``), and row 0 all equal (the construction of test_ce_uwso_matches_torch)"""
    B, C = case.B, case.C
    g = _gen(B, C, ("hard", "soft", "sums").index(case.target), int(case.smoothing * 100), case.margin)
    logits = torch.randn(B, C, generator=g) * 3
    soft = labels = None
    if case.target == "hard":
        labels = torch.randint(C, (B,), generator=g)
        labels[0] = 0
        if B > 1:
            labels[1] = C - 1
        top = labels.clone()
    else:
        t = torch.rand(B, C, generator=g) + 1e-3
        soft = t / t.sum(-1, keepdim=True)
        if case.target == "sums":
            soft = soft * torch.tensor([1.0, 0.5, 2.0, 1.0]).repeat(_ceil(B, 4))[:B].view(B, 1)
            soft[3] = 0.0
            soft[3, C // 3] = 1.0
        top = soft.argmax(-1)
    if case.margin:
        if not case.right and C > 1:
            other = (top + torch.randint(1, C, (B,), generator=g)) % C
            top[1::2] = other[1::2]
        rows = torch.arange(B)
        logits[rows, top] = -float("inf")
        logits[rows, top] = logits.amax(-1) + case.margin
        if not case.right:
            logits[0] = 7.25
    geo = None if case.geo is None else torch.tensor(case.geo, dtype=torch.float32)
    return logits.float().contiguous(), None if soft is None else soft.float().contiguous(), labels, geo


def _targets64(B, C, soft, labels):
    if soft is not None:
        return soft.double()
    return torch.nn.functional.one_hot(labels, C).double()


# The bounds (u = 2^-24).  Per element of row b, with zl = z - lse, p = exp(zl), tsum = sum_c t':
#   dlogits  scale (K u ((1 + |zl|) p tsum + |t'|)) + |dlogits| (rel. error of scale) + 2^-126.  (1 + |zl|) u is the
#            argument error of an fp32 exp2(x log2 e): x log2 e is rounded at size |x| log2 e, which moves the result
#            by |x| u relative; |t'| u the roundings of t' and of the subtraction.  The classes whose probability
#            underflows (margin 100) are computed as 0 or as a denormal: 2^-126 covers either, whatever scale is.
#   row_loss K u sum_c t' (|z_c| + |lse|): each term t' (z_c - lse) is formed from an fp32 lse (u |lse|) and an fp32
#            difference (u (|z_c| + |lse|)), and the terms are summed in fp32.
#   out4     ce = mean(row_loss): the mean of the row bounds plus the fp32 sum of B terms (B / 256 per lane, 8 tree
#            steps, the division).  With cc = max(ce, eps), gg = max(geo, eps): w_ce = gg / (cc + gg), so
#            |d w_ce| = |d w_geo| = w_ce d_ce / (cc + gg) (the clamp has slope <= 1), each plus K u of itself for the two
#            reciprocals, the sum and the division; total = w_ce ce + w_geo geo by the product rule plus K u of its terms.
K_CE_DL = 8.0        # CPU worst at K = 1: 2.41 (2049x1024-hard-s0.1); at K = 6: 0.501 (7x10-soft-geoNone), at 8: 0.38
K_CE_ROW = 12.0      # CPU worst at K = 1: 5.82 (2049x1024-hard-s0.1: label smoothing puts |z_c| + |lse| of all 1024 classes in the sum)
K_CE_OUT = 2.0       # CPU worst at K = 1 (all three constants): 0.72 (64x1000-soft-margin100)


class CERef:
    def __init__(self, logits, soft, labels, smoothing: float, geo):
        z = logits.double()
        B, C = z.shape
        s = f32(smoothing)
        tp = (1.0 - s) * _targets64(B, C, soft, labels) + s / C
        lse = torch.logsumexp(z, -1, keepdim=True)
        zl = z - lse
        p = zl.exp()
        tsum = tp.sum(-1, keepdim=True)
        self.row = -(tp * zl).sum(-1)
        ce = self.row.mean()
        self.row_b = K_CE_ROW * U * (tp * (z.abs() + lse.abs())).sum(-1)
        d_ce = self.row_b.mean() + (_ceil(B, CE_LANES) + 9) * U * self.row.abs().mean()
        zero = torch.zeros((), dtype=torch.float64, device=z.device)
        if geo is None:
            g, w_ce, w_geo, d_w, self.clamped = zero, zero + 1.0, zero, zero, (False, False)
            d_wce = d_wgeo = zero
        else:
            g = geo.double().reshape(())
            cc, gg = ce.clamp_min(EPS32), g.clamp_min(EPS32)
            self.clamped = (bool(ce < EPS32), bool(g < EPS32))
            ic, ig = 1.0 / cc, 1.0 / gg
            w_ce, w_geo = ic / (ic + ig), ig / (ic + ig)
            d_w = w_ce * d_ce / (cc + gg)
            d_wce, d_wgeo = d_w + K_CE_OUT * U * w_ce, d_w + K_CE_OUT * U * w_geo
        total = w_ce * ce + w_geo * g
        d_total = d_wce * ce.abs() + w_ce * d_ce + d_wgeo * g.abs() + K_CE_OUT * U * ((w_ce * ce).abs() + (w_geo * g).abs())
        self.out4 = torch.stack([total, ce, w_ce, w_geo])
        self.out4_b = torch.stack([d_total, d_ce, d_wce, d_wgeo])
        scale = w_ce / B
        self.dl = (p * tsum - tp) * scale
        self.dl_b = (scale * K_CE_DL * U * ((1.0 + zl.abs()) * p * tsum + tp.abs())
                     + self.dl.abs() * (d_wce / w_ce + 2.0 * U) + TINY)

    def ratios(self, row, dl, out4) -> dict:
        return {"row_loss": ratio(row, self.row, self.row_b), "dlogits": ratio(dl, self.dl, self.dl_b),
                "out4": ratio(out4, self.out4, self.out4_b)}


def ce_chain32(logits, soft, labels, smoothing: float, geo):
    """the same formula as an fp32 torch chain, the exponential as exp2(x log2 e): -> (row_loss, dlogits, out4)"""
    z = logits.float()
    B, C = z.shape
    one = torch.ones((), dtype=torch.float32)
    log2e = one * 1.4426950408889634
    s = one * smoothing
    t = soft.float() if soft is not None else torch.nn.functional.one_hot(labels, C).float()
    tp = (one - s) * t + s / C
    mx = z.amax(-1, keepdim=True)
    lse = mx + torch.exp2((z - mx) * log2e).sum(-1, keepdim=True).log()
    row = -(tp * (z - lse)).sum(-1)
    dl = torch.exp2((z - lse) * log2e) * tp.sum(-1, keepdim=True) - tp
    ce = row.sum() / B
    w_ce, w_geo, g = one, one * 0, one * 0
    if geo is not None:
        g = geo.float().reshape(())
        ic, ig = one / ce.clamp_min(EPS32), one / g.clamp_min(EPS32)
        w_ce, w_geo = ic / (ic + ig), ig / (ic + ig)
    return row, dl * (w_ce / B), torch.stack([w_ce * ce + w_geo * g, ce, w_ce, w_geo])


# ======================================================================================================================
# angle weights, forward (csrc/selector.hip, angle_weights_kernel)
# ======================================================================================================================
# lt: None (linspace(-0.5, 0.8, E)) or a tuple of E values;  sig: random | edges (the special cosines in columns 0 ..);
# ranks: mixed (per-layer rank mask, layer 0 has rank 1) | rank0 (layer 1 all zero)
AWCase = collections.namedtuple("AWCase", "E L D unnorm lt sig ranks")


def _aw(E, L, D, unnorm, lt=None, sig="random", ranks="mixed"):
    return AWCase(E, L, D, unnorm, lt, sig, ranks)


def aw_id(c: AWCase) -> str:
    s = f"E{c.E}-L{c.L}-D{c.D}-{'unnorm' if c.unnorm else 'norm'}-{c.sig}"
    return s + ("-lt" + "_".join(str(v) for v in c.lt) if c.lt else "") + ("" if c.ranks == "mixed" else "-" + c.ranks)


AW_WIDTHS = [1, 63, 64, 255, 256, 257, 513]
AW_LAYERS = [1, 2, 63, 64]
AW_LT = (-8.0, 0.0, 19.5, 20.0, 20.5, 30.0)
# at 19.5 and above softplus(x) IS x in fp32 (e^-19.5 = 3e-9 < u x): a threshold moved below 20 shows only further
# down, where e^-x is still above fp32's rounding of x
AW_LT_MID = (10.5, 12.0, 15.0)
AW_FLOOR_U, AW_FLOOR_N = f32(1e-9), f32(1e-12)


def _next_up(x: float) -> float:
    t = torch.tensor(x, dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(2.0, dtype=torch.float32)))


# the special cosines: exactly 1 - eps (kept), the next float above (clamped), 1, two that cancel in 1 - s^2, both
# floors and the floats just above them, 0
AW_EDGES = [1.0 - EPS32, _next_up(1.0 - EPS32), 1.0, f32(0.9999), f32(0.999999), AW_FLOOR_U, _next_up(AW_FLOOR_U),
            AW_FLOOR_N, _next_up(AW_FLOOR_N), 0.0]
AW_CASES = ([_aw(2, 3, D, un, sig="edges" if D >= 63 else "random") for D in AW_WIDTHS for un in (True, False)]
            + [_aw(E, L, 40, un) for L in AW_LAYERS for E, un in ((1, True), (3, False))]
            + [_aw(6, 5, 70, un, AW_LT, "edges") for un in (True, False)]
            + [_aw(3, 5, 70, True, AW_LT_MID, "edges")]
            + [_aw(2, 3, 70, un, None, "edges", "rank0") for un in (True, False)])

AWLaunch = collections.namedtuple("AWLaunch", "trips idle_lanes last_trip")


def aw_launch(L: int, D: int) -> AWLaunch:
    """angle_weights_kernel: one workgroup per extraction point, the D directions of a layer in ceil(D / 256) trips"""
    assert 1 <= L <= AW_MAX_L and D >= 1
    trips = _ceil(D, AW_LANES)
    return AWLaunch(trips, max(0, AW_LANES - D), D - (trips - 1) * AW_LANES)


def aw_inputs(case: AWCase):
    """(sigma [E, L, D], sw [L, D], log_temp [E]) fp32"""
    E, L, D = case.E, case.L, case.D
    g = _gen(E, L, D, int(case.unnorm), 3)
    sig = torch.rand(E, L, D, generator=g).sort(dim=-1, descending=True).values
    if case.sig == "edges":
        sig[:, :, :len(AW_EDGES)] = torch.tensor(AW_EDGES, dtype=torch.float64).float()
    sw = torch.rand(L, D, generator=g).sort(dim=-1, descending=True).values + 0.1
    ranks = torch.randint(1, D + 1, (L,), generator=g)
    ranks[0] = 1
    if L > 1:
        ranks[1] = D
    if case.ranks == "rank0":
        ranks[1] = 0
    sw = sw * (torch.arange(D).unsqueeze(0) < ranks.unsqueeze(1))
    lt = torch.linspace(-0.5, 0.8, E) if case.lt is None else torch.tensor(case.lt)
    return sig.float().contiguous(), sw.float().contiguous(), lt.float()


def softplus64(lt: torch.Tensor) -> torch.Tensor:
    """softplus with torch's threshold, as the kernels' header states it"""
    return torch.where(lt > 20.0, lt, torch.log1p(torch.exp(lt.clamp(max=20.0))))


# The bounds.  coef = sw 2 theta (-1 / sqrt(1 - s^2)) / den / s^(1 | 3): 1 - s^2 is formed from an fp32 s^2 (u s^2
# absolute, s^2 / (1 - s^2) u relative to it): relative K u (1 + s^2 / (1 - s^2)), the conditioning of 1 / sqrt(1 - s^2)
# in fp32 (sc = min(s, 1 - eps) in place of s); the numerator sw theta / den may underflow before the guarded division
# by s^3 >= floor^3 blows it up again: + 2^-126 / s^(1 | 3).  Where the reference is exactly 0 (clamped, at or below the
# floor) so must the kernel be.  d2 = sum_m sw theta^2 / den, all terms >= 0: K u d2 + the fp32 sums (D / 256 per lane,
# 8 tree steps) (D / 256 + 8) u d2.  pre = -d2 / tau: d2's bound / tau + K u |pre| (softplus, division).  w = softmax:
# d w_j = w_j (d pre_j + sum_l w_l d pre_l) + (K + L) u w_j (L sequential additions) + 2^-126 (weights that underflow).
K_AW_COEF = 12.0     # CPU worst at K = 1: 5.50 (E3-L64-D40-norm-random)
K_AW_D2 = 2.0        # CPU worst at K = 1 (with the sum term): 0.47 (E3-L64-D40-norm-random)
K_AW_PRE = 2.0       # CPU worst at K = 1: 0.41
K_AW_W = 2.0         # CPU worst at K = 1: 0.29 (lt 10.5 / 12 / 15)


class AWRef:
    def __init__(self, sigma, sw, log_temp, unnorm: bool):
        s, w64, lt = sigma.double(), sw.double(), log_temp.double()
        E, L, D = s.shape
        one_m = 1.0 - EPS32
        sc = s.clamp(max=one_m)
        th = torch.acos(sc)
        den = w64.sum(-1)
        self.d2 = (w64.unsqueeze(0) * th * th).sum(-1) / den.unsqueeze(0)
        self.tau = softplus64(lt)
        self.pre = -self.d2 / self.tau.unsqueeze(1)
        self.w = torch.softmax(self.pre, dim=1)
        floor = AW_FLOOR_U if unnorm else AW_FLOOR_N
        self.ok = (s <= one_m) & (s > floor)
        one_m_s2 = 1.0 - sc * sc
        gs = w64.unsqueeze(0) * 2.0 * th * (-1.0 / torch.sqrt(one_m_s2)) / den.view(1, L, 1)
        div = torch.where(self.ok, s, torch.ones_like(s)) ** (3 if unnorm else 1)
        self.coef = torch.where(self.ok, gs / div, torch.zeros_like(gs))
        self.coef_b = torch.where(self.ok, K_AW_COEF * U * (1.0 + sc * sc / one_m_s2) * self.coef.abs() + TINY / div,
                                  torch.zeros_like(gs))
        self.d2_b = (K_AW_D2 + _ceil(D, AW_LANES) + 8) * U * self.d2
        self.pre_b = self.d2_b / self.tau.unsqueeze(1) + K_AW_PRE * U * self.pre.abs()
        self.w_b = (self.w * (self.pre_b + (self.w * self.pre_b).sum(1, keepdim=True)) + (K_AW_W + L) * U * self.w + TINY)

    def ratios(self, d2, pre, w, coef, nan_ok: bool = False) -> dict:
        return {"d2": ratio(d2, self.d2, self.d2_b, nan_ok), "pre": ratio(pre, self.pre, self.pre_b, nan_ok),
                "w": ratio(w, self.w, self.w_b, nan_ok), "coef": ratio(coef, self.coef, self.coef_b, nan_ok)}


# ======================================================================================================================
# angle weights, backward (csrc/selector.hip, basd_angle_weights_bwd)
# ======================================================================================================================
ABCase = collections.namedtuple("ABCase", "E L D Ds gpo lt")


def ab_id(c: ABCase) -> str:
    return f"E{c.E}-L{c.L}-D{c.D}-Ds{c.Ds}-{'gpo' if c.gpo else 'nogpo'}-lt" + "_".join(str(v) for v in c.lt)


AB_WIDTHS = [1, 48, 255, 256, 257, 320]
AB_DS = [1, 16, 17, 80]
AB_CASES = ([ABCase(2, 3, D, 24, D % 2 == 0, (0.3, 20.5)) for D in AB_WIDTHS]
            + [ABCase(2, 3, 48, Ds, Ds % 2 == 1, (-0.5, 0.8)) for Ds in AB_DS]
            + [ABCase(2, L, 32, 24, L == 1, (19.5, 25.0)) for L in (1, 64)])

ABLaunch = collections.namedtuple("ABLaunch", "seed_grid seed_trips idle_lanes sym_blocks sym_last ws_bytes")


def ab_workspace_bytes(E: int, D: int, Ds: int) -> int:
    """basd_angle_weights_bwd_workspace_bytes: K, K V, V^T K V [E, D, D], G P [E, D, D_s], P^T G P [E, D_s, D_s] in
    fp64, and 1024 bytes for the entry to align the first of them to 256"""
    return E * (3 * D * D + D * Ds + Ds * Ds) * 8 + 1024


def ab_launch(E: int, L: int, D: int, Ds: int) -> ABLaunch:
    """selector_bwd_seed_kernel on (E, D) workgroups, the D columns of a row of K in ceil(D / 256) trips;
    symmetrise_store_kernel on (ceil(D_s^2 / 256), E) workgroups, the last block ``sym_last`` elements"""
    assert 1 <= L <= AW_MAX_L and D >= 1 and Ds >= 1
    blocks = _ceil(Ds * Ds, AW_LANES)
    return ABLaunch((E, D), _ceil(D, AW_LANES), max(0, AW_LANES - D), blocks, Ds * Ds - (blocks - 1) * AW_LANES,
                    ab_workspace_bytes(E, D, Ds))


def ab_ties(D: int):
    """pairs of equal eigenvalues: the first two, the last two, and the pair across the 256-column trip boundary"""
    if D < 4:
        return []
    return [(0, 1), (D - 2, D - 1)] + ([(255, 256)] if D > 258 else [])


AB_MIN_GAP = 1e-3


def ab_inputs(case: ABCase) -> dict:
    E, L, D, Ds = case.E, case.L, case.D, case.Ds
    g = _gen(E, L, D, Ds, 5)
    lam = (AB_MIN_GAP + 0.01 * torch.rand(E, D, generator=g, dtype=torch.float64)).cumsum(1).flip(1).contiguous()
    for a, b in ab_ties(D):
        lam[:, b] = lam[:, a]              # raises lam_b: its gap to the next eigenvalue only grows
    return dict(
        g_w=torch.randn(E, L, generator=g), g_pre_out=torch.randn(E, L, generator=g) if case.gpo else None,
        wts=torch.softmax(torch.randn(E, L, generator=g), dim=1), d2=torch.rand(E, L, generator=g),
        log_temp=torch.tensor(case.lt).float(), t_seed=torch.randn(E, L, D, D, generator=g),
        v_s=torch.linalg.qr(torch.randn(E, D, D, generator=g, dtype=torch.float64))[0].float().contiguous(),
        lam_s=lam, proj_s=torch.randn(D, Ds, generator=g))


# The bounds.  g_pre = w (g_w - <w, g_w>) (+ g_pre_out) in fp32: the dot is L sequential additions (L u S,
# S = sum_l |w_l g_w_l|), the difference and the products round at the size of their operands:
#   d g_pre_j = K u (w_j (|g_w_j| + L S) + |g_pre_out_j|),   d g_d2_j = (d g_pre_j + K u |g_pre_j|) / tau.
# C = sum_j g_d2_j T_j is summed in fp64 from fp32 products: d C = sum_j (K u |g_d2_j| + d g_d2_j) |T_j|, d K = d C / |gap|
# (0 where the gap is 0: K is 0 there by definition).  The four fp64 products carry it on:
#   d W = |P|^T (|V|^T d K |V| + transpose) |P| + u |W| (the fp32 store) + 8 D v |P|^T (|V|^T |K| |V| + transpose) |P|.
# g_lt = sigmoid(lt) sum_j g_pre_j d2_j / tau^2: sigmoid / tau^2 sum_j (d g_pre_j |d2_j| + (K + L) u |g_pre_j d2_j|).
K_AB_W = 1.0         # CPU worst at K = 1: 0.004 (the fp32 part is g_d2 alone; L S is a worst case no input reaches)
K_AB_LT = 2.0        # CPU worst at K = 1: 0.42


class ABRef:
    def __init__(self, g_w, g_pre_out, wts, d2, log_temp, t_seed, v_s, lam_s, proj_s):
        gw, w, d2, lt, t = g_w.double(), wts.double(), d2.double(), log_temp.double(), t_seed.double()
        v, p, lam = v_s.double(), proj_s.double(), lam_s.double()
        E, L, D, _ = t.shape
        tau = softplus64(lt).unsqueeze(1)
        sig = torch.sigmoid(lt)
        dotw = (w * gw).sum(1, keepdim=True)
        g_pre = w * (gw - dotw)
        gpo = torch.zeros_like(g_pre) if g_pre_out is None else g_pre_out.double()
        g_pre = g_pre + gpo
        g_d2 = -g_pre / tau
        self.g_lt = sig * (g_pre * d2).sum(1) / (tau.squeeze(1) ** 2)
        gap = lam.unsqueeze(1) - lam.unsqueeze(2)                     # [b, a] = lam_a - lam_b
        tie = gap == 0
        safe = torch.where(tie, torch.ones_like(gap), gap)
        self.ties = int(tie.sum()) - E * D
        self.min_gap = float(safe.abs().min())
        c = torch.einsum("ej,ejba->eba", g_d2, t)
        k = torch.where(tie, torch.zeros_like(c), c / safe)
        gg = v.transpose(1, 2) @ k @ v
        self.w_tok = p.t() @ (gg + gg.transpose(1, 2)) @ p

        def bounds(kw, klt):
            d_pre = kw * U * (w * (gw.abs() + L * (w * gw).abs().sum(1, keepdim=True)) + gpo.abs())
            d_d2 = (d_pre + kw * U * g_pre.abs()) / tau
            d_c = torch.einsum("ej,ejba->eba", kw * U * g_d2.abs() + d_d2, t.abs())
            d_k = torch.where(tie, torch.zeros_like(c), d_c / safe.abs())
            av, ap = v.abs(), p.abs()
            spread = lambda m: ap.t() @ ((lambda q: q + q.transpose(1, 2))(av.transpose(1, 2) @ m @ av)) @ ap
            w_b = spread(d_k) + U * self.w_tok.abs() + 8 * D * V * spread(k.abs())
            d_pre_lt = d_pre * (klt / kw)
            lt_b = sig / (tau.squeeze(1) ** 2) * (d_pre_lt * d2.abs() + (klt + L) * U * (g_pre * d2).abs()).sum(1)
            return w_b, lt_b
        self.w_b, self.g_lt_b = bounds(K_AB_W, K_AB_LT)

    def ratios(self, g_lt, w_tok) -> dict:
        return {"g_lt": ratio(g_lt, self.g_lt, self.g_lt_b), "w_tok": ratio(w_tok, self.w_tok, self.w_b)}


def ab_chain32(g_w, g_pre_out, wts, d2, log_temp, t_seed, v_s, lam_s, proj_s):
    """the arithmetic of the entry as a torch chain: fp32 up to the products g_d2 T, fp64 from their sum on, one fp32
    rounding at the end -> (g_lt fp32, w_tok fp32)"""
    tau = torch.nn.functional.softplus(log_temp.float()).unsqueeze(1)
    g_pre = wts * (g_w - (wts * g_w).sum(1, keepdim=True))
    if g_pre_out is not None:
        g_pre = g_pre + g_pre_out
    g_d2 = -g_pre / tau
    g_lt = (g_pre * d2).sum(1) / (tau.squeeze(1) * tau.squeeze(1)) * torch.sigmoid(log_temp.float())
    c = (g_d2.view(*g_d2.shape, 1, 1) * t_seed).double().sum(1)
    gap = lam_s.unsqueeze(1) - lam_s.unsqueeze(2)
    k = torch.where(gap != 0, c / torch.where(gap != 0, gap, torch.ones_like(gap)), torch.zeros_like(c))
    v, p = v_s.double(), proj_s.double()
    gg = v.transpose(1, 2) @ k @ v
    return g_lt, (p.t() @ (gg + gg.transpose(1, 2)) @ p).float()


# ======================================================================================================================
# health-word flag (csrc/selector.hip, flag_if_exceeds_kernel)
# ======================================================================================================================
FLAG_SIZES = [1, 63, 64, 255, 256, 257, 65536, 65537, 200001]
FLAG_TOL = 1.0 + 2.0 ** -30
FLAG_KINDS = {"above": (float(torch.nextafter(torch.tensor(FLAG_TOL, dtype=torch.float64),
                                              torch.tensor(2.0, dtype=torch.float64))), 1),
              "nan": (float("nan"), 2), "inf": (float("inf"), 0x1000)}       # kind -> (offending value, bit to raise)
FlagLaunch = collections.namedtuple("FlagLaunch", "grid trips last_trip cap")


def flag_launch(n: int) -> FlagLaunch:
    """basd_flag_if_exceeds_f64: min(ceil(n / 256), 256) workgroups of 256 lanes, grid-stride"""
    grid = min(_ceil(n, 256), FLAG_CAP)
    per = grid * 256
    trips = _ceil(n, per)
    limit = FLAG_CAP * 256
    return FlagLaunch(grid, trips, n - (trips - 1) * per, "below" if n < limit else "at" if n == limit else "above")


def flag_positions(n: int):
    """where the single offender sits: the first and the last index, and both sides of the grid-stride wrap"""
    return sorted({0, n - 1} | {i for i in (65535, 65536) if i < n})


def flag_clean(n: int) -> torch.Tensor:
    """fp64 values none of which offends: exactly tol, -inf, -0.0 and values below"""
    v = torch.full((n,), FLAG_TOL, dtype=torch.float64)
    v[1::3] = -float("inf")
    v[2::3] = -0.0
    v[5::7] = 0.25
    return v


# ======================================================================================================================
# Schedule-Free AdamW step and lerp (csrc/optim.hip)
# ======================================================================================================================
ADCase = collections.namedtuple("ADCase", "n ckp1 bc2 wd")
LPCase = collections.namedtuple("LPCase", "n w")
AD_HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8)
AD_PASS = OPT_CAP * OPT_LANES * 4                    # 2 097 152 parameters per grid-stride trip
AD_SIZES = [1, 3, 4, 5, 6, 1023, 1024, 1027, AD_PASS - 1, AD_PASS, AD_PASS + 1, AD_PASS + 1027, 5_000_003]
AD_SCALARS = [(ckp1, bc2, wd) for ckp1 in (1.0, 0.25) for bc2 in (1.0 - 0.999, 0.3) for wd in (0.0, 0.05)]
AD_CASES = ([ADCase(n, *s) for n in AD_SIZES if n <= 1027 for s in AD_SCALARS]
            + [ADCase(n, *s) for n in AD_SIZES if 1027 < n < 5_000_000 for s in (AD_SCALARS[7], AD_SCALARS[0])]
            + [ADCase(5_000_003, *AD_SCALARS[7])])
LP_PASS = OPT_CAP * OPT_LANES                        # 524 288 elements per grid-stride trip
LP_SIZES = [1, 255, 256, 257, LP_PASS - 1, LP_PASS, LP_PASS + 1, 1_300_001]
LP_WEIGHTS = [0.0, 1.0, 1.0 - 1.0 / 0.9]
LP_CASES = [LPCase(n, w) for n in LP_SIZES for w in LP_WEIGHTS]


def ad_id(c: ADCase) -> str:
    return f"n{c.n}-ckp1_{c.ckp1}-bc2_{c.bc2:.3g}-wd{c.wd}"


def lp_id(c: LPCase) -> str:
    return f"n{c.n}-w{c.w:.4g}"


OptLaunch = collections.namedtuple("OptLaunch", "grid trips last_trip tail cap")


def _strided(items: int, limit_items: int):
    grid = max(1, min(_ceil(items, OPT_LANES), OPT_CAP))
    per = grid * OPT_LANES
    trips = _ceil(items, per)
    return grid, trips, items - (trips - 1) * per if trips else 0, \
        "below" if items < limit_items else "at" if items == limit_items else "above"


def ad_launch(n: int) -> OptLaunch:
    """basd_sf_adamw_step: n / 4 float4 items on clamp(ceil(n4 / 256), 1, 2048) workgroups, grid-stride; the n % 4 tail
    elements on the first lanes of workgroup 0"""
    grid, trips, last, cap = _strided(n // 4, OPT_CAP * OPT_LANES)
    return OptLaunch(grid, trips, last, n - 4 * (n // 4), cap)


def lp_launch(n: int) -> OptLaunch:
    """basd_lerp: n elements on min(ceil(n / 256), 2048) workgroups, grid-stride"""
    grid, trips, last, cap = _strided(n, OPT_CAP * OPT_LANES)
    return OptLaunch(grid, trips, last, 0, cap)


def index_signature(n: int) -> torch.Tensor:
    """fp32 in [0.5, 1.5), a hash of the index: equal for no two neighbours and for no two elements a trip apart"""
    i = torch.arange(n, dtype=torch.int64)
    return (0.5 + ((i * 2654435761) % (2 ** 32)).double() / 2.0 ** 32).float()


# special elements, by position in a run of 8: none, g = 0 and v = 0 (the update is exactly wd y), g = 0 with v > 0,
# |g| = 1e-20 on v = 0 (v underflows), |g| = 1e3, both signs
AD_KINDS = ["none", "g0v0", "g0", "tiny+", "big+", "tiny-", "big-", "none"]


def ad_special_runs(n: int):
    """first indices of the runs of special elements: the start, the end, both sides of the grid-stride wrap"""
    return sorted({a for a in (0, n - 8, AD_PASS - 4, AD_PASS + 4) if 0 <= a and a + 8 <= n} | {0})


def ad_inputs(case: ADCase):
    """(y, g, z, v) fp32 [n]; v carries the index signature"""
    n = case.n
    gen = _gen(n, 11)
    y, g, z = (torch.randn(n, generator=gen) for _ in range(3))
    v = index_signature(n)
    for a in ad_special_runs(n):
        for k, kind in enumerate(AD_KINDS):
            if a + k >= n:
                break
            if kind in ("g0v0", "g0"):
                g[a + k] = 0.0
            if kind in ("g0v0", "tiny+", "tiny-"):
                v[a + k] = 0.0
            if kind.startswith("tiny"):
                g[a + k] = 1e-20 if kind.endswith("+") else -1e-20
            if kind.startswith("big"):
                g[a + k] = 1e3 if kind.endswith("+") else -1e3
    return y, g, z, v


def lp_inputs(case: LPCase):
    gen = _gen(case.n, 13)
    return torch.randn(case.n, generator=gen) * index_signature(case.n), torch.randn(case.n, generator=gen)


def ad_kwargs(case: ADCase) -> dict:
    return dict(AD_HYPER, weight_decay=case.wd, ckp1=case.ckp1, bias_correction2=case.bc2)


def ad_scalars(case: ADCase) -> dict:
    """the kernel's scalar arguments as basd_sf_adamw_step forms them: in double, then rounded to float"""
    h = AD_HYPER
    return dict(lr=f32(h["lr"]), y_step=f32(h["lr"] * (h["beta1"] * (1.0 - case.ckp1) - 1.0)), beta2=f32(h["beta2"]),
                omb2=f32(1.0 - h["beta2"]), eps=f32(h["eps"]), wd=f32(case.wd), ckp1=f32(case.ckp1),
                inv_bc2=f32(1.0 / case.bc2))


# The bounds: a few u of the sum of the absolute values of the terms of each update, plus what the error of gn moves.
#   v' = beta2 v + omb2 g^2:  K u (|beta2 v| + omb2 g^2) + 2^-126 (g^2 = 1e-40 is denormal or flushed).
#   denom = sqrt(v' / bc2) + eps:  d denom = K u denom + sqrt(2^-126 / bc2)   (|sqrt a - sqrt b| <= sqrt |a - b|: the
#           absolute part of v's error; its relative part is halved by the root and is inside K u).
#   gn = g / denom + wd y:  d gn = |g / denom| (d denom / denom + K u) + K u |wd y| + 2^-126.
#   y' = y + ckp1 (z - y) + y_step gn:  K u (|y| + |ckp1 (z - y)| + |y_step| (|g / denom| + |wd y|)) + |y_step| d gn.
#   z' = z - lr gn:  K u (|z| + lr (|g / denom| + |wd y|)) + lr d gn.
#   lerp: y + w (z - y):  K u (|y| + |w (z - y)|).
K_AD = 6.0           # CPU worst at K = 1: y 2.58, z 1.17, v 1.98 (5 000 003 and 2 097 151 elements)
K_LP = 4.0           # CPU worst at K = 1: 1.92 (524 288 elements, w = 1)


class ADRef:
    def __init__(self, y, g, z, v, case: ADCase):
        s = ad_scalars(case)
        y, g, z, v = y.double(), g.double(), z.double(), v.double()
        k = K_AD
        self.v = s["beta2"] * v + s["omb2"] * g * g
        self.v_b = k * U * ((s["beta2"] * v).abs() + s["omb2"] * g * g) + TINY
        denom = torch.sqrt(self.v * s["inv_bc2"]) + s["eps"]
        d_denom = k * U * denom + math.sqrt(TINY * s["inv_bc2"])
        ga, wy = (g / denom).abs(), (s["wd"] * y).abs()
        gn = g / denom + s["wd"] * y
        d_gn = ga * (d_denom / denom + k * U) + k * U * wy + TINY
        self.y = y + s["ckp1"] * (z - y) + s["y_step"] * gn
        self.y_b = k * U * (y.abs() + (s["ckp1"] * (z - y)).abs() + abs(s["y_step"]) * (ga + wy)) + abs(s["y_step"]) * d_gn + TINY
        self.z = z - s["lr"] * gn
        self.z_b = k * U * (z.abs() + s["lr"] * (ga + wy)) + s["lr"] * d_gn + TINY

    def ratios(self, y, z, v) -> dict:
        return {"y": ratio(y, self.y, self.y_b), "z": ratio(z, self.z, self.z_b), "v": ratio(v, self.v, self.v_b)}


class LPRef:
    def __init__(self, y, z, w: float):
        w = f32(w)
        y, z = y.double(), z.double()
        self.y = y + w * (z - y)
        self.y_b = K_LP * U * (y.abs() + (w * (z - y)).abs()) + TINY

    def ratios(self, y) -> dict:
        return {"y": ratio(y, self.y, self.y_b)}

"""Case list, inputs and bounds of tests/test_layernorm_family_gpu.py.

A plain-Python mirror of the HOST arithmetic of csrc/layernorm.hip -- the template configuration (G, NCH, U) picked from
D / 8, ``ln_grid`` and the grid-stride loops of ``ln_fwd_kernel`` / ``ln_bwd_kernel`` -- which must be updated together
with them.  It says which configuration a case launches, on how many workgroups and in how many loop trips, so that the
case list cannot drift into shapes that no longer take the paths they are there for (pinned by
tests/test_ln_cases_cpu.py); it is bookkeeping for the GPU cases, not evidence about the kernels.

Also the input builders (CPU generators: the same case has the same inputs everywhere) and the error bounds.  The
bounds take any device and work in fp64; tests/test_ln_cases_cpu.py applies them to the emulation of tests/_emul.py,
tests/test_layernorm_family_gpu.py to the kernels.
"""
from __future__ import annotations

import collections

import torch

# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
WIDTHS = [8, 192, 248, 256, 264, 512, 520, 768, 1024, 1032, 1536, 1544, 2048]
ROWS = [1, 2, 3, 37, 131]
REGIMES = ["plain", "trained"]
# (rows, D): the forward's grid of 2048 workgroups wraps from 2048 * 4 * (64 / G) * U rows on; one per configuration
# (two at G = 32: the narrowest row and a full chunk column)
FWD_WRAP = [(65536 + 33, 8), (65536 + 33, 256), (32768 + 9, 264), (16384 + 5, 520), (8192 + 3, 1032), (8192 + 3, 1544)]
# the backward's grid of 512 workgroups is sized for 4 * (64 / G) * 4 rows each, whatever the kernel's own U: the
# smallest D of each configuration, just above 512 workgroups' worth of rows
BWD_WRAP = [(16384 + 5, 8), (8192 + 3, 264), (8192 + 3, 520), (8192 + 3, 1032), (8192 + 3, 1544)]
# the fp32 evaluation LayerNorm (csrc/eval_f32x3.hip): one wave per row, 4 rows per workgroup, float4 chunks
F32_WIDTHS = [4, 12, 252, 256, 260, 2044, 2048]
F32_ROWS = [1, 3, 5, 131]

EPS = 1e-6                                        # timm's nn.LayerNorm eps of the ViT blocks
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))     # what the kernels receive: `float eps`
GUARD = 64                                        # rows behind `rows` in every output buffer of the GPU tests
SENTINEL_BF16 = 0x7FC1                            # quiet-NaN payloads no kernel produces
SENTINEL_F32 = 0x7FC00D1E
CONSTANT_ROWS = [100.0, -37.5, 0.0, 1e-3]         # appended to every trained-regime case
OFFSET_ROW = 30.0                                 # and one row of 0.7 randn around it: mean^2 = 1800 var


def case_rows(rows: int, regime: str) -> int:
    """rows a width case launches: the trained regime appends the four constant rows and the offset row"""
    return rows + (len(CONSTANT_ROWS) + 1 if regime == "trained" else 0)


WIDTH_CASES = [(rows, D, regime) for D in WIDTHS for rows in ROWS for regime in REGIMES]


def case_id(case) -> str:
    return "x".join(str(v) for v in case[:2]) + "".join(f"-{v}" for v in case[2:])


# ------------------------------------------------------------------------------------------------------------------
# mirror of the launchers (csrc/layernorm.hip)
# ------------------------------------------------------------------------------------------------------------------
CONFIGS = [(32, 1, 4), (64, 1, 4), (64, 2, 2), (64, 3, 1), (64, 4, 1)]
FWD_CAP, BWD_CAP = 2048, 512


def config(D: int):
    """(G, NCH, U) of launch_ln_fwd / basd_layernorm_bwd_bf16"""
    assert D % 8 == 0 and 8 <= D <= 2048
    nchunk = D // 8
    for limit, cfg in zip((32, 64, 128, 192, 256), CONFIGS):
        if nchunk <= limit:
            return cfg
    raise AssertionError(D)


def ln_grid(rows: int, rows_per_wg: int, cap: int = FWD_CAP) -> int:
    return max(1, min((rows + rows_per_wg - 1) // rows_per_wg, cap))


Launch = collections.namedtuple("Launch", "config grid trips t full_last_column ragged_tail dead_second_group")


def _launch(rows: int, D: int, rows_per_wg: int, cap: int) -> Launch:
    G, NCH, U = cfg = config(D)
    grid = ln_grid(rows, rows_per_wg, cap)
    wstride = grid * 4 * (64 // G)                 # row groups of the grid = rows between the u of one group
    period = wstride * U                           # rows of one loop trip of the whole grid
    trips = (rows + period - 1) // period          # of the busiest row group (the one that starts at row 0)
    # in the last, partial trip the groups with r0 < rows are live and hold a dead row u > 0: their r0 + (U - 1) wstride
    # is >= wstride > r0's trip remainder, or, if more than wstride rows remain, the last group's is >= the remainder
    ragged = U > 1 and rows % period != 0
    # G = 32: rows r0 and r0 + 1 share a wave; an odd row count leaves the last live wave without its second row
    dead_second = G == 32 and rows % 2 == 1
    return Launch(cfg, grid, trips, trips * U, D // 8 == NCH * G, ragged, dead_second)


def forward(rows: int, D: int) -> Launch:
    G, _NCH, U = config(D)
    return _launch(rows, D, 4 * (64 // G) * U, FWD_CAP)


def backward(rows: int, D: int) -> Launch:
    G, _NCH, _U = config(D)
    return _launch(rows, D, 4 * (64 // G) * 4, BWD_CAP)


def rows_visited(rows: int, D: int, which: str) -> collections.Counter:
    """row -> how many (workgroup, wave, row group, trip, u) process it: the loops of the two kernels, walked"""
    la = forward(rows, D) if which == "forward" else backward(rows, D)
    G, _NCH, U = la.config
    rpw = 64 // G
    wstride = la.grid * 4 * rpw
    seen = collections.Counter()
    for block in range(la.grid):
        for wave in range(4):
            for sub in range(rpw):
                r0 = (block * 4 + wave) * rpw + sub
                while r0 < rows:
                    for u in range(U):
                        if r0 + u * wstride < rows:
                            seen[r0 + u * wstride] += 1
                    r0 += wstride * U
    return seen


# ------------------------------------------------------------------------------------------------------------------
# inputs (CPU tensors, seeded generators)
# ------------------------------------------------------------------------------------------------------------------
def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1_000_003 + int(k) + 17) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


def spike_columns(D: int) -> torch.Tensor:
    """the max(1, D // 96) fixed columns of the trained regime that sit 80 above the rest"""
    return torch.randperm(D, generator=_gen(D, 5))[:max(1, D // 96)]


def inputs(rows: int, D: int, regime: str) -> dict:
    """x, r (a residual), dy, dres: bf16 [case_rows, D]; gamma = 1 + 0.5 randn, beta = 0.1 randn: fp32 [D].
    plain: x = bf16(randn).  trained: x = bf16(0.7 randn + 3) with the spike columns raised by 80 -- a ViT residual
    stream: a common offset and a few channels 50 to 200 times larger than the rest -- four constant rows behind them
    (rstd = eps^-1/2 there) and one row of 0.7 randn + 30.  The last one is what tells a one-pass variance from the
    kernel's: on bf16 constants fl(1 / D) sum X rounds back to X and mean(x^2) - mean^2 is exactly 0, and on the
    spiked rows mean^2 is a fifth of the variance, so a one-pass variance is good to 4 u there (measured) and no sound
    bound can reject it; at mean^2 = 1800 var it is off by thousands of u."""
    g = _gen(rows, D, REGIMES.index(regime))
    if regime == "plain":
        x = torch.randn(rows, D, generator=g)
    else:
        x = 0.7 * torch.randn(rows, D, generator=g) + 3.0
        x[:, spike_columns(D)] += 80.0
        x = torch.cat([x] + [torch.full((1, D), v) for v in CONSTANT_ROWS]
                      + [0.7 * torch.randn(1, D, generator=g) + OFFSET_ROW])
    n = x.shape[0]
    assert n == case_rows(rows, regime)
    return {"x": x.bfloat16(), "r": torch.randn(n, D, generator=g).bfloat16(),
            "dy": torch.randn(n, D, generator=g).bfloat16(), "dres": torch.randn(n, D, generator=g).bfloat16(),
            "gamma": 1.0 + 0.5 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g)}


SCALES = [0.0, 1.0, float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(0.7, dtype=torch.float32))]


def scaled_add_inputs(rows: int, D: int) -> dict:
    """x, r: bf16 of +-2^U(-6, 6), so |x|, |r| in [2^-6, 2^6]: with a row scale from SCALES (24 bits), r + sc x spans
    at most 2^-36 .. 2^7 -- fp64 holds it exactly, and fp32 rounds it once, like the kernel's fma"""
    g = _gen(rows, D, 77)

    def draw():
        mag = torch.exp2(12.0 * torch.rand(rows, D, generator=g) - 6.0).bfloat16().float().clamp(2.0 ** -6, 2.0 ** 6)
        sign = 1.0 - 2.0 * torch.randint(0, 2, (rows, D), generator=g)
        return (sign * mag).bfloat16()

    return {"x": draw(), "r": draw(), "gamma": 1.0 + 0.5 * torch.randn(D, generator=g),
            "beta": 0.1 * torch.randn(D, generator=g)}


def row_scales(rows: int, rows_per_scale: int) -> torch.Tensor:
    """fp32 [ceil(rows / rows_per_scale)]: 0, 1 and fp32(1 / 0.7) in a seeded random order, each present if it fits"""
    n = (rows + rows_per_scale - 1) // rows_per_scale
    g = _gen(rows, rows_per_scale, 3)
    pick = torch.cat([torch.arange(3), torch.randint(0, 3, (max(0, n - 3),), generator=g)])[:n]
    pick = pick[torch.randperm(n, generator=g)]
    return torch.tensor(SCALES, dtype=torch.float32)[pick]


def scale_row_counts(rows: int):
    """the rows_per_scale of the row-scale cases: one row, seven rows and a third of the rows per sample"""
    return sorted({1, 7, max(1, rows // 3)})


def f32_inputs(rows: int, D: int, regime: str) -> dict:
    """the fp32 evaluation LayerNorm's inputs: as ``inputs``, not rounded to bf16; xscale is a LayerScale gamma"""
    g = _gen(rows, D, 31 + REGIMES.index(regime))
    if regime == "plain":
        x = torch.randn(rows, D, generator=g)
    else:
        x = 0.7 * torch.randn(rows, D, generator=g) + 3.0
        x[:, spike_columns(D) if D >= 8 else torch.tensor([1])] += 80.0
        x = torch.cat([x] + [torch.full((1, D), v) for v in CONSTANT_ROWS]
                      + [0.7 * torch.randn(1, D, generator=g) + OFFSET_ROW])
    n = x.shape[0]
    return {"x": x, "res": torch.randn(n, D, generator=g), "xscale": torch.rand(D, generator=g) + 0.5,
            "gamma": 1.0 + 0.5 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g)}


# ------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------
# u = 2^-24 is fp32's unit roundoff, 2^-8 bf16's.  An fp32 value v32 within e32 of the exact v64 rounds to a bf16 with
#     |bf16(v32) - v64| <= 2^-8 |v32| + |v32 - v64| <= 2^-8 |v64| + (1 + 2^-8) e32,
# so every bf16 output is checked per element as err <= 2^-8 |ref| + (1 + 2^-8) e32 and every fp32 output as
# err <= e32.  Nothing is relative to the largest element; an exactly correct element passes a zero bound.
#
# Row sums (``depth``).  A lane adds its 8 NCH columns one after the other (8 NCH - 1 roundings behind the first
# term), the DPP / permlane tree over the G <= 64 lanes adds 6 levels, 1 / D is rounded once and the product with it
# once more: 8 NCH + 7 roundings on any path from a term to the mean.  n = 8 NCH + 9 leaves two for a term that is
# itself a rounded product (g = dy gamma) and for the second-order terms, so
#     |fl(mean of v) - mean of v| <= n u mean|v|.
U32 = 2.0 ** -24
UBF16 = 2.0 ** -8
F32_DEPTH = 20        # ln_f32_kernel: a pair tree inside a float4 (2), 8 float4 per lane (8), 6 tree levels, the
#                       division by D (<= 2 u), two spare as above


def depth(nch: int) -> int:
    return 8 * nch + 9


def ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err / bound; an exact element passes a zero bound; a NaN (in the output, or read from where none should be
    read) fails"""
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    assert not bool(torch.isnan(q).any()), "NaN in an output"
    return float(q.max()) if q.numel() else 0.0


def forward_reference(x, gamma, beta):
    """fp64 LayerNorm of x [rows, D] (any float dtype): mu, var, rs [rows, 1]; xh, y [rows, D]"""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    c = xd - mu
    var = (c * c).mean(-1, keepdim=True)
    rs = (var + EPS32).rsqrt()
    xh = c * rs
    return mu, var, rs, xh, xh * gamma.double() + beta.double()


def mean_bound(x, n: int):
    """|mean - mu| <= d_mu = n u mean|x| (see above), [rows, 1]"""
    return n * U32 * x.double().abs().mean(-1, keepdim=True)


def rstd_rel_bound(var, d_mu, n: int, rsqrt_u: int = 2):
    """|rstd / rs - 1| <= (n / 2 + 2 + rsqrt_u) u + d_mu^2 / (2 (var + eps)).

    The variance is two-pass: with mu_c = mu + D_mu the computed mean, sum (x - mu_c)^2 = sum (x - mu)^2 + D D_mu^2
    exactly (the cross term 2 D_mu sum (x - mu) vanishes), so the error of the mean enters in SECOND order only: the
    last term, which u-sized errors make negligible except on a constant row, where var = 0 and eps = 1e-6 is all there
    is to compare D_mu^2 with.  (A one-pass variance mean(x^2) - mean^2 carries u mean(x^2) / var instead, in first
    order: tests/test_ln_cases_cpu.py shows this bound rejecting it on the offset row of the trained regime.)  First order: x - mu_c is rounded once (relative to itself: 2 u on the square), the squares are
    added by fma -- one rounding per term, 8 NCH + 6 + 2 = n - 1 on a path through lane, tree and 1 / D -- and eps is
    added with one more: (n + 2) u on var + eps, halved by the inverse square root.  rsqrtf is good to one ulp,
    <= 2 u (``rsqrt_u``; 1 / sqrtf of the fp32 kernel: two such operations).  One u for the second-order terms."""
    return ((n + 2) / 2 + rsqrt_u + 1) * U32 + d_mu * d_mu / (2.0 * (var + EPS32))


def y_e32(gamma, rs, xh, ref, d_mu, rho):
    """fp32 error of y = fma((x - mu_c) rs_c, gamma, beta) before the rounding to bf16.

    (x - mu_c) rs_c = (x - mu - D_mu) (1 + e1) rs (1 + rho') (1 + e2), |rho'| <= rho: it differs from xh by at most
    |xh| k + rs d_mu (1 + k), 1 + k = (1 + u)^3 (1 + rho).  The third (1 + u) is the product with gamma where it is
    rounded on its own (the emulation; the kernel's fma rounds product and sum together).  The last rounding is
    relative to the computed value.  The rs d_mu term is what lets a constant row of 100s through honestly: fl(1 / D)
    sum X need not equal X, and rs is 1000 there."""
    k = (1.0 + U32) ** 3 * (1.0 + rho) - 1.0
    inner = gamma.double().abs() * (xh.abs() * k + rs * d_mu * (1.0 + k))
    return inner + U32 * (ref.abs() + inner)


_CHUNK = 1 << 22          # elements of an fp64 reference piece


def _pieces(rows: int, D: int):
    step = max(1, _CHUNK // D)
    return [(r0, min(r0 + step, rows)) for r0 in range(0, rows, step)]


def forward_ratios(x, gamma, beta, y, mean, rstd, n: int, rsqrt_u: int = 2) -> dict:
    """largest err / bound of y (bf16, or fp32 when y is fp32), mean and rstd (either may be None) against fp64 on the
    same inputs, in row chunks"""
    rows, D = x.shape
    worst = {"y": 0.0}
    bf16_term = UBF16 if y.dtype == torch.bfloat16 else 0.0
    for r0, r1 in _pieces(rows, D):
        mu, var, rs, xh, ref = forward_reference(x[r0:r1], gamma, beta)
        d_mu = mean_bound(x[r0:r1], n)
        rho = rstd_rel_bound(var, d_mu, n, rsqrt_u)
        e32 = y_e32(gamma, rs, xh, ref, d_mu, rho)
        worst["y"] = max(worst["y"], ratio((y[r0:r1].double() - ref).abs(), bf16_term * ref.abs() + (1 + bf16_term) * e32))
        if mean is not None:
            worst["mean"] = max(worst.get("mean", 0.0), ratio((mean[r0:r1].double().view(-1, 1) - mu).abs(), d_mu))
            worst["rstd"] = max(worst.get("rstd", 0.0), ratio((rstd[r0:r1].double().view(-1, 1) / rs - 1.0).abs(), rho))
    return worst


def backward_ratios(dy, x, gamma, mean, rstd, dx, la: Launch, dres=None, dbranch=None, scale_of_row=None,
                    dgamma=None, dbeta=None, prefill_gamma=None, prefill_beta=None) -> dict:
    """largest err / bound of the backward's outputs against fp64, as a function of ITS inputs: mean and rstd are the
    fp32 values passed in, whatever they are.

        xh = (x - mean) rstd,  g = dy gamma,  dx = rstd (g - mean(g) - xh mean(g xh)) + dres

    dx: with A = |g| + mean|g| + |xh| mean|g xh| the kernel's fp32 value is within (n + 8) u |rstd| A + u |dres|:
    xh carries 2 u and g one; mean(g) n u mean|g| and mean(g xh) (n + 2) u mean|g xh| (its terms are products of
    rounded factors); the product with xh and the two subtractions round three more times, each on at most A; that is
    (n + 6) u A inside the bracket, one more u for the product with rstd and one for the sum with dres, which also
    rounds dres's share.
    dbranch = bf16(sc * fp32 dx): the same bound times |sc|, and u |sc dx| for the product.
    dgamma[c] = sum_r dy xh, dbeta[c] = sum_r dy: a lane accumulates its t = trips * U rows by fma (t roundings; xh adds
    2 u per term), the two row groups and the four waves combine in 3 more, and every workgroup adds its partial to the
    global sum with one atomic, in any order (grid roundings): (t + 3 + grid + 2) u sum_r |dy xh|, and likewise
    sum_r |dy|.  They are accumulated INTO: dgamma / dbeta are the buffers after the launch and prefill_* what they
    held before; each of the grid atomics also rounds what is already there: + grid u |prefill|."""
    rows, D = x.shape
    n = depth(la.config[1])
    gd = gamma.double()
    worst = {"dx": 0.0}
    sum_g = torch.zeros(D, dtype=torch.float64, device=x.device)
    sum_b, abs_g, abs_b = sum_g.clone(), sum_g.clone(), sum_g.clone()
    for r0, r1 in _pieces(rows, D):
        m, s = mean[r0:r1].double().view(-1, 1), rstd[r0:r1].double().view(-1, 1)
        dyd = dy[r0:r1].double()
        xh = (x[r0:r1].double() - m) * s
        g = dyd * gd
        m2 = (g * xh).mean(-1, keepdim=True)
        ref = s * (g - g.mean(-1, keepdim=True) - xh * m2)
        A = g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)
        e32 = (n + 8) * U32 * s.abs() * A
        if dres is not None:
            dr = dres[r0:r1].double()
            ref = ref + dr
            e32 = e32 + U32 * dr.abs()
        worst["dx"] = max(worst["dx"], ratio((dx[r0:r1].double() - ref).abs(), UBF16 * ref.abs() + (1 + UBF16) * e32))
        if dbranch is not None:
            sc = torch.ones_like(s) if scale_of_row is None else scale_of_row[r0:r1].double().view(-1, 1)
            refb = sc * ref
            eb = sc.abs() * e32 + U32 * refb.abs()
            worst["dbranch"] = max(worst.get("dbranch", 0.0),
                                   ratio((dbranch[r0:r1].double() - refb).abs(), UBF16 * refb.abs() + (1 + UBF16) * eb))
        if dgamma is not None:
            p = dyd * xh
            sum_g += p.sum(0)
            abs_g += p.abs().sum(0)
            sum_b += dyd.sum(0)
            abs_b += dyd.abs().sum(0)
    if dgamma is not None:
        c = (la.t + 3 + la.grid + 2) * U32
        for name, got, pre, want, mag in (("dgamma", dgamma, prefill_gamma, sum_g, abs_g),
                                          ("dbeta", dbeta, prefill_beta, sum_b, abs_b)):
            pre = torch.zeros_like(want) if pre is None else pre.double()
            worst[name] = ratio((got.double() - pre - want).abs(), c * mag + la.grid * U32 * pre.abs())
    return worst


def f32_sum_ratio(s, x, res, xscale) -> float:
    """s = res + xscale x of the fp32 kernel: the product and the sum round once each (or once together, contracted
    into an fma): within 2 u (|x xscale| + |res|); without either operand s is x itself"""
    p = x.double() * (1.0 if xscale is None else xscale.double())
    want = p + (0.0 if res is None else res.double())
    bound = 2 * U32 * (p.abs() + (0.0 if res is None else res.double().abs()))
    if res is None and xscale is None:
        bound = torch.zeros_like(bound)
    return ratio((s.double() - want).abs(), bound)

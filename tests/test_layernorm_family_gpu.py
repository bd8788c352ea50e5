"""The LayerNorm kernels of csrc/layernorm.hip (basd_layernorm_fwd_bf16, basd_add_layernorm_fwd_bf16,
basd_layernorm_bwd_bf16) and the fp32 evaluation LayerNorm of csrc/eval_f32x3.hip (basd_add_layernorm_fwd_f32), per
element against fp64 on every dispatch path (GPU box only).  tests/_ln_cases.py holds the cases, the inputs and the
derived bounds, and says which path a case reaches (pinned by tests/test_ln_cases_cpu.py, which also holds the entries'
refusals: they need no GPU).

The C entries are called directly.  Every output is a caller-owned buffer with 64 guard rows behind ``rows``,
pre-filled with a NaN bit pattern no kernel produces (torch.empty may hand back the block that held the previous
launch's correct result): after a launch the guard rows must hold the pattern bit for bit and no row in front of them
may hold it, or any NaN."""
import pytest
import torch

from tests import _ln_cases as C

pytestmark = pytest.mark.gpu

_WORST = {}          # output -> (largest err / bound, case): printed when the module is done (pytest -s)


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    _CACHE.clear()
    for name, (v, case) in sorted(_WORST.items()):
        print(f"ln-worst {name}: {v:.4f} at {case}")


def _note(ratios, prefix, case):
    for name, v in ratios.items():
        print(f"ln-bound {prefix} {case} {name} {v:.4f}")
        if v >= _WORST.get(f"{prefix} {name}", (-1.0, None))[0]:
            _WORST[f"{prefix} {name}"] = (v, case)
        assert v <= 1.0, (prefix, name, case, v)


_CACHE = {}          # one entry per kind: the device inputs of the case under test


def _cached(kind, key, make):
    hit = _CACHE.get(kind)
    if hit is None or hit[0] != key:
        _CACHE.pop(kind, None)
        hit = _CACHE[kind] = (key, make())
    return hit[1]


def _inputs(rows, D, regime):
    return _cached("in", (rows, D, regime), lambda: {k: v.cuda() for k, v in C.inputs(rows, D, regime).items()})


# ------------------------------------------------------------------------------------------------------------------
# buffers with guard rows
# ------------------------------------------------------------------------------------------------------------------
def _bf16(rows, D):
    return torch.full((rows + C.GUARD, D), C.SENTINEL_BF16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _f32(rows, D=None):
    shape = (rows + C.GUARD,) if D is None else (rows + C.GUARD, D)
    return torch.full(shape, C.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(buf):
    return buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)


def _sentinel_of(buf):
    return C.SENTINEL_BF16 if buf.dtype == torch.bfloat16 else C.SENTINEL_F32


def _check_guards(bufs, rows, written=True):
    """the guard rows keep the sentinel bit for bit; rows < ``rows`` hold neither it nor any NaN (``written`` False:
    nothing at all was written)"""
    for name, buf in bufs.items():
        if buf is None:
            continue
        bits = _bits(buf)
        assert bool((bits[rows:] == _sentinel_of(buf)).all()), f"{name}: written behind row {rows}"
        if written:
            assert not bool((bits[:rows] == _sentinel_of(buf)).any()), f"{name}: a sentinel is left in the first {rows} rows"
            assert not bool(torch.isnan(buf[:rows].float()).any()), f"{name}: NaN"
        else:
            assert bool((bits == _sentinel_of(buf)).all()), f"{name}: written"


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------------------------
def _fwd(nat, x, gamma, beta, stats=True):
    rows, D = x.shape
    out = {"y": _bf16(rows, D), "mean": _f32(rows) if stats else None, "rstd": _f32(rows) if stats else None}
    p = nat._ptr
    rc = nat.lib().basd_layernorm_fwd_bf16(p(x), p(gamma), p(beta), rows, D, C.EPS, p(out["y"]), p(out["mean"]),
                                           p(out["rstd"]), nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    _check_guards(out, rows)
    return out


def _add_fwd(nat, x, r, gamma, beta, scale=None, rows_per_scale=1, stats=True):
    rows, D = x.shape
    out = {"sum": _bf16(rows, D), "y": _bf16(rows, D), "mean": _f32(rows) if stats else None,
           "rstd": _f32(rows) if stats else None}
    p = nat._ptr
    rc = nat.lib().basd_add_layernorm_fwd_bf16(p(x), p(r), p(gamma), p(beta), rows, D, C.EPS, p(out["sum"]), p(out["y"]),
                                               p(out["mean"]), p(out["rstd"]), p(scale), rows_per_scale, nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    _check_guards(out, rows)
    return out


def _bwd(nat, dy, x, gamma, mean, rstd, grads=None, dres=None, branch=False, scale=None, rows_per_scale=1):
    """grads: None (frozen layer: null dgamma / dbeta) or the (dgamma, dbeta) values the buffers hold before the launch"""
    rows, D = x.shape
    out = {"dx": _bf16(rows, D), "dbranch": _bf16(rows, D) if branch else None, "dgamma": None, "dbeta": None}
    if grads is not None:
        # [D] values and 64 guard elements behind them
        for name, pre in zip(("dgamma", "dbeta"), grads):
            out[name] = _f32(D)
            out[name][:D] = pre
    p = nat._ptr
    rc = nat.lib().basd_layernorm_bwd_bf16(p(dy), p(x), p(gamma), p(mean), p(rstd), rows, D, p(out["dx"]),
                                           p(out["dgamma"]), p(out["dbeta"]), p(dres), p(out["dbranch"]), p(scale),
                                           rows_per_scale, nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    _check_guards({"dx": out["dx"], "dbranch": out["dbranch"]}, rows)
    _check_guards({"dgamma": out["dgamma"], "dbeta": out["dbeta"]}, D)
    return out


# ------------------------------------------------------------------------------------------------------------------
# a. forward against fp64
# ------------------------------------------------------------------------------------------------------------------
def _check_forward(nat, rows, D, regime):
    a = _inputs(rows, D, regime)
    n_rows = a["x"].shape[0]
    la = C.forward(n_rows, D)
    out = _fwd(nat, a["x"], a["gamma"], a["beta"])
    got = C.forward_ratios(a["x"], a["gamma"], a["beta"], out["y"][:n_rows], out["mean"][:n_rows], out["rstd"][:n_rows],
                           C.depth(la.config[1]))
    _note(got, "fwd", (rows, D, regime))
    # without statistics (the frozen teacher's call): the same y
    assert _same_bits(_fwd(nat, a["x"], a["gamma"], a["beta"], stats=False)["y"], out["y"])
    return a, out


@pytest.mark.parametrize("regime", C.REGIMES)
@pytest.mark.parametrize("D", C.WIDTHS)
def test_forward_against_fp64_at_every_width(nat, D, regime):
    """basd_layernorm_fwd_bf16 on every configuration, with a full and a partial last chunk column, at 1, 2, 3, 37 and
    131 rows (ragged tails, dead second row groups), in both regimes: mean, rstd and every element of y inside the
    bounds of tests/_ln_cases.py."""
    for rows in C.ROWS:
        _check_forward(nat, rows, D, regime)


@pytest.mark.parametrize("case", C.FWD_WRAP, ids=C.case_id)
def test_forward_against_fp64_on_the_second_loop_trip(nat, case):
    """more rows than 2048 workgroups hold: the grid-stride loop makes a second trip, for an odd handful of rows"""
    rows, D = case
    assert C.forward(rows, D).trips == 2
    _check_forward(nat, rows, D, "plain")


# ------------------------------------------------------------------------------------------------------------------
# b. the fused residual add
# ------------------------------------------------------------------------------------------------------------------
def _check_fused_add(nat, rows, D, regime):
    a = _inputs(rows, D, regime)
    n_rows = a["x"].shape[0]
    out = _add_fwd(nat, a["x"], a["r"], a["gamma"], a["beta"])
    s_ref = a["x"] + a["r"]                                                # torch's bf16 add: one rounding of the fp32 sum
    assert torch.equal(out["sum"][:n_rows], s_ref), "sum_out is not bf16(x + r)"
    ref = _fwd(nat, s_ref, a["gamma"], a["beta"])
    for name in ("y", "mean", "rstd"):
        assert _same_bits(out[name], ref[name]), f"{name} differs from LayerNorm(sum_out)"
    quiet = _add_fwd(nat, a["x"], a["r"], a["gamma"], a["beta"], stats=False)
    assert _same_bits(quiet["y"], out["y"]) and _same_bits(quiet["sum"], out["sum"])


@pytest.mark.parametrize("regime", C.REGIMES)
@pytest.mark.parametrize("D", C.WIDTHS)
def test_fused_add_is_add_then_layernorm_bitwise(nat, D, regime):
    """without row_scale: sum_out is bitwise x + r in bf16 and y, mean, rstd are bitwise those of the plain entry on
    sum_out; with mean == rstd == NULL the same y"""
    for rows in C.ROWS:
        _check_fused_add(nat, rows, D, regime)


@pytest.mark.parametrize("case", C.FWD_WRAP, ids=C.case_id)
def test_fused_add_is_add_then_layernorm_bitwise_on_the_second_loop_trip(nat, case):
    _check_fused_add(nat, case[0], case[1], "plain")


def _check_scaled_add(nat, rows, D):
    a = _cached("scaled", (rows, D), lambda: {k: v.cuda() for k, v in C.scaled_add_inputs(rows, D).items()})
    for rps in C.scale_row_counts(rows):
        sc = C.row_scales(rows, rps).cuda()
        out = _add_fwd(nat, a["x"], a["r"], a["gamma"], a["beta"], scale=sc, rows_per_scale=rps)
        per_row = sc.repeat_interleave(rps)[:rows].double().view(-1, 1)
        step = max(1, (1 << 22) // D)
        for r0 in range(0, rows, step):
            want = (a["r"][r0:r0 + step].double() + per_row[r0:r0 + step] * a["x"][r0:r0 + step].double()).float().bfloat16()
            got = out["sum"][r0:min(r0 + step, rows)]
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                raise AssertionError(f"sum_out: {len(bad)} elements differ from bf16(fp32(r + sc x)), rows_per_scale "
                                     f"{rps}, the first at [{r0 + int(bad[0, 0])}, {int(bad[0, 1])}]")
        ref = _fwd(nat, out["sum"][:rows], a["gamma"], a["beta"])
        for name in ("y", "mean", "rstd"):
            assert _same_bits(out[name], ref[name]), f"{name} differs from LayerNorm(sum_out), rows_per_scale {rps}"
        quiet = _add_fwd(nat, a["x"], a["r"], a["gamma"], a["beta"], scale=sc, rows_per_scale=rps, stats=False)
        assert _same_bits(quiet["y"], out["y"]) and _same_bits(quiet["sum"], out["sum"])


@pytest.mark.parametrize("D", C.WIDTHS)
def test_fused_add_with_row_scale_is_exact(nat, D):
    """row_scale of 0, 1 and fp32(1 / 0.7) mixed over the samples, 1, 7 and rows / 3 rows per sample, |x| and |r| in
    [2^-6, 2^6]: r + sc x is exact in fp64, so sum_out EQUALS bf16(fp32(r + sc x)) -- the kernel's one fma and one
    rounding to bf16 -- with no tolerance; y and the statistics are bitwise those of the plain entry on sum_out."""
    for rows in C.ROWS:
        _check_scaled_add(nat, rows, D)


def test_fused_add_with_row_scale_is_exact_on_the_second_loop_trip(nat):
    rows, D = C.FWD_WRAP[2]
    _check_scaled_add(nat, rows, D)


# ------------------------------------------------------------------------------------------------------------------
# c. backward against fp64, as a function of its inputs
# ------------------------------------------------------------------------------------------------------------------
def _prefill(D):
    g = torch.Generator().manual_seed(D + 1)
    return torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()


def _check_backward(nat, rows, D, regime, perturb=False):
    a = _inputs(rows, D, regime)
    n_rows = a["x"].shape[0]
    la = C.backward(n_rows, D)
    stats = _fwd(nat, a["x"], a["gamma"], a["beta"])
    mean, rstd = stats["mean"][:n_rows].clone(), stats["rstd"][:n_rows].clone()
    if perturb:                                    # any mean / rstd: the entry is a function of what it is given
        g = torch.Generator().manual_seed(D)
        mean *= (1 + 0.03 * torch.randn(n_rows, generator=g)).cuda()
        rstd *= (1 + 0.03 * torch.randn(n_rows, generator=g)).cuda()
    rps = max(1, n_rows // 3)
    sc = C.row_scales(n_rows, rps).cuda()
    per_row = sc.repeat_interleave(rps)[:n_rows]
    pre = _prefill(D)
    full = _bwd(nat, a["dy"], a["x"], a["gamma"], mean, rstd, grads=pre, dres=a["dres"], branch=True, scale=sc,
                rows_per_scale=rps)
    got = C.backward_ratios(a["dy"], a["x"], a["gamma"], mean, rstd, full["dx"][:n_rows], la, dres=a["dres"],
                            dbranch=full["dbranch"][:n_rows], scale_of_row=per_row, dgamma=full["dgamma"][:D],
                            dbeta=full["dbeta"][:D], prefill_gamma=pre[0], prefill_beta=pre[1])
    assert set(got) == {"dx", "dbranch", "dgamma", "dbeta"}
    _note(got, "bwd", (rows, D, regime) + (("perturbed",) if perturb else ()))
    # no residual gradient, no branch, gradients accumulated into zeros
    zeros = (torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"))
    plain = _bwd(nat, a["dy"], a["x"], a["gamma"], mean, rstd, grads=zeros)
    got = C.backward_ratios(a["dy"], a["x"], a["gamma"], mean, rstd, plain["dx"][:n_rows], la, dgamma=plain["dgamma"][:D],
                            dbeta=plain["dbeta"][:D])
    _note(got, "bwd-plain", (rows, D, regime) + (("perturbed",) if perturb else ()))
    # frozen layer: null dgamma / dbeta, the same dx
    frozen = _bwd(nat, a["dy"], a["x"], a["gamma"], mean, rstd)
    assert _same_bits(frozen["dx"], plain["dx"])
    frozen = _bwd(nat, a["dy"], a["x"], a["gamma"], mean, rstd, dres=a["dres"], branch=True, scale=sc, rows_per_scale=rps)
    assert _same_bits(frozen["dx"], full["dx"]) and _same_bits(frozen["dbranch"], full["dbranch"])
    # dres without dbranch: the full call's dx; dbranch without row_scale: dx itself
    part = _bwd(nat, a["dy"], a["x"], a["gamma"], mean, rstd, dres=a["dres"])
    assert _same_bits(part["dx"], full["dx"])
    part = _bwd(nat, a["dy"], a["x"], a["gamma"], mean, rstd, dres=a["dres"], branch=True)
    assert _same_bits(part["dx"], full["dx"]) and _same_bits(part["dbranch"], full["dx"])


@pytest.mark.parametrize("regime", C.REGIMES)
@pytest.mark.parametrize("D", C.WIDTHS)
def test_backward_against_fp64_at_every_width(nat, D, regime):
    """basd_layernorm_bwd_bf16 with the forward's mean / rstd, dres, dbranch with a row scale (0, 1, 1 / 0.7) and
    dgamma / dbeta accumulated into random values: every element of dx, dbranch, dgamma - prefill and dbeta - prefill
    inside the bounds of tests/_ln_cases.py; the calls with fewer operands give bitwise the same outputs."""
    for rows in C.ROWS:
        _check_backward(nat, rows, D, regime)


@pytest.mark.parametrize("D", [8, 264, 768, 1544, 2048])
def test_backward_is_a_function_of_the_statistics_it_is_given(nat, D):
    """mean and rstd off by a few percent (not those of x): the reference follows them, the bounds stay"""
    _check_backward(nat, 37, D, "trained", perturb=True)


@pytest.mark.parametrize("case", C.BWD_WRAP, ids=C.case_id)
def test_backward_against_fp64_beyond_512_workgroups(nat, case):
    rows, D = case
    la = C.backward(rows, D)
    assert la.grid == C.BWD_CAP and la.trips == 4 // la.config[2] + 1
    _check_backward(nat, rows, D, "plain")


# ------------------------------------------------------------------------------------------------------------------
# d. the fp32 evaluation LayerNorm
# ------------------------------------------------------------------------------------------------------------------
def _ln_f32(nat, x, res, xscale, gamma, beta, want_s, want_y, want_img):
    rows, D = x.shape
    out = {"s": _f32(rows, D) if want_s else None, "y": _f32(rows, D) if want_y else None,
           "img": _bf16(rows, 2 * D) if want_img else None}
    p = nat._ptr
    rc = nat.lib().basd_add_layernorm_fwd_f32(p(x), p(res), p(xscale), p(gamma), p(beta), rows, D, C.EPS, p(out["s"]),
                                              p(out["y"]), p(out["img"]), nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    _check_guards(out, rows)
    return out


@pytest.mark.parametrize("regime", C.REGIMES)
@pytest.mark.parametrize("D", C.F32_WIDTHS)
def test_fp32_layernorm_against_fp64(nat, D, regime):
    """basd_add_layernorm_fwd_f32 at one chunk per row, around one chunk per lane (252 / 256 / 260) and around eight
    (2044 / 2048), at 1, 3, 5 and 131 rows (the ``r >= rows`` exit of the last workgroup's waves), with and without
    residual and xscale.  s within 2 u (|x xscale| + |res|); y against the fp64 LayerNorm of the kernel's own s, within
    the fp32 part of the bf16 kernels' bound (n = 20, see _ln_cases.F32_DEPTH; 1 / sqrtf counts 4 u); the image
    reconstructs y to 2^-16 |y|; every accepted subset of the outputs is bitwise the full call's."""
    for rows in C.F32_ROWS:
        a = _cached("f32", (rows, D, regime), lambda: {k: v.cuda() for k, v in C.f32_inputs(rows, D, regime).items()})
        n_rows = a["x"].shape[0]
        for res, xscale in ((None, None), (a["res"], None), (None, a["xscale"]), (a["res"], a["xscale"])):
            full = _ln_f32(nat, a["x"], res, xscale, a["gamma"], a["beta"], True, True, True)
            s, y, img = full["s"][:n_rows], full["y"][:n_rows], full["img"][:n_rows]
            case = (rows, D, regime, res is not None, xscale is not None)
            got = {"s": C.f32_sum_ratio(s, a["x"], res, xscale)}
            got.update(C.forward_ratios(s, a["gamma"], a["beta"], y, None, None, C.F32_DEPTH, rsqrt_u=4))
            _note(got, "f32", case)
            rec = img[:, :D].double() + img[:, D:].double()
            assert float(((rec - y.double()).abs() - 2.0 ** -16 * y.double().abs()).max()) <= 0.0, case
            for want_s, want_y, want_img in ((False, True, True), (True, True, False), (False, True, False),
                                             (True, False, True), (False, False, True)):
                part = _ln_f32(nat, a["x"], res, xscale, a["gamma"], a["beta"], want_s, want_y, want_img)
                for name in ("s", "y", "img"):
                    assert part[name] is None or _same_bits(part[name], full[name]), (case, name)


# ------------------------------------------------------------------------------------------------------------------
# no rows: nothing is launched, nothing written
# ------------------------------------------------------------------------------------------------------------------
def test_no_rows_writes_nothing(nat):
    a = _inputs(3, 192, "plain")
    p, L, st = nat._ptr, nat.lib(), nat._stream()
    y, s, mean, rstd, dg = _bf16(3, 192), _bf16(3, 192), _f32(3), _f32(3), _f32(192)
    assert L.basd_layernorm_fwd_bf16(p(a["x"]), p(a["gamma"]), p(a["beta"]), 0, 192, C.EPS, p(y), p(mean), p(rstd), st) == 0
    assert L.basd_add_layernorm_fwd_bf16(p(a["x"]), p(a["r"]), p(a["gamma"]), p(a["beta"]), 0, 192, C.EPS, p(s), p(y),
                                         p(mean), p(rstd), None, 1, st) == 0
    assert L.basd_layernorm_bwd_bf16(p(a["dy"]), p(a["x"]), p(a["gamma"]), p(mean), p(rstd), 0, 192, p(y), p(dg), p(dg),
                                     None, p(s), None, 1, st) == 0
    torch.cuda.synchronize()
    _check_guards({"y": y, "s": s, "mean": mean, "rstd": rstd, "dg": dg}, 0, written=False)

"""Bookkeeping of the LayerNorm cases (tests/test_layernorm_family_gpu.py), without a GPU.

tests/_ln_cases.py mirrors the launchers of csrc/layernorm.hip (the configuration (G, NCH, U) from D / 8, ``ln_grid``,
the grid-stride loops).  These tests pin the reason every GPU case is in the list -- which configuration it launches,
whether its last chunk column is full, how many loop trips its busiest row group makes, where a row group holds dead
rows -- so the list cannot drift off those paths.  They also run the emulation of tests/_emul.py (what every CPU step
test treats as the kernels) through the very bound functions the GPU test applies to the kernels: the inputs and the
bounds are sane without the kernel.  And the C entries' refusals, which return before anything touches a GPU."""
import ctypes

import pytest
import torch

from tests import _emul
from tests import _ln_cases as C


# ------------------------------------------------------------------------------------------------------------------
# the paths the cases claim
# ------------------------------------------------------------------------------------------------------------------
def _width_launches(which):
    fn = C.forward if which == "forward" else C.backward
    return [fn(C.case_rows(rows, regime), D) for rows, D, regime in C.WIDTH_CASES]


def test_configuration_boundaries():
    assert [C.config(D) for D in (8, 256, 264, 512, 520, 1024, 1032, 1536, 1544, 2048)] == [
        (32, 1, 4), (32, 1, 4), (64, 1, 4), (64, 1, 4), (64, 2, 2), (64, 2, 2), (64, 3, 1), (64, 3, 1), (64, 4, 1),
        (64, 4, 1)]
    assert {C.config(D) for D in C.WIDTHS} == set(C.CONFIGS)
    # the backward's dynamic LDS, 4 waves x 2 x D floats, is exactly 64 KiB at the widest row
    assert 4 * 2 * max(C.WIDTHS) * 4 == 64 * 1024


def test_every_configuration_has_a_full_and_a_partial_last_chunk_column():
    full = {C.config(D): D for D in C.WIDTHS if C.forward(1, D).full_last_column}
    partial = {C.config(D) for D in C.WIDTHS if not C.forward(1, D).full_last_column}
    assert full == {(32, 1, 4): 256, (64, 1, 4): 512, (64, 2, 2): 1024, (64, 3, 1): 1536, (64, 4, 1): 2048}
    assert partial == set(C.CONFIGS)
    for D in C.WIDTHS:
        G, NCH, _U = C.config(D)
        assert (NCH - 1) * G < D // 8 <= NCH * G                     # the last chunk column holds at least one chunk


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_every_configuration_makes_one_trip_and_several(which):
    one = {la.config for la in _width_launches(which) if la.trips == 1}
    wrap_cases = C.FWD_WRAP if which == "forward" else C.BWD_WRAP
    fn = C.forward if which == "forward" else C.backward
    wrapped = {fn(rows, D).config: fn(rows, D) for rows, D in wrap_cases}
    assert one == set(C.CONFIGS) == set(wrapped)
    for la in wrapped.values():
        assert la.trips >= 2 and la.grid == (C.FWD_CAP if which == "forward" else C.BWD_CAP)
    if which == "forward":
        # below the cap the forward's grid covers the rows in ONE trip: only a wrap case can make a second one, and
        # each wrap case is the cap's worth of rows plus an odd remainder smaller than one workgroup
        assert all(la.trips == 1 for la in _width_launches(which))
        for rows, D in C.FWD_WRAP:
            G, _NCH, U = C.config(D)
            rem = rows - C.FWD_CAP * 4 * (64 // G) * U
            assert 0 < rem and rem % 2 == 1 and rem <= 33 and C.forward(rows, D).trips == 2
            assert C.forward(rows - rem, D).trips == 1
        # a teacher at D = 768 wraps from 16385 rows on
        assert C.forward(16384, 768).trips == 1 and C.forward(16385, 768).trips == 2
    else:
        # the backward's grid assumes 4 rows per group and trip, the narrow-U kernels walk 2 or 1: they make 2 and 4
        # trips below the cap already (rows 37 and 131), one trip only where one workgroup's first rows suffice
        by_cfg = {}
        for la in _width_launches(which):
            by_cfg.setdefault(la.config, set()).add(la.trips)
        assert by_cfg[(32, 1, 4)] == {1} and by_cfg[(64, 1, 4)] == {1}
        assert by_cfg[(64, 2, 2)] == {1, 2} and by_cfg[(64, 3, 1)] == {1, 2, 4} == by_cfg[(64, 4, 1)]
        for rows, D in C.BWD_WRAP:
            G, _NCH, U = C.config(D)
            rem = rows - C.BWD_CAP * 4 * (64 // G) * 4
            assert 0 < rem <= 5 and rem % 2 == 1 and D == min(d for d in C.WIDTHS if C.config(d) == C.config(D))
            assert C.backward(rows, D).trips == 4 // U + 1 and C.backward(rows, D).t == 4 + U


def test_backward_single_trip_cases_have_a_ragged_tail():
    """a live row group whose rows u > 0 are dead: every configuration with U > 1 has a single-trip case with one (at
    U = 1 a group holds one row per trip: there is no u > 0)"""
    ragged = {la.config for la in _width_launches("backward") if la.trips == 1 and la.ragged_tail}
    assert ragged == {cfg for cfg in C.CONFIGS if cfg[2] > 1}
    ragged_fwd = {la.config for la in _width_launches("forward") if la.ragged_tail}
    assert ragged_fwd == ragged
    assert not any(la.ragged_tail for la in _width_launches("backward") if la.config[2] == 1)


def test_odd_row_counts_leave_the_second_row_group_of_a_wave_dead():
    dead = [(rows, D, regime) for rows, D, regime in C.WIDTH_CASES
            if C.forward(C.case_rows(rows, regime), D).dead_second_group]
    assert {D for _r, D, _g in dead} == {8, 192, 248, 256}                    # every G = 32 width
    assert {C.case_rows(r, g) for r, _D, g in dead} == {1, 3, 7, 37, 131}
    assert all(C.forward(rows, D).dead_second_group and C.backward(rows, D).dead_second_group
               for rows, D in C.FWD_WRAP[:2] + C.BWD_WRAP[:1])


_WALKED = sorted({(C.case_rows(rows, regime), D) for rows, D, regime in C.WIDTH_CASES if D in (8, 520, 1544)}
                 | set(C.FWD_WRAP) | set(C.BWD_WRAP))


@pytest.mark.parametrize("case", _WALKED, ids=C.case_id)
def test_the_loops_visit_every_row_once(case):
    """the mirror's closed forms against the loops themselves, walked group by group"""
    rows, D = case
    for which, fn in (("forward", C.forward), ("backward", C.backward)):
        la = fn(rows, D)
        G, _NCH, U = la.config
        seen = C.rows_visited(rows, D, which)
        assert sorted(seen) == list(range(rows)) and set(seen.values()) == {1}
        wstride = la.grid * 4 * (64 // G)
        period = wstride * U
        assert la.trips == len(range(0, rows, period))
        # a ragged tail: a group whose first row of a trip is live and whose last is not
        ragged = any(r0 + (U - 1) * wstride >= rows for t0 in range(0, rows, period)
                     for r0 in range(t0, min(t0 + wstride, rows)))
        assert ragged == la.ragged_tail


def test_inputs_are_what_the_cases_say():
    for D in (8, 192, 1544):
        a = C.inputs(37, D, "trained")
        x = a["x"].float()
        cols = C.spike_columns(D)
        assert len(cols) == max(1, D // 96) and x.shape == (42, D) and a["x"].dtype == torch.bfloat16
        rest = torch.ones(D, dtype=torch.bool)
        rest[cols] = False
        assert float(x[:37][:, cols].min()) > 75 and float(x[:37][:, rest].max()) < 8
        assert abs(float(x[41].mean()) - C.OFFSET_ROW) < 1 and 0.3 < float(x[41].std()) < 1.5
        for row, v in zip(x[37:41], C.CONSTANT_ROWS):
            assert bool((row == row[0]).all()) and abs(float(row[0]) - v) <= 2.0 ** -8 * abs(v)
        assert torch.equal(a["x"], C.inputs(37, D, "trained")["x"])              # seeded
        assert C.inputs(37, D, "plain")["x"].shape == (37, D)
    a = C.scaled_add_inputs(131, 264)
    for t in (a["x"], a["r"]):
        assert t.dtype == torch.bfloat16 and 2.0 ** -6 <= float(t.float().abs().min())
        assert float(t.float().abs().max()) <= 2.0 ** 6 and bool((t.float() < 0).any()) and bool((t.float() > 0).any())
    for rows in (1, 3, 37, 131):
        for rps in C.scale_row_counts(rows):
            sc = C.row_scales(rows, rps)
            assert len(sc) == -(-rows // rps) and set(sc.tolist()) <= set(torch.tensor(C.SCALES).float().tolist())
            assert len(set(sc.tolist())) == min(3, len(sc))
    assert C.scale_row_counts(131) == [1, 7, 43] and C.SCALES[2] == float(torch.tensor(1 / 0.7).float())


def test_scaled_add_is_exact_in_fp64():
    """the condition of the no-tolerance check of sum_out: r + sc x needs at most 53 bits"""
    a = C.scaled_add_inputs(131, 264)
    x, r = a["x"].double(), a["r"].double()
    for sc in C.SCALES:
        # the smallest bit that can be set is 2^-6 2^-7 2^-23 (x's last bit times the scale's), the sums stay below 2^8
        assert 2.0 ** 8 / (2.0 ** -6 * 2.0 ** -7 * 2.0 ** -23) < 2.0 ** 53 and float((r.abs() + sc * x.abs()).max()) < 2.0 ** 8
        s = r + sc * x
        # the fp64 sum is exact: what was rounded off (two-sum) is zero
        t = s - r
        assert bool(((r - (s - t)) + (sc * x - t) == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# the emulation inside the bounds the kernels get
# ------------------------------------------------------------------------------------------------------------------
_WORST = {}


def _note(name, value, case):
    if value > _WORST.get(name, (0.0, None))[0]:
        _WORST[name] = (value, case)


@pytest.mark.parametrize("D", C.WIDTHS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_emulated_forward_is_inside_the_bounds(D, regime):
    n = C.depth(C.config(D)[1])
    for rows in C.ROWS:
        a = C.inputs(rows, D, regime)
        y, mean, rstd = _emul.layernorm_fwd(a["x"], a["gamma"], a["beta"], C.EPS)
        got = C.forward_ratios(a["x"], a["gamma"], a["beta"], y, mean, rstd, n)
        for name, v in got.items():
            _note("fwd " + name, v, (rows, D, regime))
            assert v <= 1.0, (name, rows, D, regime, v)
        s, y2, mean2, rstd2 = _emul.add_layernorm_fwd(a["x"], a["r"], a["gamma"], a["beta"], C.EPS, want_stats=True)
        assert torch.equal(s, a["x"] + a["r"])
        assert torch.equal(y2, _emul.layernorm_fwd(s, a["gamma"], a["beta"], C.EPS)[0])
        for name, v in C.forward_ratios(s, a["gamma"], a["beta"], y2, mean2, rstd2, n).items():
            assert v <= 1.0, ("add", name, rows, D, regime, v)


def test_emulated_scaled_add_is_exact():
    for rows, D in ((37, 8), (131, 264)):
        a = C.scaled_add_inputs(rows, D)
        for rps in C.scale_row_counts(rows):
            sc = C.row_scales(rows, rps)
            per_row = sc.repeat_interleave(rps)[:rows]
            s, _y = _emul.add_layernorm_fwd(a["x"], a["r"], a["gamma"], a["beta"], C.EPS, row_scale=per_row)
            p = per_row.double().view(-1, 1) * a["x"].double()
            exact = a["r"].double() + p
            # the emulation rounds the product before the sum (2 u on the operands' magnitudes): where that matters it
            # may differ from bf16(fp32(exact)) by a bf16 ulp; the kernel's fma may not
            # (tests/test_layernorm_family_gpu.py)
            assert float((s != exact.float().bfloat16()).float().mean()) < 1e-2
            bound = C.UBF16 * exact.abs() + (1 + C.UBF16) * 2 * C.U32 * (a["r"].double().abs() + p.abs())
            assert C.ratio((s.double() - exact).abs(), bound) <= 1.0


@pytest.mark.parametrize("D", C.WIDTHS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_emulated_backward_is_inside_the_bounds(D, regime):
    for rows in C.ROWS:
        a = C.inputs(rows, D, regime)
        n_rows = C.case_rows(rows, regime)
        la = C.backward(n_rows, D)
        _y, mean, rstd = _emul.layernorm_fwd(a["x"], a["gamma"], a["beta"], C.EPS)
        if rows == 37:                             # the entry as the function of mean / rstd it is
            g = torch.Generator().manual_seed(D)
            mean = mean * (1 + 0.03 * torch.randn(n_rows, generator=g))
            rstd = rstd * (1 + 0.03 * torch.randn(n_rows, generator=g))
        rps = max(1, n_rows // 3)
        per_row = C.row_scales(n_rows, rps).repeat_interleave(rps)[:n_rows]
        g = torch.Generator().manual_seed(D + 1)
        pre_g, pre_b = torch.randn(D, generator=g), torch.randn(D, generator=g)
        dgamma, dbeta = pre_g.clone(), pre_b.clone()
        dx, dbranch = _emul.layernorm_bwd(a["dy"], a["x"], a["gamma"], mean, rstd, dgamma, dbeta, dres=a["dres"],
                                          row_scale=per_row, want_branch=True)
        got = C.backward_ratios(a["dy"], a["x"], a["gamma"], mean, rstd, dx, la, dres=a["dres"], dbranch=dbranch,
                                scale_of_row=per_row, dgamma=dgamma, dbeta=dbeta, prefill_gamma=pre_g,
                                prefill_beta=pre_b)
        assert set(got) == {"dx", "dbranch", "dgamma", "dbeta"}
        for name, v in got.items():
            _note("bwd " + name, v, (rows, D, regime))
            assert v <= 1.0, (name, rows, D, regime, v)


def _one_pass_rstd(x):
    """the variance as mean(x^2) - mean^2 in fp32, the mean as sum * fl(1 / D) like the kernel: what the two-pass
    kernel must not be mistaken for"""
    xf = x.float()
    inv_d = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(x.shape[1]), dtype=torch.float32)
    mean = xf.sum(-1) * inv_d
    var = (xf * xf).sum(-1) * inv_d - mean * mean
    return mean, torch.rsqrt(var + torch.tensor(C.EPS, dtype=torch.float32))


def test_the_rstd_bound_rejects_a_one_pass_variance_on_the_trained_regime():
    rejected = []
    for D in C.WIDTHS:
        a = C.inputs(37, D, "trained")
        n = C.depth(C.config(D)[1])
        mu, var, rs, _xh, _y = C.forward_reference(a["x"], a["gamma"], a["beta"])
        mean, rstd = _one_pass_rstd(a["x"])
        rho = C.rstd_rel_bound(var, C.mean_bound(a["x"], n), n)
        bad = ~((rstd.double().view(-1, 1) / rs - 1.0).abs() <= rho)             # a NaN (negative variance) is rejected
        if bool(bad.any()):
            rejected.append(D)
        # the two-pass emulation passes on the same rows
        _y2, _m2, rstd2 = _emul.layernorm_fwd(a["x"], a["gamma"], a["beta"], C.EPS)
        assert bool(((rstd2.double().view(-1, 1) / rs - 1.0).abs() <= rho).all())
    print("one-pass variance rejected at D =", rejected)
    assert len(rejected) >= len(C.WIDTHS) - 2, rejected


def test_report_emulation_ratios():
    """runs after the two bound tests above: the largest err / bound of the emulation, for the record (pytest -s)"""
    for name, (v, case) in sorted(_WORST.items()):
        print(f"ln-emul {name}: {v:.4f} at {case}")


# ------------------------------------------------------------------------------------------------------------------
# refusals: every check below returns before a kernel is launched, so no GPU is needed
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def entries():
    import basd_amd._native as native
    if not __import__("os").path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


_NULL = ctypes.c_void_p(0)
BASD_OK, BASD_ERR_SHAPE = 0, 1


def _host(n, dtype):
    """a host buffer behind a fake pointer: nothing may be read or written through it"""
    t = torch.full((n,), -7, dtype=dtype)
    return t, ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("D", [0, 4, 12, 2056])
def test_bf16_entries_refuse_unsupported_widths(entries, D):
    t, p = _host(64, torch.float32)
    assert entries.basd_layernorm_fwd_bf16(p, p, p, 3, D, C.EPS, p, p, p, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_add_layernorm_fwd_bf16(p, p, p, p, 3, D, C.EPS, p, p, p, p, _NULL, 1, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_layernorm_bwd_bf16(p, p, p, p, p, 3, D, p, p, p, _NULL, _NULL, _NULL, 1, _NULL) == BASD_ERR_SHAPE
    assert str(D).encode() in entries.basd_last_error()
    assert bool((t == -7).all())


@pytest.mark.parametrize("D", [0, 2, 6, 2052])
def test_fp32_entry_refuses_unsupported_widths(entries, D):
    t, p = _host(64, torch.float32)
    assert entries.basd_add_layernorm_fwd_f32(p, p, p, p, p, 3, D, C.EPS, p, p, p, _NULL) == BASD_ERR_SHAPE
    assert bool((t == -7).all())


def test_no_rows_is_ok_and_writes_nothing(entries):
    t, p = _host(4096, torch.float32)
    for rows in (0, -1):
        assert entries.basd_layernorm_fwd_bf16(p, p, p, rows, 192, C.EPS, p, p, p, _NULL) == BASD_OK
        assert entries.basd_add_layernorm_fwd_bf16(p, p, p, p, rows, 192, C.EPS, p, p, p, p, p, 1, _NULL) == BASD_OK
        assert entries.basd_layernorm_bwd_bf16(p, p, p, p, p, rows, 192, p, p, p, p, p, p, 1, _NULL) == BASD_OK
        assert entries.basd_add_layernorm_fwd_f32(p, p, p, p, p, rows, 192, C.EPS, p, p, p, _NULL) == BASD_OK
    assert bool((t == -7).all())


def test_fused_entry_refuses_null_operands_and_bad_rows_per_scale(entries):
    t, p = _host(4096, torch.float32)
    add = entries.basd_add_layernorm_fwd_bf16
    assert add(p, _NULL, p, p, 3, 192, C.EPS, p, p, p, p, _NULL, 1, _NULL) == BASD_ERR_SHAPE       # no residual
    assert add(p, p, p, p, 3, 192, C.EPS, _NULL, p, p, p, _NULL, 1, _NULL) == BASD_ERR_SHAPE       # no sum_out
    for rps in (0, -3):
        assert add(p, p, p, p, 3, 192, C.EPS, p, p, p, p, p, rps, _NULL) == BASD_ERR_SHAPE         # row_scale given
    assert b"rows_per_scale" in entries.basd_last_error()
    # the fp32 entry needs an output
    assert entries.basd_add_layernorm_fwd_f32(p, p, p, p, p, 3, 192, C.EPS, p, _NULL, _NULL, _NULL) == BASD_ERR_SHAPE
    assert bool((t == -7).all())

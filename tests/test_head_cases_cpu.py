"""Bookkeeping and bounds of the head / selector-weight / optimizer cases (tests/test_head_kernels_gpu.py), without a GPU.

tests/_head_cases.py mirrors the host launch arithmetic of csrc/ce_uwso.hip, csrc/selector.hip (angle weights, their
backward, the health-word flag) and csrc/optim.hip.  These tests pin (1) that the case lists reach every regime the
mirror names -- for each strided loop lanes without a trip, exactly one trip, at least two; for each grid cap below, at
and above; for each switch both sides -- so a changed shape that leaves its regime fails here; (2) that an fp32 torch
chain of each formula stays within HALF of the bounds the kernels get, on every case: the bounds are reachable by a
correct fp32 implementation; (3) that the fp64 references agree with a second, independent writing of the formulas
(tests/_emul.ce_uwso, tests/test_optim._scalar_trace)."""
import pytest
import torch

from tests import _emul
from tests import _head_cases as H

_WORST = {}


def _note(family, got, where):
    for name, v in got.items():
        if v >= _WORST.get((family, name), (-1.0, None))[0]:
            _WORST[(family, name)] = (v, where)
        assert v <= 0.5, (family, where, name, v)


# ----------------------------------------------------------------------------------------------------------------------
# (1) the regimes the cases claim
# ----------------------------------------------------------------------------------------------------------------------
def _trip_regimes(launches, lanes_idle="idle_lanes", trips="trips"):
    got = set()
    for la in launches:
        t = getattr(la, trips)
        if getattr(la, lanes_idle, 0):
            got.add("idle")
        got.add("one" if t == 1 else "many")
        if t == 1 and not getattr(la, lanes_idle, 0):
            got.add("exact")
    return got


def test_ce_cases_reach_every_regime():
    las = {c: H.ce_launch(c.B, c.C) for c in H.CE_CASES}
    assert {la.class_trips for la in las.values()} >= {1, 2, 4}
    assert any(la.idle_lanes for la in las.values()) and H.ce_launch(5, 256).idle_lanes == 0 == H.ce_launch(5, 1000).idle_lanes
    assert H.ce_launch(5, 256).class_trips == 1 and H.ce_launch(5, 257).class_trips == 2       # one class in trip two
    assert {H.ce_launch(B, 10).row_trips for B in H.CE_BATCHES} == {1, 2, 3}
    assert [H.ce_launch(B, 10).row_trips for B in (255, 256, 257)] == [1, 1, 2]
    assert {la.cap for la in las.values()} == {"below", "at", "above"}
    at, above = (H.ce_launch(c.B, c.C) for c in H.CE_CAP_CASES)
    assert (at.grid, at.scale_trips, at.last_trip) == (1024, 8, 1024 * 256)
    assert (above.grid, above.scale_trips, above.last_trip) == (1024, 9, 1024)                 # one more trip: one row
    assert H.ce_launch(5, 1).grid == 1 and H.ce_launch(5, 1).scale_trips == 1 and H.ce_launch(5, 1).last_trip == 5
    assert {c.target for c in las} == {"hard", "soft", "sums"} and {c.smoothing for c in las} == {0.0, 0.1}
    assert {c.geo for c in las} == set(H.CE_GEO) and {c.margin for c in las} == {0, 30, 100}
    assert {c.C for c in las if c.B == 5} == set(H.CE_CLASSES) and {c.B for c in las if c.C == 10} >= set(H.CE_BATCHES)
    # the eps clamps: both sides of each, read from the fp64 reference
    seen = set()
    for c in [k for k in H.CE_CASES if k.B * k.C < 10000 and k.geo is not None]:
        logits, soft, labels, geo = H.ce_inputs(c)
        seen.add(H.CERef(logits, soft, labels, c.smoothing, geo).clamped)
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    logits, soft, labels, _geo = H.ce_inputs(H.CE_CASES[0])
    assert int(labels[0]) == 0 and int(labels[1]) == H.CE_CASES[0].C - 1
    _l, soft, _n, _g = H.ce_inputs(H.CE_CASES[[c.target for c in H.CE_CASES].index("sums")])
    assert torch.allclose(soft.sum(1), torch.tensor([1.0, 0.5, 2.0, 1.0])) and int((soft[3] != 0).sum()) == 1


def test_angle_weight_cases_reach_every_regime():
    las = [H.aw_launch(c.L, c.D) for c in H.AW_CASES]
    assert _trip_regimes(las) == {"idle", "one", "exact", "many"}
    assert [H.aw_launch(3, D).trips for D in (255, 256, 257, 513)] == [1, 1, 2, 3] and H.aw_launch(3, 513).last_trip == 1
    assert {c.L for c in H.AW_CASES} >= {1, 2, 63, H.AW_MAX_L} and {c.E for c in H.AW_CASES} >= {1, 3}
    assert {c.D for c in H.AW_CASES} >= set(H.AW_WIDTHS) and {c.unnorm for c in H.AW_CASES} == {True, False}
    assert any(c.D > 256 and c.D % 64 for c in H.AW_CASES)
    lts = {v for c in H.AW_CASES if c.lt for v in c.lt}
    assert {19.5, 20.0} <= {v for v in lts if not v > 20.0} and {20.5, 30.0} <= {v for v in lts if v > 20.0}
    assert any(10.0 < v < 16.0 for v in lts)                      # where softplus(x) != x in fp32
    for un in (True, False):
        case = next(c for c in H.AW_CASES if c.sig == "edges" and c.unnorm == un and c.ranks == "mixed")
        sig, sw, lt = H.aw_inputs(case)
        ref = H.AWRef(sig, sw, lt, un)
        col = {v: i for i, v in enumerate(H.AW_EDGES)}
        ok = ref.ok[0, 1]                                          # layer 1 has full rank
        floor, other = (H.AW_FLOOR_U, H.AW_FLOOR_N) if un else (H.AW_FLOOR_N, H.AW_FLOOR_U)
        assert bool(ok[col[1.0 - H.EPS32]]) and not bool(ok[col[H.AW_EDGES[1]]]) and not bool(ok[col[1.0]])
        assert not bool(ok[col[floor]]) and bool(ok[col[H._next_up(floor)]]) and not bool(ok[col[0.0]])
        assert bool(ok[col[other]]) == (not un) and bool(ok[col[H._next_up(other)]]) == (not un)
        assert float(ref.coef[0, 1, col[1.0 - H.EPS32]]) != 0.0 and float(ref.coef[0, 1, col[H._next_up(floor)]]) != 0.0
        assert bool((ref.coef[~ref.ok] == 0).all())
        assert bool(((sw != 0).sum(1) == 1)[0]) and int((sw != 0).sum(1)[1]) == case.D      # rank 1, full rank
    case = next(c for c in H.AW_CASES if c.ranks == "rank0")
    sig, sw, lt = H.aw_inputs(case)
    ref = H.AWRef(sig, sw, lt, case.unnorm)
    assert float(sw[1].abs().sum()) == 0.0
    assert bool(torch.isnan(ref.d2[:, 1]).all()) and not bool(torch.isnan(ref.d2[:, [0, 2]]).any())
    assert bool(torch.isnan(ref.w).all()) and torch.equal(torch.isnan(ref.coef[:, 1]), ref.ok[:, 1])
    assert not bool(torch.isnan(ref.coef[:, [0, 2]]).any())


def test_angle_weight_bwd_cases_reach_every_regime():
    las = [H.ab_launch(c.E, c.L, c.D, c.Ds) for c in H.AB_CASES]
    assert _trip_regimes(las, trips="seed_trips") == {"idle", "one", "exact", "many"}
    assert [H.ab_launch(2, 3, D, 24).seed_trips for D in (255, 256, 257, 320)] == [1, 1, 2, 2]
    sym = {c.Ds: H.ab_launch(c.E, c.L, c.D, c.Ds) for c in H.AB_CASES if c.D == 48}
    assert {ds: (la.sym_blocks, la.sym_last) for ds, la in sym.items()} == {
        1: (1, 1), 16: (1, 256), 17: (2, 33), 80: (25, 256), 24: (3, 64)}
    assert {c.L for c in H.AB_CASES} >= {1, H.AW_MAX_L} and {c.gpo for c in H.AB_CASES} == {True, False}
    lts = {v for c in H.AB_CASES for v in c.lt}
    assert any(v > 20.0 for v in lts) and any(v <= 20.0 for v in lts)
    assert H.ab_ties(320) == [(0, 1), (318, 319), (255, 256)] and H.ab_ties(48) == [(0, 1), (46, 47)] and H.ab_ties(1) == []
    for c in H.AB_CASES:
        ref = H.ABRef(**H.ab_inputs(c))
        assert ref.ties == 2 * c.E * len(H.ab_ties(c.D)), c                  # tie and no tie, exactly where listed
        assert c.D == 1 or ref.min_gap >= H.AB_MIN_GAP, (c, ref.min_gap)
    assert any(H.ab_ties(c.D) for c in H.AB_CASES) and any(not H.ab_ties(c.D) for c in H.AB_CASES)


def test_workspace_mirror_is_the_entry(entries):
    for e, d, ds in [(c.E, c.D, c.Ds) for c in H.AB_CASES] + [(4, 192, 192), (1, 768, 1280)]:
        assert H.ab_workspace_bytes(e, d, ds) == int(entries.basd_angle_weights_bwd_workspace_bytes(e, d, ds))
        # what the entry carves out behind a base 8 bytes off a 256-byte boundary (248 bytes of padding) fits
        assert 248 + e * (3 * d * d + d * ds + ds * ds) * 8 <= H.ab_workspace_bytes(e, d, ds)


def test_flag_cases_reach_every_regime():
    las = {n: H.flag_launch(n) for n in H.FLAG_SIZES}
    assert {la.cap for la in las.values()} == {"below", "at", "above"}
    assert (las[65536].grid, las[65536].trips, las[65536].last_trip) == (256, 1, 65536)
    assert (las[65537].grid, las[65537].trips, las[65537].last_trip) == (256, 2, 1)
    assert las[200001].trips == 4 and [las[n].grid for n in (1, 255, 256, 257)] == [1, 1, 1, 2]
    assert H.flag_positions(65537) == [0, 65535, 65536] and H.flag_positions(65536) == [0, 65535] and H.flag_positions(1) == [0]
    v = H.flag_clean(64)
    assert not bool((~(v <= H.FLAG_TOL)).any()) and float(v[0]) == H.FLAG_TOL and float(v[1]) == -float("inf")
    assert all(not (val <= H.FLAG_TOL) for val, _bit in H.FLAG_KINDS.values())
    assert all(bit & H.STATUS_PRE == 0 for _v, bit in H.FLAG_KINDS.values())
    assert H.FLAG_KINDS["above"][0] - H.FLAG_TOL == 2.0 ** -52


def test_optimizer_cases_reach_every_regime():
    ad = {n: H.ad_launch(n) for n in H.AD_SIZES}
    assert {la.cap for la in ad.values()} == {"below", "at", "above"} and {la.tail for la in ad.values()} == {0, 1, 2, 3}
    assert (ad[1].grid, ad[1].trips, ad[1].tail) == (1, 0, 1) and (ad[4].trips, ad[4].last_trip, ad[4].tail) == (1, 1, 0)
    assert (ad[H.AD_PASS].grid, ad[H.AD_PASS].trips, ad[H.AD_PASS].last_trip) == (2048, 1, 2048 * 256)
    assert (ad[H.AD_PASS - 1].trips, ad[H.AD_PASS - 1].tail) == (1, 3) and (ad[H.AD_PASS + 1].trips, ad[H.AD_PASS + 1].tail) == (1, 1)
    assert (ad[H.AD_PASS + 1027].trips, ad[H.AD_PASS + 1027].last_trip, ad[H.AD_PASS + 1027].tail) == (2, 256, 3)
    assert ad[5_000_003].trips == 3 and (ad[1023].last_trip, ad[1023].tail) == (255, 3) and (ad[1027].last_trip, ad[1027].tail) == (256, 3)
    assert {(c.ckp1, c.bc2, c.wd) for c in H.AD_CASES if c.n == 1027} == set(H.AD_SCALARS) and len(H.AD_SCALARS) == 8
    assert {c.n for c in H.AD_CASES} == set(H.AD_SIZES)
    lp = {n: H.lp_launch(n) for n in H.LP_SIZES}
    assert {la.cap for la in lp.values()} == {"below", "at", "above"}
    assert [lp[n].grid for n in (1, 255, 256, 257)] == [1, 1, 1, 2]
    assert (lp[H.LP_PASS].trips, lp[H.LP_PASS + 1].trips, lp[H.LP_PASS + 1].last_trip, lp[1_300_001].trips) == (1, 2, 1, 3)
    assert {c.w for c in H.LP_CASES} == set(H.LP_WEIGHTS)
    y, g, z, v = H.ad_inputs(H.ADCase(H.AD_PASS + 1027, 0.25, 0.3, 0.05))
    assert H.ad_special_runs(H.AD_PASS + 1027) == [0, H.AD_PASS - 4, H.AD_PASS + 4, H.AD_PASS + 1019]
    for a in H.ad_special_runs(H.AD_PASS + 1027):
        assert (float(g[a + 1]), float(v[a + 1])) == (0.0, 0.0) and float(g[a + 2]) == 0.0 and float(v[a + 2]) > 0.0
        assert abs(float(g[a + 3])) == pytest.approx(1e-20) and float(v[a + 3]) == 0.0 and float(g[a + 4]) == 1e3
    sig = H.index_signature(H.AD_PASS + 1027)
    assert bool((sig[1:] != sig[:-1]).all()) and bool((sig[H.AD_PASS:] != sig[:1027]).all())
    assert [float(g[i]) for i in range(3)] != [0.0] * 3 and float(H.ad_inputs(H.ADCase(3, 1.0, 0.3, 0.0))[1][1]) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# (2) an fp32 torch chain of each formula within half of the bounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.CE_CASES, ids=H.ce_id)
def test_ce_fp32_chain_is_inside_half_the_bounds(case):
    logits, soft, labels, geo = H.ce_inputs(case)
    ref = H.CERef(logits, soft, labels, case.smoothing, geo)
    _note("ce", ref.ratios(*H.ce_chain32(logits, soft, labels, case.smoothing, geo)), H.ce_id(case))


@pytest.mark.parametrize("case", H.AW_CASES, ids=H.aw_id)
def test_angle_weights_fp32_chain_is_inside_half_the_bounds(case):
    sig, sw, lt = H.aw_inputs(case)
    ref = H.AWRef(sig, sw, lt, case.unnorm)
    _note("angle_weights", ref.ratios(*_emul.angle_weights(sig, sw, lt, case.unnorm), nan_ok=case.ranks == "rank0"),
          H.aw_id(case))


@pytest.mark.parametrize("case", H.AB_CASES, ids=H.ab_id)
def test_angle_weights_bwd_fp32_chain_is_inside_half_the_bounds(case):
    inp = H.ab_inputs(case)
    _note("angle_weights_bwd", H.ABRef(**inp).ratios(*H.ab_chain32(**inp)), H.ab_id(case))


@pytest.mark.parametrize("case", H.AD_CASES, ids=H.ad_id)
def test_adamw_fp32_chain_is_inside_half_the_bounds(case):
    y, g, z, v = H.ad_inputs(case)
    ref = H.ADRef(y, g, z, v, case)
    g0 = g.clone()
    _emul.sf_adamw_step(y, g, z, v, **H.ad_kwargs(case))
    assert torch.equal(g, g0)
    _note("sf_adamw", ref.ratios(y, z, v), H.ad_id(case))


@pytest.mark.parametrize("case", H.LP_CASES, ids=H.lp_id)
def test_lerp_fp32_chain_is_inside_half_the_bounds(case):
    y, z = H.lp_inputs(case)
    ref = H.LPRef(y, z, case.w)
    _emul.lerp_(y, z, case.w)
    _note("lerp", ref.ratios(y), H.lp_id(case))


def test_report_chain_ratios():
    """runs after the bound tests above: the largest err / bound of the fp32 chains per output (pytest -s)"""
    for (family, name), (v, where) in sorted(_WORST.items()):
        print(f"head-chain {family} {name}: {v:.4f} at {where}")


def test_the_bounds_reject_what_the_cases_are_there_for():
    """a dropped element, a tsum of 1 on rows that do not sum to 1, a doubled update"""
    case = next(c for c in H.CE_CASES if c.target == "sums")
    logits, soft, labels, geo = H.ce_inputs(case)
    ref = H.CERef(logits, soft, labels, case.smoothing, geo)
    row, dl, out4 = H.ce_chain32(logits, soft, labels, case.smoothing, geo)
    t1 = H.ce_chain32(logits, soft / soft.sum(1, keepdim=True), labels, case.smoothing, geo)[1]
    assert ref.ratios(row, t1, out4)["dlogits"] > 1.0
    dl[-1, -1] = 0.0
    assert ref.ratios(row, dl, out4)["dlogits"] > 1.0
    case = H.ADCase(1027, 0.25, 0.3, 0.05)
    y, g, z, v = H.ad_inputs(case)
    ref = H.ADRef(y, g, z, v, case)
    v0 = v.clone()
    _emul.sf_adamw_step(y, g, z, v, **H.ad_kwargs(case))
    skipped, twice = v.clone(), v.clone()
    skipped[1026] = v0[1026]
    twice[100] = 0.999 * v[100] + 0.001 * g[100] * g[100]
    assert ref.ratios(y, z, skipped)["v"] > 1.0 and ref.ratios(y, z, twice)["v"] > 1.0


# ----------------------------------------------------------------------------------------------------------------------
# (3) two independent writings of the formulas agree
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in H.CE_CASES if c.B * c.C <= 64000], ids=H.ce_id)
def test_ce_reference_agrees_with_the_emulation(case):
    logits, soft, labels, geo = H.ce_inputs(case)
    ref = H.CERef(logits, soft, labels, case.smoothing, geo)
    out4, dl = _emul.ce_uwso(logits, soft if soft is not None else labels, case.smoothing, geo)
    # the emulation smooths with the double 0.1, the entry (and the reference) with the float: 1.5e-8 relative
    torch.testing.assert_close(out4.double(), ref.out4, rtol=1e-6, atol=1e-12)
    torch.testing.assert_close(dl.double(), ref.dl, rtol=1e-6, atol=1e-9 * float(ref.dl.abs().max()) + H.TINY)


def test_adamw_reference_agrees_with_the_scalar_trace():
    from tests.test_optim import _scalar_trace
    lr, wd = H.AD_HYPER["lr"], 0.05
    for y0, grads in ((0.7, [0.3, 0.1, -0.6, 0.0, 2.0]), (-1.3, [-0.2, 0.4, 0.0, 1e3, -1e-3])):
        y = z = torch.tensor([y0], dtype=torch.float64)
        v = torch.zeros(1, dtype=torch.float64)
        for k, (ty, tz, tv) in enumerate(_scalar_trace(y0, grads, lr=lr, wd=wd)):
            case = H.ADCase(1, 1.0 / (k + 1), 1.0 - 0.999 ** (k + 1), wd)         # constant lr: ckp1 = 1 / (k + 1)
            ref = H.ADRef(y, torch.tensor([grads[k]], dtype=torch.float64), z, v, case)
            y, z, v = ref.y, ref.z, ref.v
            # the reference takes the entry's fp32-rounded scalars, the trace the doubles: 6e-8 relative each
            assert float(y) == pytest.approx(ty, rel=2e-6, abs=1e-9) and float(z) == pytest.approx(tz, rel=2e-6, abs=1e-9)
            assert float(v) == pytest.approx(tv, rel=2e-6, abs=1e-15)


@pytest.fixture(scope="module")
def entries():
    import basd_amd._native as native
    if not __import__("os").path.exists(native.LIB_PATH):
        native.build()
    return native.lib()

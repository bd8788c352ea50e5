"""Bookkeeping of the token-statistics cases (tests/test_token_stats_gpu.py), without a GPU.

tests/_token_stats_cases.py mirrors the launchers of csrc/token_gram.hip and the routing of _native.token_gram.  These
tests pin the reason every GPU case is in the list -- which kernel template it launches, in how many grid-stride trips,
what its last tile and its Gram passes hold -- so the list cannot drift off those paths, and walk the kernels' loops
against the mirror's closed forms.  They run the CPU emulation of each path through the very bound functions the GPU
test applies to the kernels, on every case and regime, and then show that the same bounds REJECT the emulation made
wrong in the ways the cases are there to catch.  And the C entries' refusals, which return before anything touches a
GPU."""
import ctypes

import pytest
import torch

from tests import _token_stats_cases as C


# ------------------------------------------------------------------------------------------------------------------
# the paths the cases claim
# ------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_path_it_is_listed_for():
    for case in C.GENERIC_CASES + C.GENERIC_WRAP:
        la = C.launch_of(case)
        assert la.template == (case.dtype, 10 if case.d_out <= 192 else 17) and la.lds <= 160 * 1024
    for case in C.T128_CASES:
        assert C.launch_of(case).kernel == "t128", case
    for case in C.T256_CASES:
        assert C.launch_of(case).kernel == "t256", case
    assert [C.launch_of(c).kernel for c in C.VIEW_CASES[:2]] == ["t128", "t256"]
    assert [C.launch_of(c).template for c in C.VIEW_CASES[2:]] == [(C.F32, 10), (C.BF16, 10)]
    for case in C.VIEW_CASES:
        b, t = case.view
        assert case.rows == b * (t - 1) and (t - 1) % 16 != 0 and (t * case.d_in) % 8 == 0
    assert C.VIEW_CASES[1].view == (169, 197) and C.VIEW_CASES[1].rows == 33124
    # a direct bf16 call of the generic entry is the generic kernel whatever d_out; through the wrapper it is not
    assert C.route(C.BF16, 200, 32, 192) == ("bf16x3",) and C.route(C.BF16, 200, 32, 208) == ("generic",)
    for case, want in C.ROUTE_CASES:
        assert C.route(case.dtype, case.rows, case.d_in, case.d_out) == want, case
    assert {want for _c, want in C.ROUTE_CASES} == {
        ("bf16x3",), ("generic",), ("wide", "gemm_bf16x3", "centred"), ("wide", "gemm_bf16x3", "splitk"),
        ("wide", "bgemm_f64", "centred"), ("wide", "bgemm_f64", "splitk")}
    assert (40, ("wide", "bgemm_f64", "splitk")) in {(c.d_out, w) for c, w in C.ROUTE_CASES}
    assert 264 in {c.d_out for c, _w in C.ROUTE_CASES}


def test_the_mirror_of_the_wrapper_matches_the_wrapper():
    import basd_amd._native as native
    for m, n, k in ((1792, 272, 128), (1793, 272, 128), (1800, 270, 128), (1800, 272, 96), (1800, 272, 192)):
        assert C.gemm_bf16x3_f32_supported(m, n, k) == native.gemm_bf16x3_f32_supported(m, n, k)
    p = C.projection(C.T128_CASES[-1])
    assert all(torch.equal(a, b) for a, b in zip(C.split3(p), native.split_bf16x3(p)))


def test_every_template_makes_one_trip_and_two():
    templates = {(dt, g) for dt in (C.F32, C.BF16) for g in (10, 17)}
    one = {C.launch_of(c).template for c in C.GENERIC_CASES if C.launch_of(c).trips == 1}
    two = {C.launch_of(c).template: C.launch_of(c) for c in C.GENERIC_WRAP}
    assert one == templates == set(two)
    for la in two.values():
        # workgroups 0 and 1 make two trips; the very last tile (of workgroup 1) is ragged
        assert (la.grid, la.ntiles, la.trips, la.last_valid) == (256, 258, 2, 37)
    for kernel, cases, wrap in (("t128", C.T128_CASES, None), ("t256", C.T256_CASES, C.T256_WRAP_ROWS)):
        las = [C.launch_of(c) for c in cases]
        assert {la.nct for la in las if la.trips == 1} == {2, 4, 8, 12}
        if wrap:
            twice = [la for c, la in zip(cases, las) if c.rows == wrap]
            assert {la.nct for la in twice} == {2, 4, 8, 12}
            assert all((la.grid, la.ntiles, la.trips, la.last) == (256, 258, 2, (41, None)) for la in twice)
    # the 128-row kernel never makes a second trip: its launcher hands over to the 256-row one first
    assert all(C.launch_of(c).trips == 1 for c in C.T128_CASES)
    full = [C.launch_of(c) for c in C.T128_CASES if c.rows == C.T128_LAST]
    assert {la.nct for la in full} == {2, 4, 8, 12} and all(la.grid == 256 and la.last == (128, None) for la in full)


def test_generic_column_tiles_split_between_the_wave_halves():
    got = {d_out: C.generic_launch(C.F32, 1, 32, d_out).halves for d_out in C.GEN_DOUT}
    assert got == {16: (1, 0), 48: (2, 1), 192: (6, 6), 208: (7, 6), 240: (8, 7), 256: (8, 8)}
    assert all(max(h) <= 8 for h in got.values())                                        # MAXCT
    assert C.generic_launch(C.F32, 1, 32, 192).ngt == 78 <= 8 * 10 and C.generic_launch(C.F32, 1, 32, 256).ngt == 136 == 8 * 17
    assert C.generic_launch(C.F32, 1, 32, 208).ngt == 91 > 8 * 10


def test_every_256_row_width_has_the_four_pass_shapes():
    for d_out in C.X3_DOUT:
        shapes = {C.launch_of(c).shape: C.launch_of(c).last for c in C.T256_CASES
                  if c.d_out == d_out and c.d_in == 32 and c.rows != C.T256_WRAP_ROWS}
        assert shapes == {"skipped": (1, None), "empty": (128, None), "partial": (128, 5), "full": (128, 128)}
    d96 = [c for c in C.T256_CASES if c.d_in == 96]
    assert {c.d_out for c in d96} == {192} and len(d96) == 5
    assert {c.d_in for c in C.T128_CASES} == {32, 64, 96, 160}            # 1, 2, 3 and 5 K chunks


def test_the_boundaries_sit_where_the_launchers_put_them():
    assert C.generic_launch(C.BF16, 1, 32, 192).template[1] == 10 and C.generic_launch(C.BF16, 1, 32, 208).template[1] == 17
    assert C.bf16x3_launch(32768, 32, 32).kernel == "t128" and C.bf16x3_launch(32769, 32, 32).kernel == "t256"
    assert C.bf16x3_launch(32769, 32, 32).grid == 129 and C.bf16x3_launch(65536, 32, 32).trips == 1
    assert C.bf16x3_launch(65537, 32, 32).trips == 2
    assert C.generic_launch(C.F32, 16384, 32, 16).trips == 1 and C.generic_launch(C.F32, 16385, 32, 16).trips == 2
    # rsplit = clamp(min(512 / nblk, ntile / 8), 1)
    assert C.wide_launch(70, 16).rsplit == 1 and C.wide_launch(70, 4096).rsplit == 1 and C.wide_launch(70, 4096).nblk == 528
    assert C.wide_launch(511, 16).rsplit == 1 and C.wide_launch(513, 16).rsplit == 1 and C.wide_launch(1025, 16).rsplit == 2
    assert C.wide_launch(1537, 400).rsplit == 3 and C.wide_launch(1537, 400).slices == [(0, 8), (8, 16), (16, 25)]
    assert C.wide_launch(64 * 8 * 60, 400).rsplit == 51 == 512 // 10 and C.wide_launch(64 * 8 * 51, 400).rsplit == 51
    assert C.wide_launch(64 * 8 * 50, 400).rsplit == 50
    got = {(c.rows, c.d_out): C.launch_of(c) for c in C.WIDE_CASES}
    assert {la.rsplit for la in got.values()} == {1, 3}
    assert {(la.nbc, la.nblk) for la in got.values()} == {(1, 1), (2, 3), (4, 10), (32, 528)}
    assert any(la.rsplit > 1 and la.ntile % la.rsplit for la in got.values())
    assert all(r % 64 == 1 for (r, _d) in got if r in (1537, 129))


_WALKED = (C.GENERIC_WRAP[:1] + [c for c in C.GENERIC_CASES if c.dtype == C.F32 and c.d_out == 48 and c.d_in == 32]
           + [c for c in C.T128_CASES if c.d_out == 64 and c.d_in == 32]
           + [c for c in C.T256_CASES if c.d_out == 32] + C.VIEW_CASES[:2] + C.WIDE_CASES[:6])


@pytest.mark.parametrize("case", _WALKED, ids=C.case_id)
def test_the_loops_visit_every_row_once(case):
    seen = C.rows_visited(case)
    assert len(seen) == case.rows and min(seen) == 0 and max(seen) == case.rows - 1 and set(seen.values()) == {1}
    la = C.launch_of(case)
    if case.kind == "wide":
        assert la.slices[0][0] == 0 and la.slices[-1][1] == la.ntile
        assert all(a[1] == b[0] for a, b in zip(la.slices, la.slices[1:]))
    else:
        tile = {"generic": C.TM, "bf16x3": C.TM2 if la[0] == "t128" else 2 * C.TM2}[case.kind]
        assert la.ntiles == len(range(0, case.rows, tile)) and la.trips == len(range(0, la.ntiles, la.grid))


def test_view_addressing_is_that_of_the_strided_view():
    for case in C.VIEW_CASES:
        b, t = case.view
        rpb, stride = C.view_args(case)
        buf = torch.arange(b * t * case.d_in).view(b, t, case.d_in)
        first = buf[:, 1:, 0].reshape(-1) - case.d_in                   # offsets from x = &buf[0, 1, 0]
        rows = [0, rpb - 1, rpb, case.rows - 1] + C.marked_rows(case)[:40]
        assert all(C.view_offset(r, rpb, stride, case.d_in) == int(first[r]) for r in rows)


def test_inputs_are_what_the_cases_say():
    case = C.T128_CASES[4]                                               # 300 x 32 -> 32
    assert (case.rows, case.d_in, case.d_out) == (300, 32, 32)
    assert C.marked_rows(case) == [0, 127, 128, 255, 256, 299]
    big = C.VIEW_CASES[1]
    marks = set(C.marked_rows(big))
    assert {0, 195, 196, 127, 128, 255, 256, 33123} <= marks             # batch, pass and tile boundaries
    x = C.tokens(case, "marked").float()
    assert bool((x[[0, 127, 128, 299]].abs() == C.MARK).all()) and not torch.equal(x[127], x[128])
    assert float(x[1:127].abs().max()) < 6
    x = C.tokens(case, "one_hot")
    assert x.dtype == torch.bfloat16 and bool((x.float().sum(1) == 1).all()) and bool(((x != 0).sum(1) == 1).all())
    x = C.tokens(case, "offset").float()
    assert 20 < float((x.mean(0).abs() / x.std(0)).mean()) < 40          # column means 30 x the spread
    assert torch.equal(C.tokens(case, "plain"), C.tokens(case, "plain")) and C.tokens(C.GENERIC_CASES[0], "plain").dtype == torch.float32
    assert torch.equal(C.tokens(C.GENERIC_CASES[0], "plain"), C.tokens(C.GENERIC_CASES[0], "plain").bfloat16().float())
    p = C.projection(case)
    assert torch.allclose(p @ p.T, torch.eye(32), atol=1e-5)
    p = C.projection(C.T128_CASES[-1])
    assert C.T128_CASES[-1].proj == "binades" and float(p.abs().max() / p.abs().median()) > 8
    hi, mid, lo = C.split3(p)
    assert float(((hi.double() + mid.double() + lo.double()) - p.double()).abs().max()) <= 2.0 ** -27 * float(p.abs().max())
    buf = C.view_buffer(C.VIEW_CASES[0], C.tokens(C.VIEW_CASES[0], "plain"))
    assert buf.shape == (3, 51, 32) and bool((buf[:, 0] == C.POISON).all())
    assert torch.equal(buf[:, 1:].reshape(150, 32), C.tokens(C.VIEW_CASES[0], "plain"))


# ------------------------------------------------------------------------------------------------------------------
# the emulation inside the bounds the kernels get
# ------------------------------------------------------------------------------------------------------------------
_WORST = {}


def _note(path, got, case, regime):
    for name, v in got.items():
        if v >= _WORST.get((path, name), (-1.0, None))[0]:
            _WORST[(path, name)] = (v, f"{C.case_id(case)} {regime}")


def _emulate(case, x, variant="", drop_lo=False, routed=None):
    accum, chunk = C.accumulation(case, routed)
    z = x if accum == "none" else C.emulate_z(x, C.projection(case), accum, drop_lo)
    return C.emulate_stats(z, chunk, variant)


def _ref(case, regime, routed=None):
    x = C.tokens(case, regime)
    return x, C.reference(case, x, None if case.kind == "wide" else C.projection(case), routed)


@pytest.mark.parametrize("case", C.DIRECT_CASES, ids=C.case_id)
def test_emulation_is_inside_the_bounds(case):
    for regime in C.regimes(case):
        x, ref = _ref(case, regime)
        got = ref.ratios(*_emulate(case, x))
        _note(C.path_of(case), got, case, regime)
        assert set(got) == {"gram", "colsum", "centred"}
        assert all(v <= 1.0 for v in got.values()), (regime, got)


@pytest.mark.parametrize("case,routed", C.ROUTE_CASES, ids=[C.case_id(c) for c, _w in C.ROUTE_CASES])
def test_emulated_routes_are_inside_the_bounds(case, routed):
    for regime in C.REGIMES:
        x, ref = _ref(case, regime, routed)
        got = ref.ratios(*_emulate(case, x, routed=routed))
        _note("route " + "/".join(routed), got, case, regime)
        assert all(v <= 1.0 for v in got.values()), (regime, got)


def test_report_emulation_ratios():
    """runs after the two bound tests above: the largest err / bound of the emulation per path (pytest -s)"""
    for (path, name), (v, where) in sorted(_WORST.items()):
        print(f"token-stats-emul {path} {name}: {v:.4f} at {where}")


# ------------------------------------------------------------------------------------------------------------------
# the bounds reject what they are there to reject
# ------------------------------------------------------------------------------------------------------------------
def _pick(cases, **want):
    hit = [c for c in cases if all(getattr(c, k) == v for k, v in want.items())]
    assert hit, want
    return hit[0]


_ROW_CASES = [_pick(C.GENERIC_CASES, dtype=C.F32, rows=200, d_in=32, d_out=48),
              _pick(C.GENERIC_CASES, dtype=C.BF16, rows=200, d_in=32, d_out=240), C.GENERIC_WRAP[0],
              _pick(C.T128_CASES, rows=300, d_in=32, d_out=64), _pick(C.T128_CASES, rows=300, d_in=160, d_out=192),
              _pick(C.T256_CASES, rows=32768 + 133, d_in=32, d_out=32),
              _pick(C.T256_CASES, rows=C.T256_WRAP_ROWS, d_in=96, d_out=192),
              _pick(C.WIDE_CASES, rows=1537, d_out=144)]


@pytest.mark.parametrize("case", _ROW_CASES, ids=C.case_id)
def test_a_row_at_risk_dropped_or_doubled_is_rejected(case):
    x, ref = _ref(case, "marked")
    assert max(ref.ratios(*_emulate(case, x)).values()) <= 1.0
    b = C.boundary_rows(case)
    at_risk = [case.rows - 1, b[0] - 1, b[0], b[-1]]
    if case.kind == "bf16x3" and C.launch_of(case).kernel == "t256":
        at_risk += [128, 127, 256 * (C.launch_of(case).ntiles - 1)]        # the pass boundary of tile 0; the last tile
    keep = torch.ones(case.rows, dtype=torch.bool)
    for r in at_risk:
        keep[r] = False
        dropped = ref.ratios(*_emulate(case, x[keep]))
        keep[r] = True
        doubled = ref.ratios(*_emulate(case, torch.cat([x, x[r:r + 1]])))
        print(f"{C.case_id(case)} row {r}: dropped {dropped['gram']:.1f}, doubled {doubled['gram']:.1f} x the bound")
        assert dropped["gram"] > 1.0 and dropped["centred"] > 1.0 and dropped["colsum"] > 1.0, (r, dropped)
        assert doubled["gram"] > 1.0 and doubled["centred"] > 1.0 and doubled["colsum"] > 1.0, (r, doubled)


@pytest.mark.parametrize("case", C.VIEW_CASES, ids=C.case_id)
def test_a_batch_boundary_off_by_one_row_is_rejected(case):
    """the batch of row r taken as (r + 1) / N: the last row of every batch is read one slot before the next batch's
    first token -- the CLS slot -- in both regimes that are there for it"""
    b, t = case.view
    n = t - 1
    for regime in ("plain", "marked"):
        x, ref = _ref(case, regime)
        flat = C.view_buffer(case, x).view(-1, case.d_in)
        r = torch.arange(case.rows)
        right = flat[(r // n) * t + 1 + r % n]
        assert torch.equal(right, x) and max(ref.ratios(*_emulate(case, right)).values()) <= 1.0
        gb = ((r + 1) // n).clamp(max=b - 1)
        wrong = flat[gb * t + 1 + (r - gb * n)]
        assert int((wrong != x).any(1).sum()) == b - 1
        assert min(ref.ratios(*_emulate(case, wrong)).values()) > 1.0


@pytest.mark.parametrize("case", [_pick(C.T128_CASES, rows=300, d_in=32, d_out=64), C.T128_CASES[-1],
                                  _pick(C.T256_CASES, rows=32768 + 1, d_in=32, d_out=128)], ids=C.case_id)
def test_a_dropped_lo_split_is_rejected_on_one_hot_rows(case):
    x, ref = _ref(case, "one_hot")
    good = ref.ratios(*_emulate(case, x))
    bad = ref.ratios(*_emulate(case, x, drop_lo=True))
    print(f"{C.case_id(case)}: colsum with lo {good['colsum']:.3f}, without {bad['colsum']:.1f} x the bound")
    # the column sums pin the split (the Gram's bound also carries the fp32 sums of the centred products: 131 u)
    assert max(good.values()) <= 1.0 and bad["colsum"] > 1.0


@pytest.mark.parametrize("case", [_pick(C.T128_CASES, rows=300, d_in=32, d_out=32),
                                  _pick(C.WIDE_CASES, rows=1537, d_out=144), _pick(C.WIDE_CASES, rows=70, d_out=16)],
                         ids=C.case_id)
def test_an_uncentred_fp32_gram_is_rejected_on_offset_rows(case):
    """On the bf16x3 paths the bound also carries the worst case of the three-split projection's 95 fp32 additions,
    which no rounding pattern of the torch products comes near: there the wrong Gram lands only 1.5 x outside the bound
    at 300 x 32 -> 32, and inside it at 127, 128 and 32768 rows (measured: 0.1 x at 32768).  basd_gram_f32_centred has
    no projection and rejects it a hundred times over; it is the same Gram arithmetic."""
    x, ref = _ref(case, "offset")
    good = ref.ratios(*_emulate(case, x))
    bad = ref.ratios(*_emulate(case, x, variant="uncentred"))
    print(f"{C.case_id(case)}: centred Gram {good['centred']:.3f}, from an uncentred fp32 Gram {bad['centred']:.1f} x the bound")
    assert max(good.values()) <= 1.0 and bad["centred"] > 1.0


@pytest.mark.parametrize("case", [_pick(C.T128_CASES, rows=300, d_in=32, d_out=64), _pick(C.T128_CASES, rows=1, d_in=32, d_out=32),
                                  _pick(C.T256_CASES, rows=32768 + 133, d_in=32, d_out=32),
                                  _pick(C.WIDE_CASES, rows=1537, d_out=16)], ids=C.case_id)
def test_sums_over_the_padded_tile_height_are_rejected(case):
    for regime in ("offset", "marked"):
        x, ref = _ref(case, regime)
        bad = ref.ratios(*_emulate(case, x, variant="padded"))
        assert bad["gram"] > 1.0 and bad["centred"] > 1.0, (regime, bad)


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
BASD_OK, BASD_ERR_SHAPE, BASD_ERR_DTYPE = 0, 1, 4


def _host(n, dtype):
    """a host buffer behind a fake pointer: nothing may be read or written through it"""
    t = torch.full((n,), -7, dtype=dtype)
    return t, ctypes.c_void_p(t.data_ptr())


def _off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


@pytest.mark.parametrize("d_out", [0, 8, 24, 257, 272])
def test_generic_entry_refuses_unsupported_d_out(entries, d_out):
    t, p = _host(4096, torch.float64)
    for code in (0, 1):
        assert entries.basd_token_gram(p, code, 100, 32, 100, 0, p, d_out, p, p, _NULL) == BASD_ERR_SHAPE
    assert str(d_out).encode() in entries.basd_last_error() and bool((t == -7).all())


@pytest.mark.parametrize("d_out", [0, 16, 48, 96, 160, 208, 256])
def test_bf16x3_entry_refuses_d_out_outside_its_set(entries, d_out):
    t, p = _host(4096, torch.float64)
    assert entries.basd_token_gram_bf16x3(p, 100, 32, 100, 0, p, d_out, p, p, _NULL) == BASD_ERR_SHAPE
    assert str(d_out).encode() in entries.basd_last_error() and bool((t == -7).all())


@pytest.mark.parametrize("d_in", [0, 16, 48, 100])
def test_entries_refuse_d_in_off_the_k_chunk(entries, d_in):
    t, p = _host(4096, torch.float64)
    assert entries.basd_token_gram(p, 0, 100, d_in, 100, 0, p, 32, p, p, _NULL) == BASD_ERR_SHAPE
    assert entries.basd_token_gram_bf16x3(p, 100, d_in, 100, 0, p, 32, p, p, _NULL) == BASD_ERR_SHAPE
    assert bool((t == -7).all())


def test_entries_refuse_bad_rows_per_batch_and_dtype_and_accept_no_rows(entries):
    t, p = _host(4096, torch.float64)
    for rpb in (0, -5):
        assert entries.basd_token_gram(p, 0, 100, 32, rpb, 0, p, 32, p, p, _NULL) == BASD_ERR_SHAPE
        assert entries.basd_token_gram_bf16x3(p, 100, 32, rpb, 0, p, 32, p, p, _NULL) == BASD_ERR_SHAPE
        assert b"rows_per_batch" in entries.basd_last_error()
    for code in (2, 3, -1):
        assert entries.basd_token_gram(p, code, 100, 32, 100, 0, p, 32, p, p, _NULL) == BASD_ERR_DTYPE
        assert entries.basd_token_gram(p, code, 100, 32, 100, 0, p, 208, p, p, _NULL) == BASD_ERR_DTYPE
    for rows in (0, -1):
        # nothing else is looked at: not even a shape no launch would take
        assert entries.basd_token_gram(p, 0, rows, 32, 100, 0, p, 32, p, p, _NULL) == BASD_OK
        assert entries.basd_token_gram(p, 9, rows, 7, 0, 0, p, 5, p, p, _NULL) == BASD_OK
        assert entries.basd_token_gram_bf16x3(p, rows, 32, 100, 0, p, 32, p, p, _NULL) == BASD_OK
        assert entries.basd_gram_f32_centred(p, rows, 16, p, p, _NULL) == BASD_OK
    assert bool((t == -7).all())


def test_bf16x3_entry_refuses_tokens_off_the_16_byte_fragments(entries):
    """the kernels read x in 16-byte fragments: a misaligned x or a batch stride that is no multiple of 8 elements
    would fault or read the wrong tokens; _token_view never passes either, another caller of the C entry may"""
    t, p = _host(4096, torch.float64)
    assert p.value % 16 == 0
    for nbytes in (2, 4, 8, 14):
        assert entries.basd_token_gram_bf16x3(_off(p, nbytes), 100, 32, 100, 0, p, 32, p, p, _NULL) == BASD_ERR_SHAPE
    assert b"aligned" in entries.basd_last_error()
    for stride in (1, 4, 12, 197 * 32 + 4, -4):
        assert entries.basd_token_gram_bf16x3(p, 100, 32, 50, stride, p, 32, p, p, _NULL) == BASD_ERR_SHAPE
        assert str(stride).encode() in entries.basd_last_error()
    assert bool((t == -7).all())


def test_wide_entry_refuses_unsupported_widths_and_a_misaligned_z(entries):
    t, p = _host(4096, torch.float64)
    for d in (0, 8, 24, 40, 4112):
        assert entries.basd_gram_f32_centred(p, 100, d, p, p, _NULL) == BASD_ERR_SHAPE
    for nbytes in (4, 8, 12):
        assert entries.basd_gram_f32_centred(_off(p, nbytes), 100, 16, p, p, _NULL) == BASD_ERR_SHAPE
    assert bool((t == -7).all())

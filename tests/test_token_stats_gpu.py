"""The token-statistics kernels of csrc/token_gram.hip -- token_gram_kernel<T, 10 | 17>, token_gram_bf16x3_kernel<NCT>,
token_gram_bf16x3_t256_kernel<NCT>, gram_wide_f32_kernel -- per element against fp64 on every dispatch path (GPU box
only).  tests/_token_stats_cases.py holds the cases, the inputs and the derived bounds, and says which kernel a case
reaches (pinned by tests/test_token_stats_cases_cpu.py, which also holds the entries' refusals: they need no GPU).

The C entries are called directly, so that the path is the one named.  gram and colsum are caller-owned fp64 buffers
that hold a known pattern before the launch, with 64 guard elements behind each: a launch ADDS z^T z to the lower
16 x 16 tiles and 1^T z to colsum (the contract _layer_grams relies on for all layers of a step) and leaves the tiles
above the diagonal and the guards bit for bit as they were; a second launch into the same buffers doubles what was
added."""
import pytest
import torch

from tests import _token_stats_cases as C

pytestmark = pytest.mark.gpu

_WORST = {}          # (path, output) -> (largest err / bound, case): printed when the module is done (pytest -s)


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    yield native
    for (path, name), (v, where) in sorted(_WORST.items()):
        print(f"token-stats-worst {path} {name}: {v:.4f} at {where}")


def _note(path, got, case, regime):
    for name, v in got.items():
        print(f"token-stats-bound {C.case_id(case)} {regime} {name} {v:.4f}")
        if v >= _WORST.get((path, name), (-1.0, None))[0]:
            _WORST[(path, name)] = (v, f"{C.case_id(case)} {regime}")
    for name, v in got.items():
        assert v <= 1.0, (path, C.case_id(case), regime, name, v)


def _launch(nat, case, x, p, gram, colsum):
    """one direct call of the case's C entry; x: what the pointer is taken from (a [B, T - 1, d_in] view for a strided case)"""
    ptr, lib, i64 = nat._ptr, nat.lib(), __import__("ctypes").c_int64
    rpb, stride = C.view_args(case)
    if case.kind == "generic":
        rc = lib.basd_token_gram(ptr(x), C.DTYPE_CODE[case.dtype], i64(case.rows), case.d_in, rpb, i64(stride), ptr(p),
                                 case.d_out, ptr(gram), ptr(colsum), nat._stream())
    elif case.kind == "bf16x3":
        rc = lib.basd_token_gram_bf16x3(ptr(x), i64(case.rows), case.d_in, rpb, i64(stride), ptr(nat.split_bf16x3(p)),
                                        case.d_out, ptr(gram), ptr(colsum), nat._stream())
    else:
        rc = lib.basd_gram_f32_centred(ptr(x), i64(case.rows), case.d_out, ptr(gram), ptr(colsum), nat._stream())
    assert rc == 0, lib.basd_last_error()
    torch.cuda.synchronize()


def _run(nat, case, regime):
    d = case.d_out
    dense = C.tokens(case, regime)
    p = None if case.kind == "wide" else C.projection(case).cuda()
    if case.view:
        buf = C.view_buffer(case, dense).cuda()
        x = buf[:, 1:, :]
        assert x.data_ptr() % 16 == 0 and not x.is_contiguous()
    else:
        x = dense.cuda()
    # the reference: fp64 of the DENSE rows, never the same kernel on a copy
    ref = C.reference(case, dense.cuda(), p)
    pre_g, pre_c = (t.cuda() for t in C.prefill(d))
    gram, colsum = pre_g.clone(), pre_c.clone()
    low = C.lower_tiles(d, "cuda")
    pg, pc = pre_g[:d * d].view(d, d), pre_c[:d]
    worst = {}
    for launches in (1, 2):
        _launch(nat, case, x, p, gram, colsum)
        g = gram[:d * d].view(d, d)
        assert torch.equal(gram[d * d:], pre_g[d * d:]) and torch.equal(colsum[d:], pre_c[d:]), "written behind a buffer"
        assert torch.equal(g[~low], pg[~low]), "a tile above the diagonal was written"
        got = ref.ratios(g - pg, colsum[:d] - pc, pg, pc, launches=launches, centred=regime in ("offset", "marked"))
        worst.update({name + ("" if launches == 1 else " x2"): v for name, v in got.items()})
    assert int(nat.status_word(gram.device).item()) == 0
    _note(C.path_of(case), worst, case, regime)


@pytest.mark.parametrize("case", C.DIRECT_CASES, ids=C.case_id)
def test_token_statistics_against_fp64(nat, case):
    for regime in C.regimes(case):
        _run(nat, case, regime)


@pytest.mark.parametrize("case,routed", C.ROUTE_CASES, ids=[C.case_id(c) for c, _w in C.ROUTE_CASES])
def test_wrapper_routes_against_fp64(nat, case, routed):
    """_native.token_gram on every route the mirror names; where the route is a C entry that is also called directly,
    the two agree to fp64 rounding (only the order of the atomics differs)"""
    d = case.d_out
    p = C.projection(case).cuda()
    for regime in C.REGIMES:
        x = C.tokens(case, regime).cuda()
        ref = C.reference(case, x, p, routed)
        gram, colsum = nat.token_gram(x, p, mirror=False)
        torch.cuda.synchronize()
        assert gram.shape == (d, d) and colsum.shape == (d,) and gram.dtype == colsum.dtype == torch.float64
        sym = torch.tril(gram) + torch.tril(gram, -1).T               # every route fills the lower triangle at least
        _note("route " + "/".join(routed), ref.ratios(sym, colsum), case, regime)
        if routed[0] != "wide":
            direct = case._replace(kind=routed[0])
            g2 = torch.zeros(d * d, dtype=torch.float64, device="cuda")
            c2 = torch.zeros(d, dtype=torch.float64, device="cuda")
            _launch(nat, direct, x, p, g2, c2)
            low = C.lower_tiles(d, "cuda")
            assert bool(((gram - g2.view(d, d)).abs() <= 2 * ref.k64 * C.U64 * ref.sqrt_ss)[low].all())
            assert bool(((colsum - c2).abs() <= 2 * ref.colsum_fp64).all())
    assert int(nat.status_word(x.device).item()) == 0

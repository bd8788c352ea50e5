"""Bookkeeping of the weight-gradient cases (tests/test_wgrad_paths_gpu.py).

tests/_wgrad_cases.py mirrors the host arithmetic of csrc/vit_gemm.hip (``wgrad_dispatch``, ``wgrad192_applies``,
``wgrad192_slices``, ``wgrad192_workspace_bytes``, ``launch_wgrad<KT>``, ``launch_wgrad192``, the slice loop of
``wgrad192_reduce_kernel``); it must be updated with them.  These tests pin the reason every GPU case is in the list --
which kernel it reaches, how the rows are split, which workgroups find no slice, what the reduce adds -- so the list cannot
drift into shapes that no longer take those paths, and the conditions under which the integer regime is exact.  They are
no evidence about the kernels: the mirror is compared with nothing but the claims below."""
import pytest
import torch

from tests import _wgrad_cases as C


def test_register_cases_reach_the_paths_they_are_listed_for():
    a, b, c, d, e, f, g, h, i, j = (C.plan(*s) for s in C.REGISTER_CASES)
    for p in (a, b, c, d, e, f, g, h, i, j):
        assert p.tail is None and p.tail_rows == 0 and p.workspace_bytes == 0 and p.reduce_adds is None
    # a: KT = 4, one row, one slice, 7 idle workgroups in the only group
    m = a.main
    assert (a.kernel, m.tn, m.tk, m.slices, m.rows, m.chunks, m.grid, m.idle) == ("reg4", 1, 1, 1, [1], [1], 8, 7)
    # b: KT = 8, two slices, the second holds one row
    m = b.main
    assert (b.kernel, m.tk, m.slices, m.rows_per_slice, m.rows, m.chunks) == ("reg8", 1, 2, 64, [64, 1], [1, 1])
    # c: KT = 12, 6 slices of 64 rows, the last holds 13
    m = c.main
    assert (c.kernel, m.tn, m.tk, m.slices, m.rows_per_slice, m.rows[-1]) == ("reg12", 2, 1, 6, 64, 13)
    assert m.rows[:-1] == [64] * 5 and m.idle == 2 * m.tiles
    # d: K % 128 != 0 takes KT = 4 with tk = 5 k tiles: four of the five tiles of a slab must add no bias
    m = d.main
    assert C.REGISTER_CASES[3][2] % 128 != 0 and (d.kernel, m.tn, m.tk, m.slices) == ("reg4", 1, 5, 3)
    # e, f: KT = 8 and KT = 12 with tk = 2
    assert (e.kernel, e.main.tk, f.kernel, f.main.tk) == ("reg8", 2, "reg12", 2)
    # g: N, K multiples of 192 and two tiles or more, but M < 4096 keeps it off the ring; 48 tiles: 8 slices of 256 rows =
    # 4 chunks (the prefetch loop runs); the last slice has 208 rows, its last chunk 16
    m = g.main
    shape = C.REGISTER_CASES[6]
    assert shape[0] < C.RING_MIN_M and C.wgrad192_applies(C.RING_MIN_M, *shape[1:]) and g.kernel == "reg12"
    assert (m.tiles, m.slices, m.rows_per_slice, m.chunks, m.rows[-1]) == (48, 8, 256, [4] * 8, 208)
    assert m.rows[-1] % C.WG_MC == 16 and m.idle == 0
    # h: 600 tiles exceed 512: slices clamps to 1 and one workgroup walks all 4 chunks
    m = h.main
    assert (h.kernel, m.tiles, 512 // m.tiles, m.slices, m.chunks, m.idle) == ("reg4", 600, 0, 1, [4], 7 * 600)
    # i: a single 192 x 192 tile stays on the register kernel at M >= 4096; 65 slices = 9 groups, 7 idle slices
    m = i.main
    shape = C.REGISTER_CASES[8]
    assert shape[0] >= C.RING_MIN_M and shape[1] == shape[2] == C.W2_T and i.kernel == "reg12"
    assert (m.slices, m.grid, m.idle, m.rows[-1]) == (65, 9 * 8 * m.tiles, 7 * m.tiles, 1)
    # j: one row under the ring's M threshold (the same N, K reach the ring one row later)
    shape = C.REGISTER_CASES[9]
    assert shape[0] == C.RING_MIN_M - 1 and j.kernel == "reg12" and C.plan(shape[0] + 1, *shape[1:]).kernel == "ring"
    assert (j.main.slices, j.main.rows[-1]) == (64, 63)


def test_ring_cases_reach_the_paths_they_are_listed_for():
    a, b, c, d, e, f, g, h, i, j = (C.plan(*s) for s in C.RING_CASES)
    for shape, p in zip(C.RING_CASES, (a, b, c, d, e, f, g, h, i, j)):
        m = p.main
        assert p.kernel == m.kernel == "ring" and m.M == shape[0] // 64 * 64 and m.M % C.W2_MC == 0
        assert p.workspace_bytes == m.tiles * m.slices * C.W2_T * C.W2_T * 4 > 0
        assert sum(p.reduce_adds) == m.slices and all(r % C.W2_MC == 0 for r in m.rows)
    # a: the smallest ring shape (one row or one tile fewer leaves the ring); tn = 1, tk = 2: the k0 != 0 tile adds no
    # bias; 64 slices of ONE chunk: prologue only, the first wait is vmcnt(0)
    m = a.main
    shape = C.RING_CASES[0]
    assert C.plan(shape[0] - 1, *shape[1:]).kernel == "reg12" and C.plan(shape[0], 192, 192).kernel == "reg12"
    assert (m.tn, m.tk, m.slices, set(m.chunks), m.idle) == (1, 2, 64, {1}, 0)
    # b: tn = 2, tk = 1: both tiles add bias
    assert (b.main.tn, b.main.tk, b.main.slices, set(b.main.chunks)) == (2, 1, 64, {1})
    # c: 64 slices of two chunks: `more` (c + 2 < nchunks) is never true
    assert (c.main.slices, set(c.main.chunks)) == (64, {2})
    # d: three chunks: the first refill of a stage
    assert (d.main.slices, set(d.main.chunks)) == (64, {3})
    # e: 16 tiles, 16 slices, 4 chunks: chunk 3 lands in the stage of chunk 0
    assert (e.main.tiles, e.main.slices, set(e.main.chunks)) == (16, 16, {4})
    # f: 5 chunks per slice
    assert (f.main.slices, set(f.main.chunks)) == (16, {5})
    # g: rows_per_slice 320: 14 slices, the last of 64 rows; 2 idle slices in the second group; reduce groups 0..5 add
    # two slices, 6..7 one
    m = g.main
    assert (m.rows_per_slice, m.slices, m.rows[-1], m.chunks) == (320, 14, 64, [5] * 13 + [1])
    assert m.idle == 2 * m.tiles and m.grid == 2 * 8 * m.tiles and g.reduce_adds == [2] * 6 + [1] * 2
    # h: 37 tail rows go to launch_wgrad<12> through offset pointers; the workspace is sized from 4096 rows
    shape = C.RING_CASES[7]
    assert h.tail_rows == 37 and (h.tail.kernel, h.tail.row0, h.tail.M, h.tail.tn, h.tail.tk) == ("reg12", 4096, 37, 3, 2)
    assert (h.tail.slices, h.tail.rows) == (1, [37]) and h.main.M == 4096
    assert h.workspace_bytes == C.wgrad192_workspace_bytes(4096, *shape[1:]) == a.workspace_bytes
    # i: 36 tiles: 7 slices, fewer than the reduce's 8 groups: one group adds nothing; the last slab is shorter
    m = i.main
    assert (m.tiles, m.slices, m.rows_per_slice, m.rows[-1], m.idle) == (36, 7, 640, 256, 36)
    assert i.reduce_adds == [1] * 7 + [0] and m.chunks == [10] * 6 + [4]
    # j: 128 slices: 16 per reduce group, the two-at-a-time loop runs 8 times
    assert (j.main.slices, j.reduce_adds, C.reduce_pair_iterations(j.main.slices)) == (128, [16] * 8, 8)
    # the back-to-back pair: more slices (and more workspace) first
    first, second = (C.plan(*s) for s in C.BACK_TO_BACK)
    assert first.main.slices > second.main.slices and first.workspace_bytes >= second.workspace_bytes


def test_the_case_list_is_complete():
    plans = [C.plan(*s) for s in C.ALL_CASES]
    assert len(set(C.ALL_CASES)) == len(C.ALL_CASES) == 20
    assert {p.kernel for p in plans} == {"reg4", "reg8", "reg12", "ring"}
    assert all(p.kernel == "ring" for p in plans[len(C.REGISTER_CASES):])
    assert all(p.kernel != "ring" for p in plans[:len(C.REGISTER_CASES)])
    for kind in ("reg", "ring"):
        mains = [p.main for p in plans if p.kernel.startswith(kind)]
        chunks = {c for m in mains for c in m.chunks}
        assert 1 in chunks and max(chunks) >= 4, (kind, chunks)              # no loop trip, and the prefetch / refill
        assert any(m.slices % 8 for m in mains), kind                       # idle workgroups in the last group
        assert any(m.tk > 1 for m in mains) and any(m.tn > 1 for m in mains), kind
    ring = [p for p in plans if p.kernel == "ring"]
    assert {1, 2, 3} <= {c for p in ring for c in p.main.chunks}             # prologue-only paths and the first refill
    assert any(p.main.slices < C.W2_SG for p in ring)
    assert any(p.main.slices % 8 and p.main.slices > 8 for p in ring)
    assert any(len(set(p.main.rows)) > 1 for p in ring)                      # a short last slab
    assert any(p.tail_rows == 0 for p in ring) and any(p.tail_rows > 0 for p in ring)
    assert any(512 // p.main.tiles < 1 for p in plans if p.kernel != "ring")  # the slices < 1 clamp
    assert {p.kernel for p in plans if p.main.tk > 1} == {"reg4", "reg8", "reg12", "ring"}
    # the subsets of parts 3 and 4 are cases of the list, one register case per KT
    assert {C.plan(*s).kernel for s in C.NO_BIAS_REGISTER_CASES} == {"reg4", "reg8", "reg12"}
    assert all(C.plan(*s).kernel == "ring" for s in C.NO_BIAS_RING_CASES) and len(C.NO_BIAS_RING_CASES) == 2
    kinds = [(C.plan(*s).kernel == "ring", C.plan(*s).tail_rows > 0) for s in C.PYTHON_ENTRY_CASES]
    assert kinds == [(False, False), (True, False), (True, True)]
    for s in C.NO_BIAS_REGISTER_CASES + C.NO_BIAS_RING_CASES + C.PYTHON_ENTRY_CASES + C.BACK_TO_BACK:
        assert s in C.ALL_CASES


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_every_row_belongs_to_exactly_one_slice(case):
    p = C.plan(*case)
    covered = 0
    for L in (p.main, p.tail):
        if L is None:
            continue
        assert L.row0 == covered and sum(L.rows) == L.M and all(0 < r <= L.rows_per_slice for r in L.rows)
        assert L.rows_per_slice % 64 == 0 and L.grid == (L.slices * L.tiles + L.idle) and L.grid % 8 == 0
        covered += L.M
    assert covered == case[0]
    n, k = case[1] - 1, case[2] - 1
    assert ("ring" in C.locate(p, n, k)) == (p.kernel == "ring") and ("tail" in C.locate(p, n, k)) == (p.tail_rows > 0)


def _row_with_nonzeros(dy, x, start):
    ok = ((dy != 0).any(1) & (x != 0).any(1)).nonzero().flatten()
    later = ok[ok >= start]
    return int(later[0] if len(later) else ok[-1])


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_integer_regime_is_exact_and_sees_a_dropped_or_doubled_row(case):
    """The condition under which fp32 sums of the integer inputs are exact in ANY order: max (|dw0| + |dy|^T |x|) and
    max (|db0| + sum |dy|) below 2^24.  And, on the reference alone, that the regime can see what it is there for: with
    one row of (dy, x) removed, or doubled, dw and db change (the reference is additive over the rows, so the change
    is the reference of that row alone; for small M it is also recomputed from the edited inputs)."""
    M, N, K = case
    dy, x, dw0, db0 = C.integer_inputs(M, N, K)
    for t, top in ((dy, C.INT_DY), (x, C.INT_X), (dw0, C.INT_INIT), (db0, C.INT_INIT)):
        assert torch.equal(t.float(), t.float().round()) and float(t.float().abs().max()) <= top
    assert dy.dtype == x.dtype == torch.bfloat16 and dw0.dtype == db0.dtype == torch.float32
    assert float(dy.float().abs().max()) == C.INT_DY or M == 1
    mag_w, mag_b = C.magnitude(dy, x)
    assert float((mag_w + dw0.double().abs()).max()) < C.EXACT_LIMIT
    assert float((mag_b + db0.double().abs()).max()) < C.EXACT_LIMIT
    assert C.INT_DY * C.INT_X * M + C.INT_INIT < C.EXACT_LIMIT
    ref_w, ref_b = C.reference(dy, x, dw0, db0)
    assert torch.equal(ref_w, ref_w.round()) and ref_w.dtype == torch.float64
    assert torch.equal(ref_w.float().double(), ref_w) and torch.equal(ref_b.float().double(), ref_b)
    for start in (0, M // 2, M - 1):                      # the last row is the one a wrong m_end drops
        m = _row_with_nonzeros(dy, x, start)
        one_w, one_b = C.reference(dy[m:m + 1], x[m:m + 1])
        assert bool((one_w != 0).any()) and bool((one_b != 0).any()), m
        if M <= 400:
            keep = torch.arange(M) != m
            gone = C.reference(dy[keep], x[keep], dw0, db0)
            twice = C.reference(torch.cat([dy, dy[m:m + 1]]), torch.cat([x, x[m:m + 1]]), dw0, db0)
            assert torch.equal(gone[0], ref_w - one_w) and torch.equal(gone[1], ref_b - one_b)
            assert torch.equal(twice[0], ref_w + one_w) and torch.equal(twice[1], ref_b + one_b)
            assert not torch.equal(gone[0], ref_w) and not torch.equal(twice[0], ref_w)
            assert not torch.equal(gone[1], ref_b) and not torch.equal(twice[1], ref_b)


@pytest.mark.parametrize("case", [s for s in C.ALL_CASES if s[0] <= 400] + [(4133, 192, 384)], ids=C.case_id)
def test_real_regime_inputs_and_tolerance(case):
    """The real regime's inputs (bf16, nothing subnormal, four decades of row scales) and the tolerance: four times the
    recorded worst ratio of the CPU emulation, never above the first-order bound M 2^-23; the emulation itself stays
    inside what it lends the kernels."""
    M, N, K = case
    dy, x = C.real_inputs(M, N, K)
    assert dy.dtype == x.dtype == torch.bfloat16 and dy.shape == (M, N) and x.shape == (M, K)
    for t in (dy, x):
        assert bool(torch.isfinite(t.float()).all()) and float(t.float().abs().min()) >= 0.99 * C.TINY
    if M >= 64:
        rows = dy.float().abs().amax(1)
        assert float(rows.max() / rows.min()) > 1e2
    assert C.TOL == 4.0 * C.EMUL_WORST_RATIO and 0 < C.tolerance(M) <= min(C.TOL, M * 2.0 ** -23)
    p = C.plan(M, N, K)
    got = C.emulate_plan(dy, x, p)
    rw, rb = C.worst_ratio(*got, *C.reference(dy, x), *C.magnitude(dy, x))
    assert rw <= C.tolerance(M) and rb <= C.tolerance(M), (rw, rb)

"""Bookkeeping of the bf16 GEMM schedule cases (tests/test_gemm_schedule_gpu.py).

tests/_gemm_cases.py mirrors the host arithmetic of csrc/gemm_bf16.hip (``gemm_dispatch``, ``pring_cus_per_xcd``,
``gemm_column_group``, ``launch_gemm_pring``) and the persistent kernel's ``block_pos`` / ``tile_at``; it must be updated
with them.  These tests pin the reason every GPU case is in the list -- which kernel it reaches, how many workgroups find
no tile, where the ragged tiles sit -- so the list cannot drift into shapes that no longer take those paths.  They are
no evidence about the kernels: the mirror is compared with nothing but the claims below."""
import pytest
import torch

from tests import _gemm_cases as C


def _s(shape, tile_run):
    return C.schedule(*shape, tile_run)


def test_pring_cases_reach_the_paths_they_are_listed_for():
    a, b, c, d, e = C.PRING_SHAPES
    for shape in C.PRING_SHAPES:
        assert C.dispatch(*shape) == "pring" and shape[2] // 64 >= 3
    # a: the smallest M on the persistent kernel at N = 3072 (one row block fewer falls off), nk = 3 = the kernel's
    # minimum, one valid row in the last block
    assert (a[0] + 255) // 256 == 24 and a[0] % 256 == 1 and a[2] // 64 == 3
    assert C.dispatch(a[0] - 256, a[1], a[2]) != "pring"
    assert [_s(a, t).ragged_followed for t in (0, 2, -32, -8)] == [1, 1, 1, 4]
    s = _s(a, 1)
    assert (s.grid, s.idle, set(s.tiles_per_workgroup)) == (512, 224, {1})
    # b: column group 4 of 12 tiles (the 1.6 MB rule): ragged tiles mid-stream
    assert b[0] % 256 == 1 and _s(b, 0).ngroup == 4 and _s(b, 0).tiles_n == 12
    assert [_s(b, t).ragged_followed for t in (0, 2, -32, -20, -8)] == [4, 4, 4, 5, 8]
    # c: K > N keeps all column tiles in one group although the weight matrix exceeds 1.6 MB; nk = 20; the last block
    # has 129 valid rows = one row into the second wave row
    assert c[2] > c[1] and c[1] * c[2] * 2 > 1.6e6 and _s(c, 0).ngroup == _s(c, 0).tiles_n == 4
    assert c[2] // 64 == 20 and c[0] % 256 == 129
    # d: 50 row blocks: XCDs 0-1 hold 84 tiles, XCDs 2-7 hold 72: blocks of 3 and 2 tiles; tile_run 2: two chunks, the
    # second of one tile or none (a last chunk shorter than chunk_tiles); tile_run 3 is fully persistent in chunks
    s = _s(d, 0)
    assert s.mblocks == 50 and s.tiles_n == 12 and set(s.tiles_per_workgroup) == {2, 3} and s.idle == 0
    per_xcd = [sum(1 for (mb, _nb) in s.coverage if mb % 8 == x) for x in range(8)]
    assert per_xcd == [84, 84, 72, 72, 72, 72, 72, 72]
    s = _s(d, 2)
    assert s.chunks == 2 and s.grid == 512 and s.idle > 0
    assert sorted(s.tiles_per_workgroup[:256]) == sorted(min(t, 2) for t in _s(d, 0).tiles_per_workgroup)
    assert set(s.tiles_per_workgroup[256:]) == {1} and len(s.tiles_per_workgroup[256:]) == 512 - 256 - s.idle
    s3 = _s(d, 3)
    assert s3.chunks == 1 and s3.tiles_per_workgroup == _s(d, 0).tiles_per_workgroup
    # e: 16 column tiles in one group; 8 workgroups per XCD: 6 to 8 tiles each, 8 ragged tiles mid-stream
    s = _s(e, -8)
    assert s.tiles_n == s.ngroup == 16 and min(s.tiles_per_workgroup) == 6 and max(s.tiles_per_workgroup) == 8
    assert s.ragged_followed == 8
    # tile_run 3 differs from 0 on d only: elsewhere no workgroup holds more than 2 tiles
    for shape in (a, b, c, e):
        assert max(_s(shape, 0).tiles_per_workgroup) == 2


def test_negative_tile_run_is_clamped_to_8_and_32_workgroups_per_xcd():
    for shape in C.PRING_SHAPES:
        assert [_s(shape, t).P for t in C.TILE_RUNS] == [32, 32, 32, 8, 20, 32, 8, 32]
        assert _s(shape, -1) == _s(shape, -8) and _s(shape, -100) == _s(shape, -32) == _s(shape, 0)


def test_other_cases_reach_the_kernels_they_are_listed_for():
    for shape, kernel in C.OTHER_SHAPES.items():
        assert C.dispatch(*shape) == kernel, shape
    ring_nk = sorted(k // 64 for (m, n, k), kernel in C.OTHER_SHAPES.items() if kernel == "ring" and m == 8193)
    assert ring_nk == [1, 2, 3, 4]                   # the prologue's three first waits and the one-unit tail
    assert sorted(k // 64 for (_m, _n, k), kernel in C.OTHER_SHAPES.items() if kernel == "nt192")[:2] == [1, 2]
    # the dispatch neighbours of the persistent kernel: one row block fewer, one K step fewer
    assert C.pring_cus_per_xcd(5633, 3072) == 24 and C.pring_cus_per_xcd(15873, 1024) == 28
    assert C.dispatch(5889, 3072, 192) == C.dispatch(16513, 1024, 192) == "pring"


@pytest.mark.parametrize("case", list(dict.fromkeys(C.INVARIANCE_CASES + C.REFERENCE_CASES + C.RAGGED_CASES)),
                         ids=C.case_id)
def test_every_tile_is_covered_exactly_once(case):
    s = C.schedule(*case)
    assert C.covers_every_tile_once(s)
    assert s.grid == s.idle + len(s.tiles_per_workgroup)
    assert sum(s.tiles_per_workgroup) == s.mblocks * s.tiles_n


@pytest.mark.parametrize("shape", [(300, 640, 192), (6401, 3072, 768), (16513, 1024, 1280)], ids=C.case_id)
def test_integer_inputs_keep_every_partial_sum_exact(shape):
    """|x| <= 1, at most 240 non-zeros per row of w and |bias| <= 8 bound every partial sum of x w^T + bias by 248 < 256:
    integers that fp32 adds exactly in any order and that bf16 holds exactly"""
    M, N, K = shape
    x, w, b = C.integer_inputs(M, N, K)
    for t in (x, w, b):
        assert t.dtype == torch.bfloat16 and torch.equal(t.float(), t.float().round())
    assert float(x.float().abs().max()) == 1 and float(w.float().abs().max()) == 1
    nnz = (w != 0).sum(1)
    assert int(nnz.max()) <= C.MAX_ROW_NONZEROS and float(b.float().abs().max()) <= C.MAX_BIAS
    assert int(nnz.min()) >= min(K, C.MAX_ROW_NONZEROS) // 3          # thinned, not emptied
    # every K step of every 16-row fragment of w keeps non-zeros: a dropped step changes an integer
    assert bool(((w != 0).view(N // 16, 16, K // 64, 64).sum((1, 3)) > 0).all())
    assert int(nnz.max()) + C.MAX_BIAS <= 256

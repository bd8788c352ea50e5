"""Case list and bookkeeping of tests/test_gemm_schedule_gpu.py.

A plain-Python mirror of the HOST arithmetic of csrc/gemm_bf16.hip -- ``gemm_dispatch`` (tile width, which kernel),
``pring_cus_per_xcd``, ``gemm_column_group``, ``launch_gemm_pring`` (P, chunks, grid) -- and of the persistent kernel's
``block_pos`` / ``tile_at``.  It must be updated together with them.  It says which kernel and which schedule a case
reaches, so that the case list cannot drift into shapes that no longer take the paths they are there for; it is
bookkeeping for the GPU cases, not evidence about the kernels.

Also the input builders of the GPU tests (CPU generators, so that the same case has the same inputs everywhere and the
integer cases' exactness condition can be checked without a GPU).
"""
from __future__ import annotations

import collections

import torch

GBM, GBK = 256, 64

# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
# shapes that reach the persistent ring kernel, with the reason each one is there (asserted in test_gemm_cases_cpu.py)
PRING_SHAPES = [
    (5889, 3072, 192),     # smallest M on the persistent kernel at this N; nk = 3; 1 valid row in the last block
    (6401, 3072, 768),     # column group 4 < 12 tiles: ragged tiles mid-stream
    (16513, 1024, 1280),   # K > N branch of the column group; nk = 20; 129 valid rows in the last block
    (12545, 3072, 192),    # uneven XCD streams (84 / 72 tiles); tile_run 2: a second chunk of one tile or none
    (6913, 4096, 192),     # 16 column tiles in one group
]
TILE_RUNS = [0, 1, 2, -8, -20, -32, -1, -100]          # -1 / -100: clamped to P = 8 / P = 32
# (shape, tile_run) of the invariance test: tile_run 3 differs from 0 only where a workgroup holds more than 2 tiles
INVARIANCE_CASES = [s + (t,) for s in PRING_SHAPES for t in TILE_RUNS] + [PRING_SHAPES[3] + (3,)]

# shapes off the persistent kernel: (M, N, K) -> the kernel gemm_dispatch picks
OTHER_SHAPES = {
    (5633, 3072, 192): "nt192",     # 23 row blocks: (23 / 8) * 12 = 24 < 32 leaves the persistent kernel
    (5889, 3072, 128): "nt192",     # K < 192 leaves the persistent kernel
    (257, 256, 64): "nt128",        # nk = 1 .. 4; one full row block plus a 1-row block
    (257, 256, 128): "nt128",
    (257, 256, 192): "nt128",
    (257, 256, 256): "nt128",
    (1, 512, 320): "nt128",         # a single row
    (255, 192, 64): "nt192",        # the peeled last K step alone
    (513, 576, 128): "nt192",
    (129, 384, 64): "nt128",
    (300, 640, 192): "nt128",       # 5 column tiles
    # The dispatcher prefers the narrow tiles wherever 256-wide ones fill the CUs worse (up to 128 tiles of 256 columns
    # always lose to twice as many of 128, and N % 192 == 0 usually wins at two rounds), so the shapes above reach the
    # two-stage kernel only.  These reach the non-persistent RING kernel: 129 .. 256 tiles of 256 columns in one
    # round, N % 192 != 0, and (row blocks / 8) * column tiles < 32 or K < 192.
    (8193, 1024, 64): "ring",       # nk = 1: prologue of 2 units, first wait vmcnt(0)
    (8193, 1024, 128): "ring",      # nk = 2: prologue of 4 units, first wait vmcnt(8)
    (8193, 1024, 192): "ring",      # nk = 3: prologue of 5 units, "exactly one unit left" tail
    (8193, 1024, 256): "ring",      # nk = 4: one steady-state step, then the one-unit tail
    (15873, 1024, 192): "ring",     # 63 row blocks: (63 / 8) * 4 = 28 < 32 leaves the persistent kernel
    (16513, 1024, 128): "ring",     # persistent-size grid, K < 192
}
# parts 2 and 3: (M, N, K, tile_run)
REFERENCE_CASES = [s + (t,) for s in PRING_SHAPES for t in (0, 1)] + [s + (0,) for s in OTHER_SHAPES]
# part 4
RAGGED_CASES = ([s + (t,) for s in PRING_SHAPES for t in (0, -8)]
                + [(257, 256, 192, 0), (255, 192, 64, 0), (300, 640, 192, 0), (8193, 1024, 192, 0)])


def case_id(case) -> str:
    return "x".join(str(v) for v in case[:3]) + "".join(f"-run{v}" for v in case[3:])


# ------------------------------------------------------------------------------------------------------------------
# mirror of the launcher (csrc/gemm_bf16.hip)
# ------------------------------------------------------------------------------------------------------------------
def gemm_column_group(tiles_n: int, bn: int, K: int) -> int:
    tile_bytes = float(bn) * K * 2.0
    if tiles_n * tile_bytes <= 1.6e6 or K > tiles_n * bn:
        return tiles_n
    best = 1
    for g in range(1, tiles_n + 1):
        if tiles_n % g == 0 and g * tile_bytes <= 1.6e6:
            best = g
    return best


def pring_cus_per_xcd(M: int, N: int) -> int:
    tiles_n, mblocks = N // 256, (M + GBM - 1) // GBM
    if N % 256 or mblocks < 8:
        return 0
    return min((mblocks // 8) * tiles_n, 32)


def dispatch(M: int, N: int, K: int) -> str:
    """the kernel gemm_dispatch launches: 'pring', 'ring', 'nt192' or 'nt128'"""
    assert M > 0 and K % GBK == 0 and K >= GBK and N >= 128 and (N % 256 == 0 or N % 192 == 0 or N % 128 == 0)
    mblocks = (M + GBM - 1) // GBM
    best_bn, best_eff = 0, -1.0
    for bn in (256, 192, 128):
        if N % bn:
            continue
        tiles = mblocks * (N // bn)
        rounds = (tiles + 255) // 256
        eff = tiles / (rounds * 256.0) * {256: 1.0, 192: 0.8, 128: 0.6}[bn]
        if eff > best_eff + 1e-9:
            best_eff, best_bn = eff, bn
    if pring_cus_per_xcd(M, N) == 32 and K >= 192:
        return "pring"
    return {256: "ring", 192: "nt192", 128: "nt128"}[best_bn]


Schedule = collections.namedtuple(
    "Schedule", "kernel grid P chunks ngroup idle tiles_per_workgroup ragged_followed coverage mblocks tiles_n")


def schedule(M: int, N: int, K: int, tile_run: int = 0) -> Schedule:
    """What a launch of (M, N, K, tile_run) runs.  For the persistent kernel: the grid, P (workgroups per XCD), the
    chunks, the idle workgroups (``if (o >= ntiles) return``), the tiles of every working workgroup in launch order,
    the number of ragged tiles (m0 + 256 > M) that are followed by another tile of the same workgroup, and a Counter
    (row block, column tile) -> how many workgroups multiply it.  For the other kernels: kernel, grid, coverage."""
    kernel = dispatch(M, N, K)
    mblocks = (M + GBM - 1) // GBM
    if kernel != "pring":
        bn = {"ring": 256, "nt192": 192, "nt128": 128}[kernel]
        tiles_n, groups = N // bn, (mblocks + 7) // 8
        ngroup = gemm_column_group(tiles_n, bn, K)
        grid = groups * tiles_n * 8
        cover, idle = collections.Counter(), 0
        for lin in range(grid):                                   # gemm_tile_of
            xcd, idx = lin & 7, lin >> 3
            nbi, rest = idx % ngroup, idx // ngroup
            mbl, ng = rest % groups, rest // groups
            mb, nb = mbl * 8 + xcd, ng * ngroup + nbi
            if mb >= mblocks:
                idle += 1
                continue
            cover[(mb, nb)] += 1
        return Schedule(kernel, grid, 0, 1, ngroup, idle, [1] * (grid - idle), 0, cover, mblocks, tiles_n)

    # launch_gemm_pring
    tiles_n = (N + 255) // 256
    ngroup = gemm_column_group(tiles_n, 256, K)
    P = 32
    if tile_run < 0:
        P = 8 if -tile_run < 8 else (32 if -tile_run > 32 else -tile_run)
        tile_run = 0
    chunk_tiles = tile_run if tile_run > 0 else 1 << 20
    max_block = ((mblocks + 7) // 8 * tiles_n + P - 1) // P
    chunks = (max_block + chunk_tiles - 1) // chunk_tiles
    grid = 8 * P * chunks
    # gemm_bf16_pring_kernel
    cover, idle, per_wg, ragged_followed = collections.Counter(), 0, [], 0
    for block in range(grid):
        chunk = block // (8 * P)
        slot_id = block - chunk * (8 * P)
        xcd, ci = slot_id & 7, slot_id >> 3
        rb = (mblocks - xcd + 7) >> 3
        n_x = rb * tiles_n
        R0 = n_x // P
        rem = n_x - R0 * P

        def block_pos(b):
            return b * R0 + (b * rem + P - 1) // P

        def tile_at(o):
            q = o * P + ci if o < R0 else R0 * P + (ci * rem + P - 1) // P
            nbi, rest = q % ngroup, q // ngroup
            mbl, ng = rest % rb, rest // rb
            return mbl * 8 + xcd, ng * ngroup + nbi

        block_tiles = block_pos(ci + 1) - block_pos(ci)
        o = chunk * chunk_tiles
        ntiles = min(o + chunk_tiles, block_tiles)
        if o >= ntiles:
            idle += 1
            continue
        tiles = [tile_at(t) for t in range(o, ntiles)]
        per_wg.append(len(tiles))
        for i, (mb, nb) in enumerate(tiles):
            cover[(mb, nb)] += 1
            if mb * GBM + GBM > M and i + 1 < len(tiles):
                ragged_followed += 1
    return Schedule(kernel, grid, P, chunks, ngroup, idle, per_wg, ragged_followed, cover, mblocks, tiles_n)


def covers_every_tile_once(s: Schedule) -> bool:
    want = {(mb, nb) for mb in range(s.mblocks) for nb in range(s.tiles_n)}
    return set(s.coverage) == want and all(v == 1 for v in s.coverage.values())


# ------------------------------------------------------------------------------------------------------------------
# inputs (CPU generators; PAD rows behind M for the ragged-row test)
# ------------------------------------------------------------------------------------------------------------------
PAD = 256
SENTINEL = 0x7FC1          # a quiet-NaN bf16 payload no kernel produces


def random_inputs(M: int, N: int, K: int):
    """x [M, K], w [N, K] / sqrt(K), bias [N], dy [M, K] * 0.1: bf16, standard normal (CPU tensors)"""
    g = torch.Generator().manual_seed(1_000_003 * M + 1009 * N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, generator=g).bfloat16()
    dy = (torch.randn(M, K, generator=g) * 0.1).bfloat16()
    return x, w, b, dy


MAX_ROW_NONZEROS = 240
MAX_BIAS = 8


def integer_inputs(M: int, N: int, K: int):
    """x, w from {-1, 0, 1}, bias integer in [-8, 8] (bf16, CPU tensors); x[m, m % K] = w[n, n % K] = 1, then every row of
    w thinned at random to at most 240 non-zeros: every partial sum of x w^T + bias is an integer of magnitude <= 248,
    exact in fp32 in any order and a bf16 number."""
    g = torch.Generator().manual_seed(7_000_003 * M + 4001 * N + K + 1)
    x = torch.randint(-1, 2, (M, K), generator=g, dtype=torch.int8)
    w = torch.randint(-1, 2, (N, K), generator=g, dtype=torch.int8)
    x[torch.arange(M), torch.arange(M) % K] = 1
    w[torch.arange(N), torch.arange(N) % K] = 1
    if K > MAX_ROW_NONZEROS:
        # keep the 240 non-zeros of a row with the smallest random keys (spread over all K steps, not a prefix)
        keys = torch.rand(N, K, generator=g)
        keys[w == 0] = 2.0
        cut = keys.sort(dim=1).values[:, MAX_ROW_NONZEROS - 1:MAX_ROW_NONZEROS]
        w[keys > cut] = 0
    b = torch.randint(-MAX_BIAS, MAX_BIAS + 1, (N,), generator=g, dtype=torch.int8)
    return x.bfloat16(), w.bfloat16(), b.bfloat16()

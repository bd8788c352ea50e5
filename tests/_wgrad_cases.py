"""Case list and bookkeeping of tests/test_wgrad_paths_gpu.py.

A plain-Python mirror of the HOST arithmetic of csrc/vit_gemm.hip -- ``wgrad_dispatch``, ``wgrad192_applies``,
``wgrad192_slices``, ``wgrad192_workspace_bytes``, ``launch_wgrad<KT>``, ``launch_wgrad192`` -- and of the slice loop of
``wgrad192_reduce_kernel``.  It MUST be updated together with that file.  It says which kernel and which slice split a
case reaches, so that the case list cannot drift into shapes that no longer take the paths they are there for; it is
bookkeeping for the GPU cases, not evidence about the kernels.

Also the input builders of the GPU tests (CPU generators, so that the same case has the same inputs everywhere and the
integer regime's exactness condition can be checked without a GPU), the fp64 reference and the CPU emulation the
tolerance of the real regime is derived from.
"""
from __future__ import annotations

import collections

import torch

WG_TN, WG_MC = 64, 64                    # register kernel: output rows per workgroup, m rows per chunk
W2_T, W2_MC, W2_SG = 192, 64, 8          # ring kernel: tile edge, m rows per chunk, slice groups of the reduction
RING_MIN_M = 4096

# ------------------------------------------------------------------------------------------------------------------
# the cases: (M, N, K), with the reason each one is there (asserted in test_wgrad_cases_cpu.py)
# ------------------------------------------------------------------------------------------------------------------
REGISTER_CASES = [
    (1, 64, 64),          # KT = 4, one row, one slice, 7 idle workgroups in the only group
    (65, 64, 128),        # KT = 8, two slices, the second holds one row
    (333, 128, 192),      # KT = 12, 6 slices of 64 rows, the last holds 13 rows
    (130, 64, 320),       # K % 128 != 0: KT = 4 with tk = 5; the bias comes from the by == 0 tile only
    (130, 128, 256),      # KT = 8 with tk = 2
    (130, 64, 384),       # KT = 12 with tk = 2
    (2000, 768, 768),     # M < 4096 keeps it off the ring; 8 slices of 256 rows = 4 chunks (the prefetch loop); the
                          # last slice has 208 rows, its last chunk 16
    (200, 1536, 1600),    # 600 tiles > 512: slices clamps to 1, one workgroup walks all 4 chunks
    (4097, 192, 192),     # a single 192 x 192 tile stays on the register kernel; 65 slices = 9 groups, 7 idle slices
    (4095, 384, 192),     # one row under the ring's M threshold
]
RING_CASES = [
    (4096, 192, 384),     # smallest ring shape; tn = 1, tk = 2: the k0 != 0 tile adds no bias; 64 slices of ONE chunk
    (4096, 384, 192),     # tn = 2, tk = 1: both tiles add bias
    (8192, 384, 384),     # 64 slices of two chunks: `more` is never true
    (12288, 384, 384),    # three chunks: the first refill of a stage
    (4096, 768, 768),     # 16 tiles, 16 slices, 4 chunks: the ring wraps
    (5120, 768, 768),     # 5 chunks per slice
    (4224, 768, 768),     # rows_per_slice 320: 14 slices, the last of 64 rows, 2 idle slices in the second group;
                          # reduce groups 0..5 add two slices, 6..7 one
    (4133, 192, 384),     # 37 tail rows go to launch_wgrad<12> through offset pointers; workspace sized from 4096
    (4096, 1152, 1152),   # 36 tiles: 7 slices < the reduce's 8 groups, one group adds nothing; shorter last slab
    (8192, 192, 384),     # 128 slices: 16 per reduce group, the two-at-a-time loop runs 8 times
]
ALL_CASES = REGISTER_CASES + RING_CASES
# parts 3 and 4 of the GPU tests
NO_BIAS_REGISTER_CASES = [(1, 64, 64), (65, 64, 128), (333, 128, 192)]          # one per KT
NO_BIAS_RING_CASES = [(4096, 192, 384), (4133, 192, 384)]
PYTHON_ENTRY_CASES = [(333, 128, 192), (4224, 768, 768), (4133, 192, 384)]     # register, ring, tail rows
BACK_TO_BACK = [(8192, 192, 384), (4096, 1152, 1152)]                          # the one with more slices first


def case_id(case) -> str:
    return "x".join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------------------------
# mirror of the launchers (csrc/vit_gemm.hip)
# ------------------------------------------------------------------------------------------------------------------
Launch = collections.namedtuple(
    "Launch", "kernel kt tn tk tiles slices rows_per_slice chunks rows grid idle row0 M")
Plan = collections.namedtuple("Plan", "kernel main tail tail_rows workspace_bytes reduce_adds")


def _split(M: int, budget: int, mc: int):
    """the slice arithmetic shared by launch_wgrad<KT> (budget 512 / tiles) and wgrad192_slices (256 / tiles)"""
    max_slices = (M + mc - 1) // mc
    slices = min(max(budget, 1), max_slices)
    rps = (M + slices - 1) // slices
    rps = (rps + mc - 1) // mc * mc
    return (M + rps - 1) // rps, rps


def _launch(kernel: str, kt: int, M: int, tn: int, tk: int, budget: int, row0: int) -> Launch:
    tiles = tn * tk
    slices, rps = _split(M, budget // tiles, WG_MC)
    groups = (slices + 7) // 8
    rows = [min((s + 1) * rps, M) - s * rps for s in range(slices)]
    chunks = [(r + WG_MC - 1) // WG_MC for r in rows]
    return Launch(kernel, kt, tn, tk, tiles, slices, rps, chunks, rows, groups * tiles * 8,
                  (groups * 8 - slices) * tiles, row0, M)


def launch_wgrad(kt: int, M: int, N: int, K: int, row0: int = 0) -> Launch:
    return _launch(f"reg{kt}", kt, M, N // WG_TN, K // (16 * kt), 512, row0)


def wgrad192_applies(M: int, N: int, K: int) -> bool:
    return N % W2_T == 0 and K % W2_T == 0 and M >= RING_MIN_M and (N // W2_T) * (K // W2_T) >= 2


def wgrad192_workspace_bytes(M: int, N: int, K: int) -> int:
    if not wgrad192_applies(M, N, K):
        return 0
    tiles = (N // W2_T) * (K // W2_T)
    slices, _rps = _split(M // W2_MC * W2_MC, 256 // tiles, W2_MC)
    return tiles * slices * W2_T * W2_T * 4


def reduce_adds(slices: int):
    """how many partial tiles each of the reduce kernel's 8 slice groups adds (its own loop, literally)"""
    out = []
    for g in range(W2_SG):
        n, sl = 0, g
        while sl + W2_SG < slices:
            n, sl = n + 2, sl + 2 * W2_SG
        if sl < slices:
            n += 1
        out.append(n)
    return out


def reduce_pair_iterations(slices: int) -> int:
    """trips of the reduce kernel's two-at-a-time loop in slice group 0"""
    n, sl = 0, 0
    while sl + W2_SG < slices:
        n, sl = n + 1, sl + 2 * W2_SG
    return n


def plan(M: int, N: int, K: int) -> Plan:
    """what wgrad_dispatch launches for a legal shape"""
    assert M > 0 and N % WG_TN == 0 and K % 64 == 0 and N >= WG_TN and K >= 64
    if wgrad192_applies(M, N, K):
        Mr = M // W2_MC * W2_MC
        tail = launch_wgrad(12, M - Mr, N, K, row0=Mr) if M > Mr else None
        main = _launch("ring", 0, Mr, N // W2_T, K // W2_T, 256, 0)
        return Plan("ring", main, tail, M - Mr, wgrad192_workspace_bytes(M, N, K), reduce_adds(main.slices))
    kt = 12 if K % 192 == 0 else 8 if K % 128 == 0 else 4
    return Plan(f"reg{kt}", launch_wgrad(kt, M, N, K), None, 0, 0, None)


def locate(p: Plan, n: int, k: int) -> str:
    """the tile and the wave that produce dw[n, k], for the mismatch report (C/D layouts of the two kernels)"""
    def reg(L):
        tkw = 16 * L.kt
        return (f"register kernel KT={L.kt}: tile (bx {n // WG_TN}, by {k // tkw}) = tile id "
                f"{(k // tkw) * L.tn + n // WG_TN}, wave {(k % tkw) // 16 // (L.kt // 4)}, {L.slices} slices of "
                f"{L.rows_per_slice} rows from row {L.row0}")
    if p.kernel != "ring":
        return reg(p.main)
    L = p.main
    txt = (f"ring kernel: tile (n {n // W2_T}, k {k // W2_T}) = tile id {(k // W2_T) * L.tn + n // W2_T}, wave "
           f"{(n % W2_T) // 48 * 2 + (k % W2_T) // 96} (wn {(n % W2_T) // 48}, wk {(k % W2_T) // 96}), {L.slices} slices "
           f"of {L.rows_per_slice} rows, reduce groups add {p.reduce_adds}")
    return txt + (f"; tail rows: {reg(p.tail)}" if p.tail is not None else "")


# ------------------------------------------------------------------------------------------------------------------
# inputs (CPU generators)
# ------------------------------------------------------------------------------------------------------------------
INT_DY, INT_X, INT_INIT = 2, 4, 1024           # |dY| <= 2, |X| <= 4, |dw0|, |db0| <= 1024
EXACT_LIMIT = 1 << 24


def integer_inputs(M: int, N: int, K: int):
    """dy [M, N] integers in [-2, 2], x [M, K] integers in [-4, 4] (bf16), dw0 [N, K], db0 [N] integer-valued fp32 in
    [-1024, 1024].  Every product and every partial sum, in any order, is an integer of magnitude <= 8 M + 1024 < 2^24:
    fp32 accumulation, the MFMA, the atomics and the reduce are all exact, so the result EQUALS dw0 + dy^T x."""
    g = torch.Generator().manual_seed(5_000_011 * M + 3001 * N + K + 7)
    dy = torch.randint(-INT_DY, INT_DY + 1, (M, N), generator=g, dtype=torch.int8).bfloat16()
    x = torch.randint(-INT_X, INT_X + 1, (M, K), generator=g, dtype=torch.int8).bfloat16()
    dw0 = torch.randint(-INT_INIT, INT_INIT + 1, (N, K), generator=g, dtype=torch.int32).float()
    db0 = torch.randint(-INT_INIT, INT_INIT + 1, (N,), generator=g, dtype=torch.int32).float()
    return dy, x, dw0, db0


TINY = 1e-30


def real_inputs(M: int, N: int, K: int):
    """x ~ N(0, 1), dy ~ N(0, 1) * 10^u with u uniform in [-6, -2] per row (the dynamic range of trained gradients),
    both rounded to bf16; no value below 1e-30 in magnitude (nothing subnormal in bf16)"""
    g = torch.Generator().manual_seed(9_000_011 * M + 6007 * N + K + 3)
    x = torch.randn(M, K, generator=g)
    u = torch.rand(M, 1, generator=g) * 4.0 - 6.0
    dy = torch.randn(M, N, generator=g) * torch.pow(torch.full_like(u, 10.0), u)
    out = []
    for t in (dy, x):
        t = torch.where(t.abs() < TINY, torch.where(t < 0, -TINY, TINY).to(t.dtype), t)
        out.append(t.bfloat16())
    return out[0], out[1]


def reference(dy, x, dw0=None, db0=None):
    """dw0 + dy^T x and db0 + colsum(dy) in fp64 from the bf16 values (exact in the integer regime: every term and
    every sum is an integer far below 2^53)"""
    dyd = dy.double()
    dw, db = dyd.t() @ x.double(), dyd.sum(0)
    if dw0 is not None:
        dw = dw + dw0.double()
    if db0 is not None:
        db = db + db0.double()
    return dw, db


def magnitude(dy, x):
    """|dy|^T |x| and the column sums of |dy| in fp64: what the per-element tolerance of the real regime scales with"""
    a = dy.double().abs()
    return a.t() @ x.double().abs(), a.sum(0)


def emulate(dy, x, launch: Launch):
    """The kernels' arithmetic at the granularity the host code fixes: an fp32 product per 64-row chunk, the chunks of
    a slice added in fp32 in order, the slices added in fp32 in slice order.  (Inside a chunk the order is the CPU
    matmul's, not the MFMA's, and the atomics' order is not the slice order: what the 4x margin of TOL covers.)"""
    N, K = dy.shape[1], x.shape[1]
    dw, db = torch.zeros(N, K), torch.zeros(N)
    dyf, xf = dy.float(), x.float()
    r0 = launch.row0
    for rows in launch.rows:
        sw, sb = torch.zeros(N, K), torch.zeros(N)
        for c0 in range(r0, r0 + rows, WG_MC):
            c1 = min(c0 + WG_MC, r0 + rows)
            sw += dyf[c0:c1].t() @ xf[c0:c1]
            sb += dyf[c0:c1].sum(0)
        dw += sw
        db += sb
        r0 += rows
    return dw, db


def emulate_plan(dy, x, p: Plan):
    dw, db = emulate(dy, x, p.main)
    if p.tail is not None:
        tw, tb = emulate(dy, x, p.tail)
        dw, db = dw + tw, db + tb
    return dw, db


def worst_ratio(got_w, got_b, ref_w, ref_b, mag_w, mag_b):
    """max over the elements of |got - ref| / magnitude, for dw and for db (an exact element passes a zero magnitude)"""
    out = []
    for got, ref, mag in ((got_w, ref_w, mag_w), (got_b, ref_b, mag_b)):
        err = (got.double() - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / mag)
        out.append(float(ratio.max()) if not bool(torch.isnan(ratio).any()) else float("nan"))
    return out[0], out[1]


# The worst per-element ratio of ``emulate_plan`` against the fp64 reference over ALL_CASES with ``real_inputs``, measured
# on a CPU (profiles/wgrad_margins.txt has it per case).  TOL is four times that: the kernels sum the same exact products
# in fp32 in another order (the MFMA's internal tree, the atomics), so their error has the same order.  It is a
# measurement of the reference's own error, never of the kernels; the per-case cap M 2^-23 is the first-order worst case
# of M fp32 additions (one rounding of relative size 2^-24 per addition on partial sums bounded by the magnitude, times
# two for the 64-row products).
EMUL_WORST_RATIO = 2.66e-7           # at (65, 64, 128); 3.9e-8 .. 2.7e-7 per case
TOL = 4.0 * EMUL_WORST_RATIO


def tolerance(M: int) -> float:
    return min(TOL, M * 2.0 ** -23)

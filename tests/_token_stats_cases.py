"""Case list, launcher mirror, inputs and bounds of tests/test_token_stats_gpu.py.

A plain-Python mirror of the HOST arithmetic of csrc/token_gram.hip -- ``basd_token_gram`` (template from dtype and
d_out, grid, grid-stride trips, ragged last tile), ``launch_tg_bf16x3`` (the switch to 256-row tiles, grid, trips, the
valid rows of each Gram pass), ``basd_gram_f32_centred`` (nbc, nblk, rsplit and its clamps, the row slices) -- and of
the routing of ``_native.token_gram``, which must be updated together with them.  It says which kernel a case launches,
on how many workgroups and in how many loop trips, so that the case list cannot drift into shapes that no longer take
the paths they are there for (pinned by tests/test_token_stats_cases_cpu.py); it is bookkeeping for the GPU cases, not
evidence about the kernels.

Also the input builders (CPU generators: the same case has the same inputs everywhere), a CPU emulation of the
arithmetic of each path (fp32 torch products; the three-term bf16 split; the tile-centred fp32 Gram) and the error
bounds.  The bounds take any device and work in fp64; tests/test_token_stats_cases_cpu.py applies them to the emulation
and to wrong variants of it, tests/test_token_stats_gpu.py to the kernels.
"""
from __future__ import annotations

import collections

import torch

# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
F32, BF16 = "f32", "bf16"
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
DTYPE_CODE = {F32: 0, BF16: 1}
TM, TM2, GW_TR, GW_BC, CAP = 64, 128, 64, 128, 256      # generic tile, bf16x3 tile / pass, wide tile, wide panel, grid cap
GUARD = 64                                               # fp64 elements behind gram and behind colsum

# kind: generic | bf16x3 | wide (basd_gram_f32_centred: d_in = 0, d_out = d) | route (through _native.token_gram)
# view: None or (B, T): the rows are x[:, 1:, :] of a [B, T, d_in] buffer;  proj: qr | binades
Case = collections.namedtuple("Case", "kind dtype rows d_in d_out view proj")


def _c(kind, dtype, rows, d_in, d_out, view=None, proj="qr"):
    return Case(kind, dtype, rows, d_in, d_out, view, proj)


def case_id(case: Case) -> str:
    s = f"{case.kind}-{case.dtype}-{case.rows}x{case.d_in}-{case.d_out}"
    if case.view:
        s += f"-view{case.view[0]}x{case.view[1]}"
    return s + ("" if case.proj == "qr" else "-" + case.proj)


GEN_DOUT = [16, 48, 192, 208, 240, 256]       # 1, 3, 12 | 13, 15, 16 column tiles: both sides of the 10 / 17 switch
GEN_ROWS = [1, 63, 64, 65, 200]
GEN_WRAP_ROWS = 16384 + 64 + 37               # 258 tiles on 256 workgroups, the very last one ragged
GENERIC_CASES = ([_c("generic", dt, rows, 32, d_out) for dt in (F32, BF16) for d_out in GEN_DOUT for rows in GEN_ROWS]
                 + [_c("generic", dt, 200, d_in, d_out) for dt in (F32, BF16) for d_in in (64, 96) for d_out in (48, 240)])
GENERIC_WRAP = [_c("generic", dt, GEN_WRAP_ROWS, 32, d_out) for dt in (F32, BF16) for d_out in (48, 240)]

X3_DOUT = [32, 64, 128, 192]                  # NCT 2, 4, 8, 12
T128_ROWS = [1, 127, 128, 129, 300]
T128_LAST = 32768                             # 256 tiles of 128: the last size on the 128-row kernel
T128_CASES = ([_c("bf16x3", BF16, rows, 32, d_out) for d_out in X3_DOUT for rows in T128_ROWS]
              + [_c("bf16x3", BF16, 300, d_in, d_out) for d_out in X3_DOUT for d_in in (64, 96, 160)]
              + [_c("bf16x3", BF16, T128_LAST, 32, d_out) for d_out in X3_DOUT]
              + [_c("bf16x3", BF16, 300, 64, 64, proj="binades")])
T256_ROWS = [32768 + 1, 32768 + 128, 32768 + 128 + 5, 32768 + 256]      # pass 1 skipped, exactly empty, partial, full
T256_WRAP_ROWS = 65536 + 256 + 41             # 258 tiles on 256 workgroups, the last one ragged in pass 0
T256_CASES = ([_c("bf16x3", BF16, rows, 32, d_out) for d_out in X3_DOUT for rows in T256_ROWS + [T256_WRAP_ROWS]]
              + [_c("bf16x3", BF16, rows, 96, 192) for rows in T256_ROWS + [T256_WRAP_ROWS]])

# T - 1 = 50 and 196 are no multiples of 16: 16-row fragments and tiles straddle batches
VIEW_CASES = [_c("bf16x3", BF16, 3 * 50, 32, 64, view=(3, 51)), _c("bf16x3", BF16, 169 * 196, 32, 192, view=(169, 197)),
              _c("generic", F32, 3 * 50, 32, 48, view=(3, 51)), _c("generic", BF16, 3 * 50, 32, 48, view=(3, 51))]

# basd_gram_f32_centred: rsplit 1 (ntile / 8 = 0; 512 / nblk = 0 at d = 4096), rsplit = ntile / 8 = 3 of 25 tiles (the
# slices hold 8, 8 and 9), a last tile of one row (1537 = 24 * 64 + 1, 129 = 2 * 64 + 1)
WIDE_CASES = [_c("wide", F32, rows, 0, d) for rows, d in
              ((70, 16), (1537, 16), (200, 144), (1537, 144), (129, 400), (1537, 400), (70, 4096))]

ROUTE_CASES = [(_c("route", BF16, 300, 64, 64), ("bf16x3",)),
               (_c("route", F32, 300, 64, 48), ("generic",)),
               (_c("route", BF16, 300, 64, 208), ("generic",)),
               (_c("route", BF16, 1800, 128, 272), ("wide", "gemm_bf16x3", "centred")),
               (_c("route", BF16, 1800, 128, 264), ("wide", "gemm_bf16x3", "splitk")),
               (_c("route", F32, 300, 64, 272), ("wide", "bgemm_f64", "centred")),
               (_c("route", BF16, 300, 48, 32), ("wide", "bgemm_f64", "centred")),
               (_c("route", BF16, 300, 64, 40), ("wide", "bgemm_f64", "splitk"))]

DIRECT_CASES = GENERIC_CASES + GENERIC_WRAP + T128_CASES + T256_CASES + VIEW_CASES + WIDE_CASES

REGIMES = ["plain", "offset", "marked", "one_hot"]


def regimes(case: Case):
    """one_hot is about the projection; basd_gram_f32_centred has none"""
    return REGIMES[:3] if case.kind == "wide" else REGIMES


# ------------------------------------------------------------------------------------------------------------------
# mirror of the launchers (csrc/token_gram.hip) and of _native.token_gram
# ------------------------------------------------------------------------------------------------------------------
def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b


GenericLaunch = collections.namedtuple("GenericLaunch", "template grid ntiles trips last_valid nct halves ngt lds atomics")


def generic_launch(dtype: str, rows: int, d_in: int, d_out: int) -> GenericLaunch:
    """basd_token_gram: token_gram_kernel<T, 10 | 17>, 64-row tiles on min(ntiles, 256) workgroups"""
    assert rows > 0 and d_out % 16 == 0 and 16 <= d_out <= 256 and d_in % 32 == 0 and d_in >= 32
    ntiles = _ceil(rows, TM)
    grid = min(ntiles, CAP)
    nct = d_out // 16
    half = (nct + 1) // 2                          # column tiles of waves 0-3; waves 4-7 own the rest
    lds = (TM * 34 + d_out * 34 + TM * (d_out + 16)) * 4
    return GenericLaunch((dtype, 10 if d_out <= 192 else 17), grid, ntiles, _ceil(ntiles, grid),
                         rows - (ntiles - 1) * TM, nct, (half, nct - half), nct * (nct + 1) // 2, lds, grid)


X3Launch = collections.namedtuple("X3Launch", "kernel nct grid ntiles trips chunks last shape atomics")


def bf16x3_launch(rows: int, d_in: int, d_out: int) -> X3Launch:
    """launch_tg_bf16x3<NCT>: 128-row tiles, or 256-row tiles with two 128-row Gram passes once ceil(rows / 128) > 256.
    last = (valid rows of pass 0, of pass 1 | None where it is skipped) of the last tile; shape names it (t256);
    atomics = additions into one Gram element: one per workgroup (t128), one per TILE (t256 flushes every tile)"""
    assert rows > 0 and d_out in X3_DOUT and d_in % 32 == 0 and d_in >= 32
    nt = _ceil(rows, TM2)
    if nt > CAP:
        nt2 = _ceil(rows, 2 * TM2)
        grid = min(nt2, CAP)
        rem = rows - (nt2 - 1) * 2 * TM2
        last = (min(rem, TM2), None if rem <= TM2 else rem - TM2)
        shape = "skipped" if rem < TM2 else "empty" if rem == TM2 else "partial" if rem < 2 * TM2 else "full"
        return X3Launch("t256", d_out // 16, grid, nt2, _ceil(nt2, grid), d_in // 32, last, shape, nt2)
    grid = min(nt, CAP)
    return X3Launch("t128", d_out // 16, grid, nt, _ceil(nt, grid), d_in // 32, (rows - (nt - 1) * TM2, None), None, grid)


WideLaunch = collections.namedtuple("WideLaunch", "nbc nblk ntile rsplit slices grid atomics")


def wide_launch(rows: int, d: int) -> WideLaunch:
    """basd_gram_f32_centred: nblk 128 x 128 blocks of the lower block triangle times rsplit row slices"""
    assert rows > 0 and d % 16 == 0 and 16 <= d <= 4096
    nbc = _ceil(d, GW_BC)
    nblk = nbc * (nbc + 1) // 2
    ntile = _ceil(rows, GW_TR)
    rsplit = max(1, min(512 // nblk, ntile // 8))
    slices = [(ntile * rs // rsplit, ntile * (rs + 1) // rsplit) for rs in range(rsplit)]
    return WideLaunch(nbc, nblk, ntile, rsplit, slices, nblk * rsplit, rsplit)


def gemm_bf16x3_f32_supported(m: int, n: int, k: int) -> bool:
    return m > 7 * 256 and k % 64 == 0 and k >= 128 and n % 8 == 0


def route(dtype: str, rows: int, d_in: int, d_out: int):
    """what _native.token_gram launches for a [rows, d_in] matrix of ``dtype``"""
    if d_out > 256 or d_out % 16 or d_in % 32:
        z = "gemm_bf16x3" if dtype == BF16 and gemm_bf16x3_f32_supported(rows, d_out, d_in) else "bgemm_f64"
        return ("wide", z, "centred" if d_out % 16 == 0 else "splitk")
    if dtype == BF16 and d_out in X3_DOUT:
        return ("bf16x3",)
    return ("generic",)


def launch_of(case: Case):
    if case.kind == "generic":
        return generic_launch(case.dtype, case.rows, case.d_in, case.d_out)
    if case.kind == "bf16x3":
        return bf16x3_launch(case.rows, case.d_in, case.d_out)
    assert case.kind == "wide"
    return wide_launch(case.rows, case.d_out)


def path_of(case: Case) -> str:
    """the kernel template a direct case reaches, as the margins file and the summary name it"""
    la = launch_of(case)
    if case.kind == "generic":
        return f"token_gram_kernel<{la.template[0]},{la.template[1]}>"
    if case.kind == "bf16x3":
        return f"token_gram_bf16x3{'_t256' if la.kernel == 't256' else ''}_kernel<{la.nct}>"
    return "gram_wide_f32_kernel"


def rows_visited(case: Case) -> collections.Counter:
    """row -> how many (workgroup, trip, wave, fragment row) stage it AND feed it to a Gram pass: the kernels' loops,
    walked (wide: the workgroups of block 0, whose slices together own every tile)"""
    rows = case.rows
    seen = collections.Counter()
    la = launch_of(case)
    if case.kind == "generic":
        for block in range(la.grid):
            for tile in range(block, la.ntiles, la.grid):
                for r in range(TM):
                    if tile * TM + r < rows:
                        seen[tile * TM + r] += 1
    elif case.kind == "bf16x3" and la.kernel == "t128":
        for block in range(la.grid):
            for tile in range(block, la.ntiles, la.grid):
                for wave in range(4):
                    for g in range(2):
                        for l in range(16):
                            r = tile * TM2 + wave * 32 + g * 16 + l
                            if r < rows:
                                seen[r] += 1
    elif case.kind == "bf16x3":
        for block in range(la.grid):
            for tile in range(block, la.ntiles, la.grid):
                for g in range(4):
                    if rows - (tile * 2 * TM2 + (g >> 1) * TM2) <= 0:          # the pass of this row group is skipped
                        continue
                    for wave in range(4):
                        for l in range(16):
                            r = tile * 2 * TM2 + (g >> 1) * TM2 + wave * 32 + (g & 1) * 16 + l
                            if r < rows:
                                seen[r] += 1
    else:
        for t_lo, t_hi in la.slices:
            for tile in range(t_lo, t_hi):
                for r in range(GW_TR):
                    if tile * GW_TR + r < rows:
                        seen[tile * GW_TR + r] += 1
    return seen


def view_offset(r: int, rows_per_batch: int, batch_stride: int, d_in: int) -> int:
    """element offset of logical row r from x, as every kernel computes it"""
    b = r // rows_per_batch
    return b * batch_stride + (r - b * rows_per_batch) * d_in


def view_args(case: Case):
    """(rows_per_batch, batch_stride) a launch of the case passes"""
    if case.view:
        _b, t = case.view
        return t - 1, t * case.d_in
    return case.rows, 0


def chunk_rows(case: Case):
    """rows whose fp32 products are summed before fp64 takes over: a Gram pass (bf16x3), a tile (wide); None: fp64"""
    return {"generic": None, "bf16x3": TM2, "wide": GW_TR}[case.kind]


def boundary_rows(case: Case):
    """first rows of the tiles / passes behind the first and of the batches behind the first"""
    step = {"generic": TM, "bf16x3": TM2, "wide": GW_TR, "route": TM}[case.kind]
    b = set(range(step, case.rows, step))
    if case.view:
        b |= set(range(case.view[1] - 1, case.rows, case.view[1] - 1))
    return sorted(b)


def marked_rows(case: Case):
    """the rows at risk: row 0, the last row, and the rows on either side of every boundary"""
    s = {0, case.rows - 1}
    for b in boundary_rows(case):
        s |= {b - 1, b}
    return sorted(s)


# ------------------------------------------------------------------------------------------------------------------
# inputs (CPU tensors, seeded generators)
# ------------------------------------------------------------------------------------------------------------------
MARK = 8.0
OFFSET = 30.0
POISON = 777.0            # the CLS slot of a strided buffer: a kernel that reads it is off by more than any bound


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1_000_003 + int(k) + 17) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


def projection(case: Case) -> torch.Tensor:
    """fp32 [d_out, d_in]: orthonormal rows (d_out <= d_in) or columns from a QR; ``binades``: every entry times
    2^k, k in -3 .. 3"""
    g = _gen(case.d_in, case.d_out, 7)
    if case.d_out <= case.d_in:
        p = torch.linalg.qr(torch.randn(case.d_in, case.d_out, generator=g))[0].T.contiguous()
    else:
        p = torch.linalg.qr(torch.randn(case.d_out, case.d_in, generator=g))[0].contiguous()
    if case.proj == "binades":
        p = p * torch.exp2(torch.randint(-3, 4, p.shape, generator=g).float())
    return p.float().contiguous()


def tokens(case: Case, regime: str) -> torch.Tensor:
    """the logical [rows, d_in] matrix: bf16-exact values in the case's dtype (wide: fp32 [rows, d], any fp32 values).
    plain: randn.  offset: randn + 30 o with o of N(0, 1)-sized entries: the column means are 30 x the spread; o lies
    along the first row of P (o = sqrt(d_in) P[0] / |P[0]|) so that column 0 of z carries the whole offset, the regime
    the per-tile centring exists for.  marked: plain, the rows of ``marked_rows`` replaced by 8 x a sign pattern of
    their own.  one_hot: each row a single 1.0."""
    rows, d = case.rows, (case.d_out if case.kind == "wide" else case.d_in)
    g = _gen(rows, d, case.d_out, REGIMES.index(regime))
    if regime == "one_hot":
        x = torch.zeros(rows, d)
        x[torch.arange(rows), torch.randint(0, d, (rows,), generator=g)] = 1.0
    else:
        x = torch.randn(rows, d, generator=g)
    if regime == "offset":
        if case.kind == "wide":
            o = torch.randn(1, d, generator=g)
        else:
            p0 = projection(case)[0]
            o = (d ** 0.5 * p0 / p0.norm()).view(1, d)
        x = x + OFFSET * o
    if regime == "marked":
        at = torch.tensor(marked_rows(case))
        x[at] = MARK * (1.0 - 2.0 * torch.randint(0, 2, (len(at), d), generator=g).float())
    if case.kind == "wide":
        return x.float()
    return x.bfloat16().to(TORCH_DTYPE[case.dtype])


def view_buffer(case: Case, x: torch.Tensor) -> torch.Tensor:
    """[B, T, d_in] with x in [:, 1:, :] and POISON in the CLS slots"""
    b, t = case.view
    buf = torch.full((b, t, case.d_in), POISON, dtype=x.dtype)
    buf[:, 1:, :] = x.view(b, t - 1, case.d_in)
    return buf


def prefill(d: int):
    """what gram [d * d + GUARD] and colsum [d + GUARD] hold before a launch: fp64 values between 0.5 and 1.5"""
    i = torch.arange(d * d + GUARD, dtype=torch.float64)
    j = torch.arange(d + GUARD, dtype=torch.float64)
    return 0.5 + (i * 7 % 11) / 11.0 + (i % 5) * 2.0 ** -40, 0.5 + (j * 3 % 7) / 7.0 + (j % 3) * 2.0 ** -40


def lower_tiles(d: int, device=None) -> torch.Tensor:
    """bool [d, d]: the 16 x 16 tiles on and below the diagonal, all a launch may touch"""
    t = torch.arange(d, device=device) // 16
    return t.view(-1, 1) >= t.view(1, -1)


# ------------------------------------------------------------------------------------------------------------------
# emulation of the arithmetic of each path (CPU, torch products)
# ------------------------------------------------------------------------------------------------------------------
def split3(p: torch.Tensor):
    """fp32 -> (hi, mid, lo) bf16, each the bf16 rounding of what the ones before leave (_native.split_bf16x3)"""
    hi = p.bfloat16()
    r1 = p - hi.float()
    mid = r1.bfloat16()
    return hi, mid, (r1 - mid.float()).bfloat16()


def emulate_z(x: torch.Tensor, p: torch.Tensor, accum: str, drop_lo: bool = False) -> torch.Tensor:
    """fp32 z = x p^T with the accumulation of a path: mfma32 (one fp32 product), split3 (three products over the bf16
    split of p, summed in fp32), bgemm (fp64, rounded to fp32 once)"""
    xf = x.float()
    if accum == "mfma32":
        return xf @ p.T
    if accum == "bgemm":
        return (x.double() @ p.double().T).float()
    hi, mid, lo = split3(p)
    z = xf @ hi.float().T + xf @ mid.float().T
    return z if drop_lo else z + xf @ lo.float().T


def emulate_stats(z: torch.Tensor, chunk, variant: str = ""):
    """(gram, colsum) fp64 from fp32 z.  chunk None: fp64 throughout.  Else per ``chunk`` rows: s = fp64 column sums,
    mu = fp32(s / n), G_c = fp32 product of the centred rows, gram += G_c + mu w^T + w mu^T, w = s - (n / 2) mu.
    variant ``uncentred``: the fp32 product of the rows as they are; ``padded``: the zero rows that fill the last
    chunk are centred too (their column sums run over the padded height, not over the valid rows' values)"""
    if chunk is None:
        zd = z.double()
        return zd.T @ zd, zd.sum(0)
    rows, d = z.shape
    n = _ceil(rows, chunk)
    zp = torch.zeros(n * chunk, d, dtype=torch.float32)
    zp[:rows] = z
    zp = zp.view(n, chunk, d)
    cnt = torch.full((n, 1), float(chunk), dtype=torch.float64)
    cnt[-1] = rows - (n - 1) * chunk
    s = zp.double().sum(1)
    if variant == "uncentred":
        return torch.bmm(zp.transpose(1, 2), zp).double().sum(0), s.sum(0)
    mu = (s / cnt).float()
    c = zp - mu.view(n, 1, d)
    if variant != "padded":
        c.view(n * chunk, d)[rows:] = 0.0
    w = s - 0.5 * cnt * mu.double()
    m = mu.double().T @ w
    return torch.bmm(c.transpose(1, 2), c).double().sum(0) + m + m.T, s.sum(0)


# ------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------
# u = 2^-24 is fp32's unit roundoff, v = 2^-53 fp64's.  Every bound is per element; results are err / bound.
#
# (1) z = X P^T.  The computed z^ = z + e with |e| <= E, E a [rows, d_out] matrix.  With A = |X| |P|^T and nnz the
#     number of non-zero entries of the row of X (adding an exact zero rounds nothing, in any order or tree):
#     mfma32  fp32 matrix cores over d_in: nnz products of an 8-bit by a 24-bit significand, each rounded, and nnz - 1
#             additions, in whatever order the hardware takes them: E = (nnz + 1) u A (nnz u A to first order, one
#             more u for the higher orders).
#     split3  P = hi + mid + lo + r with |r| <= 2^-27 |P| (each term the bf16 rounding of the remainder: 2^-9 each
#             time); the 3 nnz products of bf16 pairs are exact in fp32 and meet in 3 nnz - 1 rounded additions of
#             terms |x| (|hi| + |mid| + |lo|) <= |x| |p| (1 + 2^-8 + 2^-16): E = ((3 nnz - 1) u (1 + 2^-8 + 2^-16)
#             + 2^-27) A.  On a one-hot row that is 2 u |p|: two additions.
#     bgemm   an fp64 product rounded to fp32 once: E = u |z| + 4 nnz v A.
#     none    z is the input (basd_gram_f32_centred).
# (2) gram = sum_r z^ z^^T differs from the reference by sum_r (|e_ri| |z_rj| + |z_ri| |e_rj| + |e_ri| |e_rj|)
#     <= E^T |z| + |z|^T E + E^T E, whatever happens afterwards.
# (3) The Gram of z^.  generic path: fp32 z^ widened to fp64, products exact (48 bits), fp64 sums.  Centring paths,
#     per chunk T of n_T <= C rows (C = 128: a Gram pass of the bf16x3 kernels; 64: a tile of the wide kernel):
#     mu = fp32(s / n_T), c = fp32(z^ - mu) (one rounding), G_c = sum_T c c^T on the fp32 matrix cores: n_T rounded
#     products and n_T - 1 additions; the identity sum_T z^ z^^T = G_c + mu w^T + w mu^T is exact for ANY mu, so all
#     that is lost is (n_T + 3) u sum_T |c_i| |c_j| <= (C + 3) u sum_T |c_i| |c_j|  (2 u for the two roundings of c, n_T
#     for products and sums, one for the higher orders), with |c| <= |z - mean_T z| + u |mean_T z| + E + mean_T E:
#     the exact centred magnitude, the rounding of mu, and what e moves.  CENTRED magnitudes: this term is what keeps
#     unc - s s^T / m at fp32 accuracy of ITSELF; an fp32 Gram of the uncentred rows has |z_i| |z_j| in their place.
# (4) fp64.  Everything else is fp64 on partial sums no larger than sqrt(S_i S_j), S_i = sum_r (|z_ri| + E_ri)^2
#     (Cauchy-Schwarz; n mu_i^2 <= S_i covers the rank-1 terms): at most one operation per row (generic), eight per
#     chunk, and two per atomic addition (``atomics`` per element and launch, from the mirror), 64 to spare:
#     K v sqrt(S_i S_j), K = rows + 8 chunks + 2 atomics + 64.  The atomics also round what the buffer held:
#     + (atomics + 1) v |prefill| per launch (the + 1: the test's own subtraction of the prefill).
# (5) colsum = sum_r z^ in fp64: sum_r E_rc + K v sum_r (|z_rc| + E_rc) (+ the prefill term).
# (6) the centred Gram cen = gram - s s^T / m, formed in fp64 from (gram, colsum) the way the selector forms it, IS
#     the centred Gram of z^ up to (3) and (4): sum_r (z^ - mean z^)(z^ - mean z^)^T with z^ - mean z^ = (z - mean z)
#     + (e - mean e).  Its bound is (2) with centred factors -- Ec^T |c| + |c|^T Ec + Ec^T Ec, c = z - mean z over all
#     rows, Ec = E + mean E -- plus (3), plus 4 K v sqrt(S_i S_j) for the cancellation in fp64.  It is relative to the
#     centred Gram's own scale; the uncentred scale enters at fp64 level only.
U32 = 2.0 ** -24
U64 = 2.0 ** -53


def ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err / bound; an exact element passes a zero bound; a NaN fails"""
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    assert not bool(torch.isnan(q).any()), "NaN in an output"
    return float(q.max()) if q.numel() else 0.0


def z_error(x64: torch.Tensor, p64: torch.Tensor, z: torch.Tensor, accum: str) -> torch.Tensor:
    a = x64.abs() @ p64.abs().T
    nnz = (x64 != 0).sum(1, keepdim=True).double()
    if accum == "mfma32":
        return (nnz + 1.0) * U32 * a
    if accum == "split3":
        return ((3.0 * nnz - 1.0).clamp(min=0.0) * U32 * (1.0 + 2.0 ** -8 + 2.0 ** -16) + 2.0 ** -27) * a
    assert accum == "bgemm"
    return U32 * z.abs() + 4.0 * nnz * U64 * a


class Reference:
    """fp64 reference of gram, colsum and the centred Gram of one input, and the bounds (1) - (6) above"""

    def __init__(self, x, p, accum: str, chunk, atomics: int):
        xd = x.double()
        if accum == "none":
            z, e = xd, None
        else:
            z = xd @ p.double().T
            e = z_error(xd, p.double(), z, accum)
        rows, d = z.shape
        self.rows, self.d, self.atomics = rows, d, atomics
        az = z.abs()
        self.gram, self.colsum = z.T @ z, z.sum(0)
        self.centred = self.gram - torch.outer(self.colsum, self.colsum) / rows
        ze = az if e is None else az + e
        s = (ze * ze).sum(0)
        self.k64 = rows + 8 * (_ceil(rows, chunk) if chunk else 0) + 2 * atomics + 64
        self.sqrt_ss = torch.sqrt(torch.outer(s, s))
        acc32 = 0.0
        if chunk:
            n = _ceil(rows, chunk)
            pad = n * chunk - rows
            zp = torch.cat([z, z.new_zeros(pad, d)]).view(n, chunk, d)
            cnt = z.new_full((n, 1, 1), float(chunk))
            cnt[-1] = chunk - pad
            mean = zp.sum(1, keepdim=True) / cnt
            cp = (zp - mean).abs() + U32 * mean.abs()
            if e is not None:
                ep = torch.cat([e, e.new_zeros(pad, d)]).view(n, chunk, d)
                cp = cp + ep + ep.sum(1, keepdim=True) / cnt
            cp = cp.reshape(n * chunk, d)[:rows]
            acc32 = (chunk + 3) * U32 * (cp.T @ cp)
            del zp, cp
        self.gram_bound = acc32 + self.k64 * U64 * self.sqrt_ss
        self.colsum_fp64 = self.k64 * U64 * ze.sum(0)
        self.colsum_bound = self.colsum_fp64
        self.centred_bound = acc32 + 4 * self.k64 * U64 * self.sqrt_ss
        if e is not None:
            t = e.T @ (az + 0.5 * e)                   # t + t^T = E^T |z| + |z|^T E + E^T E
            self.gram_bound = self.gram_bound + t + t.T
            self.colsum_bound = self.colsum_bound + e.sum(0)
            c = (z - z.mean(0, keepdim=True)).abs()
            ec = e + e.mean(0, keepdim=True)
            t = ec.T @ (c + 0.5 * ec)
            self.centred_bound = self.centred_bound + t + t.T

    def ratios(self, gram_delta, colsum_delta, pre_gram=None, pre_colsum=None, launches: int = 1, centred: bool = True):
        """gram_delta [d, d] / colsum_delta [d]: what ``launches`` launches added to buffers that held pre_* (None: zeros).
        Only the lower 16 x 16 tiles of gram_delta are looked at.  -> {"gram", "colsum", "centred"}: max err / bound"""
        low = lower_tiles(self.d, gram_delta.device)
        n = launches
        pg = 0.0 if pre_gram is None else (n * self.atomics + 1) * U64 * (pre_gram.abs() + n * self.sqrt_ss)
        pc = 0.0 if pre_colsum is None else (n * self.atomics + 1) * U64 * (pre_colsum.abs() + n * self.colsum.abs())
        out = {"gram": ratio((gram_delta - n * self.gram).abs()[low], (n * self.gram_bound + pg)[low]),
               "colsum": ratio((colsum_delta - n * self.colsum).abs(), n * self.colsum_bound + pc)}
        if centred and n == 1:
            g = torch.tril(gram_delta) + torch.tril(gram_delta, -1).T
            cen = g - torch.outer(colsum_delta, colsum_delta) / self.rows
            sa = self.colsum.abs() + pc
            bound = self.centred_bound + pg + (torch.outer(sa, sa) - torch.outer(self.colsum.abs(), self.colsum.abs())) / self.rows
            out["centred"] = ratio((cen - self.centred).abs(), bound)
        return out


def accumulation(case: Case, routed=None) -> tuple:
    """(kind of z error, chunk) of a direct case, or of a route"""
    if case.kind == "generic" or routed == ("generic",):
        return "mfma32", None
    if case.kind == "bf16x3" or routed == ("bf16x3",):
        return "split3", TM2
    if case.kind == "wide":
        return "none", GW_TR
    return ("split3" if routed[1] == "gemm_bf16x3" else "bgemm"), (GW_TR if routed[2] == "centred" else None)


def reference(case: Case, x, p, routed=None) -> Reference:
    """x: the logical [rows, d_in] matrix (dense), p: the fp32 projection (None for wide), on any device"""
    accum, chunk = accumulation(case, routed)
    if routed is None:
        atomics = launch_of(case).atomics
    elif routed[0] == "wide":
        atomics = wide_launch(case.rows, case.d_out).atomics if routed[2] == "centred" else 64    # split-K: the slab sum
    else:
        atomics = (generic_launch if routed == ("generic",) else bf16x3_launch)(
            *((case.dtype,) if routed == ("generic",) else ()), case.rows, case.d_in, case.d_out).atomics
    return Reference(x, p, accum, chunk, atomics)

"""Bit comparison of basd_jacobi_svd on the block kernels (quad- and hex-block ordering) between two builds of the
library loaded into one process: the in-tree one and --parent <libbasd_hip.so of the commit to compare with>.  The
block kernels carry no floating-point atomics and a data-independent schedule, so a refactor of csrc/jacobi.hip has
to reproduce the rotated columns, the singular values, the sweep counts and the status word bit for bit on every
instantiation.  One line per case; exit status 1 if any bit differs.

    python scripts/jacobi_bits.py --parent /path/to/parent/libbasd_hip.so > profiles/<name>.txt"""
import argparse, ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="the other build of libbasd_hip.so")
args = ap.parse_args()

new, old = nat.lib(), ctypes.CDLL(args.parent)
old.basd_jacobi_svd.argtypes = list(nat._SIGNATURES["basd_jacobi_svd"])
old.basd_jacobi_svd.restype = ctypes.c_int
P = ctypes.c_void_p

# (rows m, columns n, batch): the smallest shapes that reach each instantiation and each seam
SHAPES = [("quad <1,16>, ragged n % 4", 40, 32, 5), ("quad <1,16>, phantom block", 33, 17, 3),
          ("quad <2,16>", 120, 64, 2), ("quad <3,16>", 176, 100, 2), ("quad <4,16>", 196, 196, 2),
          ("quad <4,16>", 250, 60, 2), ("quad <3,32>", 300, 64, 2),
          ("hex <1,2,16>, wide, n % 6 == 0", 64, 180, 2), ("hex <2,2,16>, n % 6 != 0", 120, 133, 2),
          ("hex <3,1,16>, phantom block", 192, 130, 3), ("hex <3,2,16>, batch > 256", 150, 150, 257),
          ("hex <3,2,32>", 300, 170, 2), ("hex <3,2,32>", 384, 192, 3)]
SEAMS = [(40, 32, 5), (176, 100, 2), (120, 133, 2), (192, 130, 3)]       # also sort = 0 and every `active` mode


def graded(m, n, batch):
    """column-major [batch, n, ld] copy of a graded Gaussian (tests/test_kernels_gpu.py, singular values and invariants)"""
    g = torch.Generator().manual_seed(m * 1000 + n)
    a = torch.randn(batch, m, n, generator=g) * torch.logspace(0, -5, n).view(1, 1, n)
    w = torch.zeros(batch, n, nat.jacobi_ld(m))
    w[:, :, :m] = a.transpose(1, 2)
    return w


def solve(lib, w0, m, *, sort=1, max_sweeps=60, active=None, active_rows=0):
    batch, n, ld = w0.shape
    w = w0.cuda()
    sigma = torch.full((batch, n), float("nan"), device="cuda")
    sweeps = torch.full((batch,), -777, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    act = None if active is None else active.int().cuda()
    rc = lib.basd_jacobi_svd(P(w.data_ptr()), batch, m, n, ld, m, ctypes.c_float((m ** 0.5) * 5.96e-8), max_sweeps, sort,
                             P(sigma.data_ptr()), P(sweeps.data_ptr()), P(0 if act is None else act.data_ptr()),
                             active_rows, P(status.data_ptr()), nat._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return w, sigma, sweeps, status


def bits(x):
    return x if x.dtype == torch.int32 else x.view(torch.int32)


bad = 0


def case(label, w0, m, skipped=(), **kw):
    """both builds on copies of w0; `skipped`: matrices a mask entry < 0 excludes -- their w and sigma must come back
    untouched (sigma keeps its NaN fill) with sweeps == 0"""
    global bad
    r0, r1 = solve(old, w0, m, **kw), solve(new, w0, m, **kw)
    eq = [bool(torch.equal(bits(x), bits(y))) for x, y in zip(r0, r1)]
    note = ""
    for i in skipped:
        for (w, sigma, sweeps, _) in (r0, r1):
            ok = bool(torch.equal(bits(w[i].cpu()), bits(w0[i]))) and bool(torch.isnan(sigma[i]).all()) and int(sweeps[i]) == 0
            eq[0] &= ok
        note = f" (matrix {list(skipped)} skipped: untouched in both)"
    live = [i for i in range(w0.shape[0]) if i not in skipped]
    clean = not bool(torch.isnan(r1[1][live]).any()) and -777 not in r1[2].tolist()
    bad += not (all(eq) and clean)
    batch, n, _ = w0.shape
    print(f"{label:58s} m {m:3d} n {n:3d} batch {batch:3d}  " +
          "  ".join(f"{k} {'equal' if v else 'DIFFERS'}" for k, v in zip(("w", "sigma", "sweeps", "status"), eq)) +
          f"  [sweeps {int(r1[2].min())}..{int(r1[2].max())}, status {int(r1[3]):#x}]{note}" +
          ("" if clean else "  FILL VALUES LEFT IN THE OUTPUT"), flush=True)


print(f"# basd_jacobi_svd, the in-tree library against --parent {os.path.basename(args.parent)}, one process, graded Gaussian input")
for (label, m, n, batch) in SHAPES:
    case(label, graded(m, n, batch), m)
for (m, n, batch) in SEAMS:
    w0 = graded(m, n, batch)
    case("sort = 0", w0, m, sort=0)
    # mode 1: leading-column counts (1 is clamped to 2), the other columns zero; mode 2: the same rows only
    counts = torch.tensor([1, n, n // 2 + 1, 7, n - 1][:batch])
    cols = torch.arange(n).view(1, n, 1) < counts.clamp_min(2).view(batch, 1, 1)
    case(f"active mode 1, counts {counts.tolist()}", w0 * cols, m, active=counts)
    rows = torch.arange(w0.shape[2]).view(1, 1, -1) < counts.clamp_min(2).view(batch, 1, 1)
    case(f"active mode 2, counts {counts.tolist()}", w0 * cols * rows, m, active=counts, active_rows=1)
    mask = torch.full((batch,), n)
    mask[batch - 1] = -1
    case("active mode 3 (mask)", w0, m, skipped=(batch - 1,), active=mask, active_rows=2)
# rank-deficient: half the columns are exact copies of the others, the debris pass fires
for (label, m, n, batch) in [("quad, rank n / 2 (debris)", 64, 32, 2), ("hex, rank n / 2 (debris)", 160, 150, 2)]:
    w0 = graded(m, n, batch)
    w0[:, n // 2:] = w0[:, :n // 2]
    case(label, w0, m)
# two sweeps only: not converged, negative sweep counts, kernel variant and matrix index in the status word
for (label, m, n, batch) in [("quad, max_sweeps = 2", 176, 100, 2), ("hex, max_sweeps = 2", 192, 130, 3)]:
    case(label, graded(m, n, batch), m, max_sweeps=2)
print("ALL EQUAL" if not bad else f"{bad} CASES DIFFER")
sys.exit(1 if bad else 0)

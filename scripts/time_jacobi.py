"""Jacobi timing on Procrustes-like factors (GPU): the hex-block kernel at 192 columns, the quad-block kernel at 64.

--parent <another build of libbasd_hip.so> loads that build into the same process and times basd_jacobi_svd of both on
the shapes above and on rectangular ones that reach the other block-kernel instantiations: brackets alternated parent,
this build, parent, ...; each bracket is --iters solves on fresh copies of the input between two device events.  The
spread of the parent's own brackets is the band inside which the two count as equal."""
import argparse, ctypes, statistics, sys, os, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="another build of libbasd_hip.so; its brackets and this build's are alternated")
ap.add_argument("--runs", type=int, default=5, help="--parent: brackets of this build (the parent gets one more)")
ap.add_argument("--iters", type=int, default=3, help="--parent: solves per bracket")
args = ap.parse_args()
parent = None
if args.parent:
    parent = ctypes.CDLL(args.parent)
    parent.basd_jacobi_svd.argtypes = list(nat._SIGNATURES["basd_jacobi_svd"])
    parent.basd_jacobi_svd.restype = ctypes.c_int


def ab(keep, m):
    """keep [batch, n, ld] column-major: ms per basd_jacobi_svd of the parent and of this build, alternated"""
    batch, n, ld = keep.shape
    P = ctypes.c_void_p
    ws = [torch.empty_like(keep) for _ in range(args.iters)]
    sigma = torch.empty(batch, n, device="cuda")
    sweeps = torch.empty(batch, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def bracket(lib):
        for w in ws:
            w.copy_(keep)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for w in ws:
            rc = lib.basd_jacobi_svd(P(w.data_ptr()), batch, m, n, ld, m, ctypes.c_float((m ** 0.5) * 5.96e-8), 60, 1,
                                     P(sigma.data_ptr()), P(sweeps.data_ptr()), P(0), 0, P(status.data_ptr()), nat._stream())
            assert rc == 0, rc
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    bracket(parent); bracket(nat.lib())                     # warm-up of both
    tp, tn = [], []
    for _ in range(args.runs):
        tp.append(bracket(parent)); tn.append(bracket(nat.lib()))
    tp.append(bracket(parent))
    med = statistics.median
    inside = min(tp) <= med(tn) <= max(tp)
    print(f"A/B {batch:5d} x ({m:3d} x {n:3d})   parent {med(tp):.4f} ms (brackets {min(tp):.4f} - {max(tp):.4f}, spread "
          f"{max(tp) - min(tp):.4f})   this build {med(tn):.4f} ms ({min(tn):.4f} - {max(tn):.4f})   "
          f"{'inside' if inside else 'faster than' if med(tn) < min(tp) else 'OUTSIDE'} the parent's band   "
          f"[mean sweeps {float(sweeps.float().abs().mean()):.2f}, status {int(status)}]", flush=True)


def timeit(f, it=7):
    """median over `it` device-event brackets (a host-side stall of the allocator / runtime once showed up as a 22 ms
    'launch' in the mean of three wall-clock iterations)"""
    f(); torch.cuda.synchronize()
    ts = []
    for _ in range(it):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]

for batch, n in [(1024, 192), (4, 192), (24, 192), (48, 192), (48, 64)]:
    g = torch.Generator().manual_seed(n)
    # cross-covariance-like: graded spectrum, condition ~1e5
    z = torch.randn(batch, 2 * n, n, dtype=torch.float64, generator=g) * torch.logspace(0, -2.5, n, dtype=torch.float64)
    z = z @ torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=g))[0]
    a = (z.transpose(1, 2) @ z).cuda()
    w0, lw, piv, rk = nat.pchol(a)
    ref = torch.linalg.eigvalsh(a[:4].cpu()).flip(-1)
    keep = w0.clone()
    def run():
        w = keep.clone()
        return nat.jacobi_svd(w, n)
    sigma, sweeps = run()
    torch.cuda.synchronize()
    err = float(((sigma[:4].cpu().double() ** 2) / ref - 1).abs().max())
    wout = keep.clone()
    nat.jacobi_svd(wout, n)
    cols = wout[:32, :, :n].double()                       # rotated columns of 32 matrices
    gram = cols @ cols.transpose(1, 2)
    dg = torch.diagonal(gram, dim1=1, dim2=2).clamp_min(1e-300).sqrt()
    cosm = (gram / (dg.unsqueeze(2) * dg.unsqueeze(1))).abs()
    cosm = cosm - torch.diag_embed(torch.diagonal(cosm, dim1=1, dim2=2))
    resid = float(cosm.max())
    t_clone = timeit(lambda: keep.clone())
    print(f"batch {batch} n {n}: jacobi {timeit(run) - t_clone:.3f} ms  sweeps min/mean/max {int(sweeps.min())}/{float(sweeps.float().mean()):.2f}/{int(sweeps.max())}  eig rel err {err:.2e}  max residual |cos| {resid:.2e}")
    if parent is not None:
        ab(keep, n)

# rectangular graded Gaussians (batch, rows m, columns n): quad-block <4, 16> (196 x 196), hex-block <3, 2, 32>, quad-block
# <3, 32>, hex-block <3, 2, 16> (batch > 256)
if parent is not None:
    for batch, m, n in [(256, 196, 196), (1024, 196, 196), (64, 384, 192), (64, 300, 64), (300, 176, 190)]:
        g = torch.Generator().manual_seed(m * 1000 + n)
        a = torch.randn(batch, m, n, generator=g) * torch.logspace(0, -2.5, n).view(1, 1, n)
        keep = torch.zeros(batch, n, nat.jacobi_ld(m), device="cuda")
        keep[:, :, :m] = a.transpose(1, 2).cuda()
        ab(keep, m)

# clustered spectrum (groups of nearly equal singular values): large-angle rotations at tiny cosines
batch, n = 512, 192
g = torch.Generator().manual_seed(7)
sv = torch.logspace(0, -2, 24, dtype=torch.float64).repeat_interleave(8) * (1 + 1e-6 * torch.randn(192, dtype=torch.float64, generator=g))
q1 = torch.linalg.qr(torch.randn(batch, n, n, dtype=torch.float64, generator=g))[0]
q2 = torch.linalg.qr(torch.randn(batch, n, n, dtype=torch.float64, generator=g))[0]
a = (q1 * sv) @ q2.transpose(1, 2)
ld = nat.jacobi_ld(n)
w = torch.zeros(batch, n, ld, dtype=torch.float32, device="cuda")
w[:, :, :n] = a.transpose(1, 2).float().cuda()
sigma, sweeps = nat.jacobi_svd(w, n)
cols = w[:32, :, :n].double()
gram = cols @ cols.transpose(1, 2)
dg = torch.diagonal(gram, dim1=1, dim2=2).clamp_min(1e-300).sqrt()
cosm = (gram / (dg.unsqueeze(2) * dg.unsqueeze(1))).abs()
cosm = cosm - torch.diag_embed(torch.diagonal(cosm, dim1=1, dim2=2))
ref = torch.linalg.svdvals(a[:8])
print(f"clustered spectrum batch {batch}: sweeps min/mean/max {int(sweeps.min())}/{float(sweeps.float().mean()):.2f}/{int(sweeps.max())} "
      f"sigma rel err {float((sigma[:8].cpu().double() / ref - 1).abs().max()):.2e}  max residual |cos| {float(cosm.max()):.2e}")

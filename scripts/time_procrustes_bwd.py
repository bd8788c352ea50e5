"""basd_procrustes_bwd (fused bf16 three-product split + residual epilogue) against the library fp32 bmm + the row
kernels.  Default: the c2 shapes (1024 x [196, 196] x [196, 768]); --n / --batch (with --d-s / --d-t) time one other
shape, e.g. the 384 px ones (--batch 256 --n 576, --n 729: the row-tiled kernel).  Each figure is the median of --runs
device-event brackets of --iters calls, the two paths alternated in one process.

--side times basd_procrustes_bwd_side alone (one side of the backward: fac [n, n] x W [n, d], fp32 output) at
--batch / --n / --d (--table: at every shape of the table in csrc/procrustes_bwd.hip) and prints the median of the
brackets; BASD_LIB=<another build of the library> times that build.  --parent <another build> loads that build into the
same process and alternates its brackets with the in-tree build's: parent, this build, parent, ...; the spread of the
parent's own brackets is the band inside which the two count as equal."""
import argparse, ctypes, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=None, help="tokens (rows of a matrix); default: the two c2 shapes")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--d-s", type=int, default=192)
ap.add_argument("--d-t", type=int, default=768)
ap.add_argument("--side", action="store_true", help="time basd_procrustes_bwd_side alone at --batch / --n / --d")
ap.add_argument("--d", type=int, default=768, help="columns of W for --side")
ap.add_argument("--parent", default=None, help="--side: another build of libbasd_hip.so, loaded into the same process; its "
                "brackets and this build's are alternated")
ap.add_argument("--table", action="store_true", help="--side: every shape of the table in csrc/procrustes_bwd.hip")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()


def bracket(f, it):
    """ms per call between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / it


# the shapes of the table in csrc/procrustes_bwd.hip, the one shape left on the staged kernel and a 576-token one
TABLE = [(1024, 196, 768), (512, 196, 1024), (1024, 196, 1280), (1024, 196, 192), (1024, 80, 768), (1024, 128, 768),
         (1024, 256, 768), (2, 100, 112), (300, 80, 16), (256, 576, 192)]


def time_side(batch, n, d, parent):
    g = torch.Generator().manual_seed(0)
    w = torch.randn(batch, n, d, generator=g).cuda()
    a = torch.rand(batch, n, generator=g).cuda() + 0.1; a = (a / a.sum(-1, keepdim=True)).contiguous()
    gl = torch.randn(batch, generator=g).cuda()
    fac = (torch.randn(batch, n, n, generator=g) / n ** 0.5).cuda()
    out, rowdot = torch.empty_like(w), torch.empty_like(a)
    p = ctypes.c_void_p

    def side(lib):
        nat._check(lib.basd_procrustes_bwd_side(p(fac.data_ptr()), p(w.data_ptr()), p(a.data_ptr()), p(gl.data_ptr()),
                                                batch, n, d, p(out.data_ptr()), nat.DTYPE_F32, p(rowdot.data_ptr()),
                                                nat._stream()), "basd_procrustes_bwd_side")

    libs = [nat.lib()] + ([parent] if parent is not None else [])
    for lib in libs:
        for _ in range(3):
            side(lib)
    torch.cuda.synchronize()
    med = statistics.median
    if parent is None:
        ts = [bracket(lambda: side(nat.lib()), args.iters) for _ in range(args.runs)]
        gb = (2 * batch * n * d + batch * n * n) * 4 / 1e9       # W read + gradient written + factor read, once each
        print(f"side batch {batch} n {n} d {d} ({nat.LIB_PATH}): median {med(ts):.4f} ms "
              f"({'/'.join(f'{x:.4f}' for x in ts)}), {gb / med(ts):.2f} TB/s of {gb:.2f} GB algorithmic", flush=True)
        return
    # parent, this build, parent, ... alternated: the parent's own brackets give the band a difference has to leave
    tp, tn = [], []
    for _ in range(args.runs):
        tp.append(bracket(lambda: side(parent), args.iters)); tn.append(bracket(lambda: side(nat.lib()), args.iters))
    tp.append(bracket(lambda: side(parent), args.iters))
    inside = min(tp) - 1e-4 <= med(tn) <= max(tp) + 1e-4
    print(f"side {batch:5d} x {n:4d} x {d:5d}   parent {med(tp):.4f} ms (brackets {min(tp):.4f} - {max(tp):.4f}, spread "
          f"{max(tp) - min(tp):.4f})   this build {med(tn):.4f} ms ({min(tn):.4f} - {max(tn):.4f})   "
          f"{'inside' if inside else 'faster than' if med(tn) < min(tp) else 'OUTSIDE'} the parent's band", flush=True)


if args.side:
    parent = None
    if args.parent:
        parent = ctypes.CDLL(args.parent)
        parent.basd_procrustes_bwd_side.argtypes = list(nat._SIGNATURES["basd_procrustes_bwd_side"])
        parent.basd_procrustes_bwd_side.restype = ctypes.c_int
    for (batch, n, d) in (TABLE if args.table else [(args.batch, args.n or 196, args.d)]):
        time_side(batch, n, d, parent)
    sys.exit(0)

shapes = [(1024, 196, 192, 768), (512, 196, 384, 1024)] if args.n is None else [(args.batch, args.n, args.d_s, args.d_t)]
for (batch, n, d_s, d_t) in shapes:
    g = torch.Generator().manual_seed(0)
    s_w = torch.randn(batch, n, d_s, generator=g).cuda(); t_w = torch.randn(batch, n, d_t, generator=g).cuda()
    a = torch.rand(batch, n, generator=g).cuda() + 0.1; a = (a / a.sum(-1, keepdim=True)).contiguous()
    gl = torch.randn(batch, generator=g).cuda()
    a_t = (torch.randn(batch, n, n, generator=g) / n ** 0.5).cuda()
    token = n <= d_s
    fac_s = ((torch.randn(batch, n, n, generator=g) / n ** 0.5) if token else torch.randn(batch, n, d_s, generator=g)).cuda()

    def fused():
        return nat.procrustes_bwd(s_w, t_w, a, gl, fac_s, a_t, torch.bfloat16)

    def unfused():
        p_t = a_t @ t_w
        p_s = fac_s @ s_w if token else fac_s
        g_s, dot_s = nat.procrustes_bwd_rows(p_s, s_w, a, gl, out_dtype=torch.bfloat16)
        g_t, dot_t = nat.procrustes_bwd_rows(p_t, t_w, a, gl, out_dtype=torch.float32)
        return g_s, g_t, (dot_s + dot_t) / (2.0 * a)

    f, u = fused(), unfused()
    torch.cuda.synchronize()
    err = float((f[1] - u[1]).norm() / u[1].norm())
    for _ in range(2):                                       # warm both paths at this shape
        fused(); unfused()
    torch.cuda.synchronize()
    tf, tu = [], []
    for _ in range(args.runs):                               # alternated
        tf.append(bracket(fused, args.iters)); tu.append(bracket(unfused, args.iters))
    fmt = lambda xs: "/".join(f"{x:.3f}" for x in xs)
    print(f"batch {batch} n {n} d_s {d_s} d_t {d_t}: fused {statistics.median(tf):.3f} ms ({fmt(tf)}), "
          f"library bmm + rows {statistics.median(tu):.3f} ms ({fmt(tu)}), g_t rel diff {err:.1e}", flush=True)

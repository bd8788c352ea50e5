"""Bit comparison of basd_procrustes_bwd_side / basd_procrustes_bwd between two builds of the library loaded into one
process: the in-tree one and --parent <libbasd_hip.so of the commit to compare with>.  `out` and `rowdot` carry no
atomics and a fixed slot order, so a refactor of csrc/procrustes_bwd.hip has to reproduce them bit for bit on every
dispatch arm.  One line per shape and output type; exit status 1 if any bit differs.

    python scripts/procrustes_bwd_bits.py --parent /path/to/parent/libbasd_hip.so > profiles/<name>.txt"""
import argparse, ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat
from tests import _pbwd_cases

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="the other build of libbasd_hip.so")
args = ap.parse_args()

NAMES = ("basd_procrustes_bwd_side", "basd_procrustes_bwd", "basd_procrustes_bwd_workspace_bytes")
new, old = nat.lib(), ctypes.CDLL(args.parent)
for name in NAMES:
    fn = getattr(old, name)
    fn.argtypes = list(nat._SIGNATURES[name])
    fn.restype = ctypes.c_int64 if name.endswith("_workspace_bytes") else ctypes.c_int
P = ctypes.c_void_p

# (arm, batch, n, d): every live dispatch arm of basd_procrustes_bwd_side
SHAPES = [("direct<2>", 2, 20, 16), ("direct<2>", 2, 32, 48), ("direct<4>", 2, 48, 112),
          ("staged<4>", 2, 64, 16), ("staged<4>", 2, 64, 112),
          ("staged<8>", 2, 100, 16), ("staged<8>", 2, 80, 96), ("staged<8>", 300, 80, 16)]
SHAPES += [("resident", b, n, d) for (b, n, d, _) in _pbwd_cases.CASES if n > 128 or (n > 64 and d >= 112)]
SHAPES += [("row-tiled, 16-byte loads", 2, 260, 112), ("row-tiled, 16-byte loads", 1, 576, 192),
           ("row-tiled, 4-byte loads", 2, 261, 48), ("row-tiled, 4-byte loads", 1, 729, 64),
           ("row-tiled, 4-byte loads", 2, 30, 16)]


def side(lib, fac, w, a, gl, dtype):
    batch, n, d = w.shape
    out = torch.full((batch, n, d), float("nan"), dtype=dtype, device="cuda")
    rowdot = torch.full((batch, n), float("nan"), device="cuda")
    code = nat.DTYPE_BF16 if dtype == torch.bfloat16 else nat.DTYPE_F32
    rc = lib.basd_procrustes_bwd_side(P(fac.data_ptr()), P(w.data_ptr()), P(a.data_ptr()), P(gl.data_ptr()), batch, n, d,
                                      P(out.data_ptr()), code, P(rowdot.data_ptr()), nat._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, rowdot


def same(x, y):
    """equal bits (NaN-safe: compared as integers), and no NaN left from the fill"""
    it = {4: torch.int32, 2: torch.int16}[x.element_size()]
    return bool(torch.equal(x.view(it), y.view(it))) and not bool(torch.isnan(x.float()).any())


bad = 0
print(f"# basd_procrustes_bwd_side, the in-tree library against --parent {os.path.basename(args.parent)}, one process, "
      f"inputs of tests/_pbwd_cases.white")
for (arm, batch, n, d) in SHAPES:
    inputs = [t.cuda() for t in _pbwd_cases.white(batch, n, d)]
    for dtype in (torch.float32, torch.bfloat16):
        (o0, r0), (o1, r1) = side(old, *inputs, dtype), side(new, *inputs, dtype)
        ok_o, ok_r = same(o0, o1), same(r0, r1)
        bad += not (ok_o and ok_r)
        print(f"side {arm:26s} batch {batch:4d} n {n:4d} d {d:4d} {str(dtype)[6:]:9s} out {'equal' if ok_o else 'DIFFERS'} "
              f"rowdot {'equal' if ok_r else 'DIFFERS'}", flush=True)

# one full backward (both sides on the token path + g_a)
batch, n, d_s, d_t = 2, 196, 192, 768
g = torch.Generator().manual_seed(196)
s_w, t_w = torch.randn(batch, n, d_s, generator=g).cuda(), torch.randn(batch, n, d_t, generator=g).cuda()
a = torch.rand(batch, n, generator=g) + 0.1
a = (a / a.sum(-1, keepdim=True)).contiguous().cuda()
gl = torch.randn(batch, generator=g).cuda()
a_t, fac_s = [(torch.randn(batch, n, n, generator=g) / n ** 0.5).cuda() for _ in range(2)]
res = []
for lib in (old, new):
    g_s = torch.full((batch, n, d_s), float("nan"), dtype=torch.bfloat16, device="cuda")
    g_t = torch.full((batch, n, d_t), float("nan"), device="cuda")
    g_a = torch.full((batch, n), float("nan"), device="cuda")
    nb = lib.basd_procrustes_bwd_workspace_bytes(batch, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = lib.basd_procrustes_bwd(P(s_w.data_ptr()), P(t_w.data_ptr()), P(a.data_ptr()), P(gl.data_ptr()), P(fac_s.data_ptr()),
                                 P(a_t.data_ptr()), batch, n, d_s, d_t, P(g_s.data_ptr()), nat.DTYPE_BF16, P(g_t.data_ptr()),
                                 P(g_a.data_ptr()), P(ws.data_ptr()), nb, nat._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    res.append((g_s, g_t, g_a))
oks = [same(x, y) for x, y in zip(*res)]
bad += not all(oks)
print(f"basd_procrustes_bwd batch {batch} n {n} d_s {d_s} d_t {d_t}: " +
      " ".join(f"{k} {'equal' if v else 'DIFFERS'}" for k, v in zip(("g_s", "g_t", "g_a"), oks)))
print("ALL EQUAL" if not bad else f"{bad} COMPARISONS DIFFER")
sys.exit(1 if bad else 0)

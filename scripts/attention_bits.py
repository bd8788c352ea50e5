"""Bit comparison of the seven forward attention entries (csrc/attention.hip, csrc/attention_long.hip) between two builds
of the library loaded into one process: the in-tree one and --parent <libbasd_hip.so of the commit to compare with>.
The kernels carry no atomics and a fixed summation order, so a refactor of the two files has to reproduce every output
-- out, importance and, where the entry has one, the LSE -- bit for bit.  B = 2, H = 3, logits of trained-network
spread (tests/_attn_regimes.py: a CLS sink of strength 30, and logits of std 14).  One line per entry, shape and
output combination; exit status 1 if any bit differs.

    python scripts/attention_bits.py --parent /path/to/parent/libbasd_hip.so > profiles/<name>.txt"""
import argparse, ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat
from tests import _attn_regimes as R

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="the other build of libbasd_hip.so")
args = ap.parse_args()

NAMES = ("basd_attention_fwd_bf16", "basd_attention_fwd_qmean_bf16", "basd_attention_fwd_relbias_bf16",
         "basd_attention_fwd_rope_bf16", "basd_attention_fwd_long_bf16", "basd_attention_fwd_long_relbias_bf16",
         "basd_attention_fwd_long_rope_bf16")
new, old = nat.lib(), ctypes.CDLL(args.parent)
for name in NAMES:
    fn = getattr(old, name)
    fn.argtypes = list(nat._SIGNATURES[name])
    fn.restype = ctypes.c_int
B, H = 2, 3
REGIMES = ("cls_sink30", "hot")
F = ctypes.c_float


def P(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def same(x, y):
    """equal bits (compared as integers), and no NaN left from the fill"""
    it = {4: torch.int32, 2: torch.int16}[x.element_size()]
    return bool(torch.equal(x.view(it), y.view(it))) and not bool(torch.isnan(x.float()).any())


def qkv_of(T, hd, regime):
    return R.sink_qkv(B, T, H, hd, regime=regime, seed=R.seed_of(B, T, H, hd, regime)).cuda()


def table_of(gh, gw):
    g = torch.Generator().manual_seed(1000 * gh + gw)
    return (2.0 * torch.randn((2 * gh - 1) * (2 * gw - 1) + 3, H, generator=g)).cuda()


bad = 0


def compare(label, call, outputs):
    """call(lib, *buffers) on both builds with NaN-filled buffers of the given (shape, dtype) | None"""
    global bad
    res = []
    for lib in (old, new):
        bufs = [None if o is None else nan(*o[0], dtype=o[1]) for o in outputs]
        rc = call(lib, *bufs)
        assert rc == 0, (label, rc)
        torch.cuda.synchronize()
        res.append(bufs)
    ok = all(same(x, y) for x, y in zip(*res) if x is not None)
    bad += not ok
    print(f"{label}: {'identical' if ok else 'DIFFERS'}", flush=True)


print(f"# forward attention entries, the in-tree library against --parent {os.path.basename(args.parent)}, one process; "
      f"B {B}, H {H}, inputs of tests/_attn_regimes.sink_qkv; outputs compared as integers")
for regime in REGIMES:
    bf, f32 = torch.bfloat16, torch.float32
    for hd in (64, 80):
        scale = hd ** -0.5
        for T in (1, 2, 64, 65, 208, 209, 272):
            qkv = qkv_of(T, hd, regime)
            out = ((B, T, H * hd), bf)
            for tap in (False, True):
                for lse in (False, True):
                    if tap and T < 2:
                        continue
                    compare(f"short plain  {regime:10s} T {T:4d} hd {hd} tap {int(tap)} lse {int(lse)}",
                            lambda L, o, i, l: L.basd_attention_fwd_bf16(P(qkv), B, T, H, hd, F(scale), P(o), P(i), P(l),
                                                                         nat._stream()),
                            [out, ((B, H, T - 1), f32) if tap else None, ((B, H, T), f32) if lse else None])
            compare(f"short qmean  {regime:10s} T {T:4d} hd {hd}",
                    lambda L, o, i: L.basd_attention_fwd_qmean_bf16(P(qkv), B, T, H, hd, F(scale), P(o), P(i),
                                                                    nat._stream()), [out, ((B, H, T), f32)])
        for T in (1, 2, 63, 64, 65, 129, 273, 577, 1024):
            qkv = qkv_of(T, hd, regime)
            out = ((B, T, H * hd), bf)
            # (cls, qmean, lse): each output alone and together (the query mean needs out and the LSE)
            for cls, qm, lse in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)):
                if cls and T < 2:
                    continue
                compare(f"long plain   {regime:10s} T {T:4d} hd {hd} cls {cls} qmean {qm} lse {lse}",
                        lambda L, o, c, q, l: L.basd_attention_fwd_long_bf16(P(qkv), B, T, H, hd, F(scale), P(o), P(c), P(q),
                                                                             P(l), nat._stream()),
                        [out, ((B, H, T - 1), f32) if cls else None, ((B, H, T), f32) if qm else None,
                         ((B, H, T), f32) if lse else None])
            if T >= 2:
                compare(f"long plain   {regime:10s} T {T:4d} hd {hd} cls tap alone",
                        lambda L, c: L.basd_attention_fwd_long_bf16(P(qkv), B, T, H, hd, F(scale), P(None), P(c), P(None),
                                                                    P(None), nat._stream()), [((B, H, T - 1), f32)])
    hd, scale = 64, 0.125
    for short, grids in ((True, [(1, 1), (3, 5), (7, 9), (8, 8), (9, 23), (16, 13), (1, 271)]),
                         (False, [(1, 1), (8, 8), (16, 17), (24, 24), (31, 33)])):
        for gh, gw in grids:
            T = gh * gw + 1
            qkv, table = qkv_of(T, hd, regime), table_of(gh, gw)
            name = "basd_attention_fwd_relbias_bf16" if short else "basd_attention_fwd_long_relbias_bf16"
            for tap in (False, True):
                compare(f"{'short' if short else 'long '} relbias {regime:10s} grid {gh:2d} x {gw:3d} tap {int(tap)}",
                        lambda L, o, i: getattr(L, name)(P(qkv), P(table), B, gh, gw, H, hd, F(scale), P(o), P(i),
                                                         nat._stream()),
                        [((B, T, H * hd), bf), ((B, H, T - 1), f32) if tap else None])
    for short, Ts in ((True, (2, 17, 64, 65, 208, 209, 272)), (False, (2, 65, 273, 581, 1024))):
        for T in Ts:
            qkv, rope = qkv_of(T, hd, regime), nat.rope_table(1, T - 1, hd).cuda()
            name = "basd_attention_fwd_rope_bf16" if short else "basd_attention_fwd_long_rope_bf16"
            for tap in (False, True):
                compare(f"{'short' if short else 'long '} rope    {regime:10s} T {T:4d} tap {int(tap)}",
                        lambda L, o, i: getattr(L, name)(P(qkv), P(rope), B, T, H, hd, F(scale), P(o), P(i), nat._stream()),
                        [((B, T, H * hd), bf), ((B, H, T - 1), f32) if tap else None])
print("ALL IDENTICAL" if not bad else f"{bad} COMPARISONS DIFFER")
sys.exit(1 if bad else 0)

"""Teacher attention forward: fused kernel (+tap) vs library SDPA + separate tap (GPU).

--parent <another build of libbasd_hip.so> loads that build into the same process and times the short forward entries
(csrc/attention.hip) of both at B = 256: brackets of --iters calls between device events, alternated parent, this
build, parent, ...; the spread of the parent's own brackets is the band inside which the two count as equal
(`ab_row`, shared with scripts/time_attention_long.py)."""
import argparse, ctypes, statistics, sys, os, time, torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat


def timeit(f, it=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(it):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / it * 1e6


def load_parent(path, names):
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.argtypes = list(nat._SIGNATURES[name])
        fn.restype = ctypes.c_int
    return lib


def bracket(f, it):
    """ms per call between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / it


def ab_row(label, call, parent, iters, runs):
    """call(lib) -> status; one table line: parent's brackets, this build's, and where this build's median lies"""
    for lib in (parent, nat.lib()):
        for _ in range(3):
            assert call(lib) == 0, label
    torch.cuda.synchronize()
    tp, tn = [], []
    for _ in range(runs):
        tp.append(bracket(lambda: call(parent), iters)); tn.append(bracket(lambda: call(nat.lib()), iters))
    tp.append(bracket(lambda: call(parent), iters))
    med = statistics.median
    inside = min(tp) <= med(tn) <= max(tp)
    print(f"{label:44s} parent {med(tp):.4f} ms (brackets {min(tp):.4f} - {max(tp):.4f})   this build {med(tn):.4f} ms "
          f"({min(tn):.4f} - {max(tn):.4f})   {'inside' if inside else 'below' if med(tn) < min(tp) else 'ABOVE'} "
          f"the parent's band", flush=True)


def P(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def ab_short(parent, iters, runs):
    B, hd, scale = 256, 64, ctypes.c_float(0.125)
    st = nat._stream()
    for T, H in ((197, 3), (197, 12)):
        qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()
        out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
        imp, lse = torch.empty(B, H, T - 1, device="cuda"), torch.empty(B, H, T, device="cuda")
        ab_row(f"short plain T {T} H {H:2d} with LSE", lambda L: L.basd_attention_fwd_bf16(
            P(qkv), B, T, H, hd, scale, P(out), P(None), P(lse), st), parent, iters, runs)
        ab_row(f"short plain T {T} H {H:2d} with tap", lambda L: L.basd_attention_fwd_bf16(
            P(qkv), B, T, H, hd, scale, P(out), P(imp), P(None), st), parent, iters, runs)
    H = 12
    for T, (gh, gw) in ((197, (14, 14)), (257, (16, 16))):
        qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()
        out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
        imp = torch.empty(B, H, T - 1, device="cuda")
        table = torch.randn((2 * gh - 1) * (2 * gw - 1) + 3, H, device="cuda")
        rope = nat.rope_table(gh, gw, hd).cuda()
        ab_row(f"short relbias T {T} H {H} with tap", lambda L: L.basd_attention_fwd_relbias_bf16(
            P(qkv), P(table), B, gh, gw, H, hd, scale, P(out), P(imp), st), parent, iters, runs)
        ab_row(f"short rope T {T} H {H} with tap", lambda L: L.basd_attention_fwd_rope_bf16(
            P(qkv), P(rope), B, T, H, hd, scale, P(out), P(imp), st), parent, iters, runs)


def vs_library():
    for B, T, H in [(256, 197, 12), (256, 197, 3), (256, 257, 16)]:
        hd = 64
        qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()
        scale = hd ** -0.5
        def lib():
            q, k, v = qkv.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)
            o = F.scaled_dot_product_attention(q, k, v)
            return o.transpose(1, 2).reshape(B, T, H * hd)
        with torch.no_grad():
            t_lib = timeit(lib)
            t_tap = timeit(lambda: nat.cls_importance(qkv, H, hd, scale)) if T <= 256 else float("nan")
            t_fused = timeit(lambda: nat.attention_fwd(qkv, H, hd, scale, True))
            t_fused_notap = timeit(lambda: nat.attention_fwd(qkv, H, hd, scale, False))
            err = float((lib().float() - nat.attention_fwd(qkv, H, hd, scale, False)[0].float()).abs().max())
        mb = B * T * H * hd * 2 * 4 / 1e6
        print(f"B {B} T {T} H {H}: library sdpa {t_lib:.1f} us + tap {t_tap:.1f} us | fused {t_fused:.1f} us (no tap {t_fused_notap:.1f})"
              f"  {mb / t_fused:.2f} MB/us  max |diff| vs library {err:.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="another build of libbasd_hip.so, loaded into the same process")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if args.parent:
        ab_short(load_parent(args.parent, ("basd_attention_fwd_bf16", "basd_attention_fwd_relbias_bf16",
                                           "basd_attention_fwd_rope_bf16")), args.iters, args.runs)
    else:
        vs_library()

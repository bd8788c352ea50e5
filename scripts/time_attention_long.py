"""Long-sequence attention (csrc/attention_long.hip) against the library SDPA path these shapes took before (GPU).

Forward: basd_attention_fwd_long_bf16 with the LSE (the student's forward) vs aten._scaled_dot_product_flash_attention
on the packed projection (models/vit.py:_PackedFlashAttention).  Backward: basd_attention_bwd_long_bf16 (delta, main,
dQ reduce) vs aten._scaled_dot_product_flash_attention_backward plus the stack into the packed gradient.
Medians of device-event brackets over --iters calls; TF/s counts 4 B H T^2 hd (forward) and 10 B H T^2 hd (backward)."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat  # noqa: E402

SHAPES = [  # (label, B, T, H, hd)
    ("DeiT-T/14 224px", 256, 257, 3, 64),
    ("DeiT-T/16 384px", 64, 577, 3, 64),
    ("ViT-B/16 384px", 64, 577, 12, 64),
    ("hd-80 student", 256, 197, 2, 80),
]


def median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def ab_long(parent, iters, runs):
    """the long forward entries at B = 256, this build against --parent (time_attention.ab_row)"""
    from time_attention import P, ab_row
    B, H, st = 256, 12, nat._stream()
    for T, hd in ((257, 64), (577, 64), (257, 80)):
        qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()
        out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
        imp, lse = torch.empty(B, H, T - 1, device="cuda"), torch.empty(B, H, T, device="cuda")
        ab_row(f"long plain T {T} H {H} hd {hd} with LSE + CLS tap", lambda L: L.basd_attention_fwd_long_bf16(
            P(qkv), B, T, H, hd, ctypes.c_float(hd ** -0.5), P(out), P(imp), P(None), P(lse), st), parent, iters, runs)
    hd, scale = 64, ctypes.c_float(0.125)
    gh = gw = 24
    T = gh * gw + 1
    qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()
    out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
    imp = torch.empty(B, H, T - 1, device="cuda")
    table = torch.randn((2 * gh - 1) * (2 * gw - 1) + 3, H, device="cuda")
    ab_row(f"long relbias T {T} H {H} with tap", lambda L: L.basd_attention_fwd_long_relbias_bf16(
        P(qkv), P(table), B, gh, gw, H, hd, scale, P(out), P(imp), st), parent, iters, runs)
    T = 581                                          # DINOv3 at 384 px: 24 x 24 patches + CLS + 4 registers
    qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()
    out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
    imp = torch.empty(B, H, T - 1, device="cuda")
    rope = nat.dinov3_rope_table(24, 24, hd).cuda()
    ab_row(f"long rope T {T} H {H} with tap", lambda L: L.basd_attention_fwd_long_rope_bf16(
        P(qkv), P(rope), B, T, H, hd, scale, P(out), P(imp), st), parent, iters, runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="another build of libbasd_hip.so, loaded into the same process: its "
                    "brackets of the long forward entries and this build's are alternated")
    args = ap.parse_args()
    if args.parent:
        from time_attention import load_parent
        return ab_long(load_parent(args.parent, ("basd_attention_fwd_long_bf16", "basd_attention_fwd_long_relbias_bf16",
                                                 "basd_attention_fwd_long_rope_bf16")), args.iters, args.runs)
    L = nat.lib()
    print(f"{'shape':<18} {'B':>4} {'T':>5} {'H':>3} {'hd':>3} | {'fwd ms':>8} {'TF/s':>6} {'sdpa ms':>8} {'TF/s':>6} | "
          f"{'bwd ms':>8} {'TF/s':>6} {'sdpa ms':>8} {'TF/s':>6}")
    for label, B, T, H, hd in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(T)
        qkv = (torch.randn(B, T, 3 * H * hd, device="cuda", generator=g) * 0.8).bfloat16()
        dout = torch.randn(B, T, H * hd, device="cuda", generator=g).bfloat16()
        scale = hd ** -0.5
        out = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
        lse = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
        dqkv = torch.empty_like(qkv)
        ws = torch.empty(int(L.basd_attention_bwd_long_workspace_bytes(B, T, H, hd)), dtype=torch.uint8, device="cuda")
        st = nat._stream()

        def fwd():
            nat._check(L.basd_attention_fwd_long_bf16(nat._ptr(qkv), B, T, H, hd, ctypes.c_float(scale), nat._ptr(out),
                                                      None, None, nat._ptr(lse), st), "fwd_long")

        def bwd():
            nat._check(L.basd_attention_bwd_long_bf16(nat._ptr(qkv), nat._ptr(out), nat._ptr(dout), nat._ptr(lse), B, T,
                                                      H, hd, ctypes.c_float(scale), nat._ptr(dqkv), nat._ptr(ws),
                                                      ctypes.c_int64(ws.numel()), st), "bwd_long")

        x = qkv.view(B, T, 3, H, hd)
        q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
        res = torch.ops.aten._scaled_dot_product_flash_attention(q, k, v, 0.0, False, False)
        o_l, lse_l, cq, ck, mq, mk, seed, off = res[:8]
        g_l = dout.view(B, T, H, hd).transpose(1, 2)

        def fwd_lib():
            torch.ops.aten._scaled_dot_product_flash_attention(q, k, v, 0.0, False, False)

        def bwd_lib():
            dq, dk, dv = torch.ops.aten._scaled_dot_product_flash_attention_backward(
                g_l, q, k, v, o_l, lse_l, cq, ck, mq, mk, 0.0, False, seed, off)
            torch.stack((dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)), dim=2)

        with torch.no_grad():
            tf, tb = median_ms(fwd, args.iters), median_ms(bwd, args.iters)
            tfl, tbl = median_ms(fwd_lib, args.iters), median_ms(bwd_lib, args.iters)
        ff, fb = 4.0 * B * H * T * T * hd, 10.0 * B * H * T * T * hd
        rate = lambda f, ms: f / ms / 1e9
        print(f"{label:<18} {B:>4} {T:>5} {H:>3} {hd:>3} | {tf:8.3f} {rate(ff, tf):6.1f} {tfl:8.3f} {rate(ff, tfl):6.1f} | "
              f"{tb:8.3f} {rate(fb, tb):6.1f} {tbl:8.3f} {rate(fb, tbl):6.1f}")


if __name__ == "__main__":
    main()

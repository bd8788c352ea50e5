"""The frozen vit_base_patch16_dinov3 teacher at 224 px, bf16: forward with the per-block taps (what the trainer runs,
``extract_intermediates``) on the own path -- q and k rotated inside the attention kernel
(basd_attention_fwd_rope_bf16 at 201 tokens), CLS / register / patch rows assembled by basd_vit_embed_reg_bf16 --
against the SAME model on the library path (models/eva.py, _FUSED_EVA_DISPATCH off: torch rotation + SDPA + a separate
tap, torch token assembly).

Every round is a FRESH child process with its own time limit; inside a child the two sides alternate in one process
(the order flips with the round) and the child prints one JSON line (the raw lines of profiles/dinov3_teacher_ab.txt).
``--kernel`` adds one more child: the attention call alone at the ViT-B shape of a 384 px input (64 x 12 heads x 581
tokens) -- the new tiled entry (basd_attention_fwd_long_rope_bf16), the existing tiled kernel on the same qkv unrotated
(what the in-kernel rotation costs) and torch rotation + the existing tiled kernel (the fallback it replaces).

Device events, warm-up, medians of N timed calls.

    python scripts/time_dinov3_teacher.py [--batch 256] [--iters 10] [--rounds 3] [--kernel] [--limit 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = "vit_base_patch16_dinov3"


def median_ms(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def child_forward(args):
    import torch
    import basd_amd.losses._ops as O
    import basd_amd.models.eva as E
    from basd_amd.models import extract_intermediates, load_teacher
    teacher = load_teacher(MODEL, 224, device="cuda")
    x = torch.randn(args.batch, 3, 224, 224, device="cuda").to(torch.bfloat16)

    def run(fused):
        E._FUSED_EVA_DISPATCH = fused
        try:
            return extract_intermediates(teacher, x)
        finally:
            E._FUSED_EVA_DISPATCH = True

    sides = {"own": lambda: run(True), "library": lambda: run(False)}
    (ta, ia), (tb, ib) = sides["own"](), sides["library"]()
    last = max(ta)
    rel = float((ta[last].float() - tb[last].float()).norm() / tb[last].float().norm())
    tap = float((ia[last] - ib[last]).abs().max() / ib[last].abs().max())
    del ta, ia, tb, ib
    out = {"model": MODEL, "batch": args.batch, "iters": args.iters, "round": args.round,
           "own_vs_library_rel_l2_last_layer": rel, "own_vs_library_tap_max_rel": tap}
    for name in (("own", "library") if args.round % 2 == 0 else ("library", "own")):
        out[f"{name}_ms"] = median_ms(sides[name], args.iters)
    out["library_over_own"] = out["library_ms"]["median"] / out["own_ms"]["median"]
    out["library_fallbacks_counted"] = dict(O.FALLBACKS)
    print(json.dumps(out), flush=True)


def child_kernel(args):
    import torch
    import basd_amd._native as native
    from basd_amd.models.eva import apply_rope
    b, heads, hd, gh, gw = args.kernel_batch, 12, 64, 24, 24
    t, scale = gh * gw + 5, 64 ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(b, t, 3 * heads * hd, device="cuda", generator=g).bfloat16()
    rope = native.dinov3_rope_table(gh, gw, hd).cuda()

    def torch_rotation_then_kernel():
        x = qkv.view(b, t, 3, heads, hd)
        rot = torch.empty_like(x)
        rot[:, :, :2] = apply_rope(x[:, :, :2].transpose(1, 3), rope).transpose(1, 3)      # [B, H, 2, T, hd] views
        rot[:, :, 2] = x[:, :, 2]
        return native.attention_fwd(rot.view(b, t, -1), heads, hd, scale, want_importance=True)

    cases = [("long_rope_kernel", lambda: native.attention_fwd_long_rope(qkv, rope, heads, hd, scale, True)),
             ("plain_long_kernel", lambda: native.attention_fwd(qkv, heads, hd, scale, want_importance=True)),
             ("torch_rotation_plus_plain_long_kernel", torch_rotation_then_kernel)]
    out = {"what": "attention call alone", "B": b, "H": heads, "T": t, "hd": hd, "iters": args.iters}
    for name, fn in cases + cases[::-1]:
        ms = median_ms(fn, args.iters)
        key = f"{name}_us"
        out[key] = min(out.get(key, 1e30), round(1e3 * ms["median"], 1))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kernel-batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", choices=("forward", "kernel"))
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("time_dinov3_teacher.py needs the GPU: a CPU run says nothing about it")
        (child_forward if args.child == "forward" else child_kernel)(args)
        return
    # the parent never touches the GPU: every measurement is a fresh child under its own time limit, and the first
    # child that fails, faults or runs out of time ends the run
    base = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--kernel-batch",
            str(args.kernel_batch), "--iters", str(args.iters)]
    jobs = [base + ["--child", "forward", "--round", str(r)] for r in range(max(args.rounds, 3))]
    if args.kernel:
        jobs.append(base + ["--child", "kernel"])
    for cmd in jobs:
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"child ran past {args.limit} s: {' '.join(cmd[2:])}")
        if rc != 0:
            raise SystemExit(f"child exited with status {rc}: {' '.join(cmd[2:])}")


if __name__ == "__main__":
    main()

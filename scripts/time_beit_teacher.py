"""The frozen beitv2_base_patch16_224 teacher at 224 px, bf16: forward with the per-block taps (what the trainer runs,
``extract_intermediates``) on the own attention kernel with the relative-position bias gathered in-kernel
(basd_attention_fwd_relbias_bf16) against the SAME model on the library path (models/beit.py,
_FUSED_RELBIAS_ATTENTION off: dense [H, T, T] bias from the index buffer + SDPA with that mask + a separate tap).

Every round is a FRESH child process with its own time limit; inside a child the two sides alternate in one process
(the order flips with the round) and the child prints one JSON line (the raw lines of profiles/beit_teacher_ab.txt).
``--kernel`` adds one more child: the attention call alone at ViT-B shape (B x 12 heads x 197 tokens) -- the new kernel,
the existing unbiased kernel on the same qkv (what the in-kernel gather costs) and the library form.

``--img-size 384`` times the beit_base_patch16_384 teacher instead (a 24 x 24 grid, 577 tokens: the tiled kernels,
basd_attention_fwd_long_relbias_bf16) at the same batch, and ``--kernel`` then runs the attention call alone at
B x 12 heads x 577 tokens.

Device events, warm-up, medians of N timed calls.

    python scripts/time_beit_teacher.py [--img-size 224] [--batch 256] [--iters 10] [--rounds 3] [--kernel] [--limit 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {224: "beitv2_base_patch16_224", 384: "beit_base_patch16_384"}


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
    import basd_amd.models.beit as B
    from basd_amd.models import extract_intermediates, load_teacher
    model = MODELS[args.img_size]
    teacher = load_teacher(model, args.img_size, device="cuda")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():      # a fresh BEiT has zero-mean 0.02 tables: give the bias the spread of a trained one
        for blk in teacher.model.blocks:
            t = blk.attn.relative_position_bias_table
            t.copy_(1.5 * torch.randn(t.shape, generator=g))
    x = torch.randn(args.batch, 3, args.img_size, args.img_size, device="cuda").to(torch.bfloat16)

    def run(fused):
        B._FUSED_RELBIAS_ATTENTION = fused
        try:
            return extract_intermediates(teacher, x)
        finally:
            B._FUSED_RELBIAS_ATTENTION = True

    sides = {"own": lambda: run(True), "library": lambda: run(False)}
    (ta, ia), (tb, ib) = sides["own"](), sides["library"]()
    last = max(ta)
    rel = float((ta[last].float() - tb[last].float()).norm() / tb[last].float().norm())
    tap = float((ia[last] - ib[last]).abs().max() / ib[last].abs().max())
    del ta, ia, tb, ib
    out = {"model": model, "img_size": args.img_size, "batch": args.batch, "iters": args.iters, "round": args.round,
           "own_vs_library_rel_l2_last_layer": rel, "own_vs_library_tap_max_rel": tap}
    for name in (("own", "library") if args.round % 2 == 0 else ("library", "own")):
        out[f"{name}_ms"] = median_ms(sides[name], args.iters)
    out["library_over_own"] = out["library_ms"]["median"] / out["own_ms"]["median"]
    out["library_fallbacks_counted"] = dict(O.FALLBACKS)
    print(json.dumps(out), flush=True)


def child_kernel(args):
    import torch
    import torch.nn.functional as F
    import basd_amd._native as native
    from basd_amd.models.beit import relative_position_index
    b, heads, hd, gh, gw = args.batch, 12, 64, args.img_size // 16, args.img_size // 16
    t, scale = gh * gw + 1, 64 ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(b, t, 3 * heads * hd, device="cuda", generator=g).bfloat16()
    table = 1.5 * torch.randn((2 * gh - 1) * (2 * gw - 1) + 3, heads, device="cuda", generator=g)
    index = relative_position_index(gh, gw).cuda()

    def library():
        q, k, v = qkv.view(b, t, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
        bias = table[index.reshape(-1)].reshape(t, t, heads).permute(2, 0, 1)
        logits = (q[:, :, :1] @ k.transpose(-2, -1)).float() * scale + bias[:, :1]
        tap = logits.softmax(dim=-1)[:, :, 0, 1:].mean(dim=1)
        return F.scaled_dot_product_attention(q, k, v, attn_mask=bias.unsqueeze(0).to(q.dtype)), tap

    # the entry RelPosAttention.forward takes at this grid; attention_fwd dispatches the unbiased call the same way
    relbias = (native.attention_fwd_relbias if native.attention_fwd_relbias_supported(gh, gw, hd)
               else native.attention_fwd_long_relbias)
    cases = [("relbias_kernel", lambda: relbias(qkv, table, gh, gw, heads, hd, scale, True)),
             ("unbiased_kernel", lambda: native.attention_fwd(qkv, heads, hd, scale, want_importance=True)),
             ("library_mask_sdpa_tap", library)]
    out = {"what": "attention call alone", "B": b, "H": heads, "T": t, "hd": hd, "iters": args.iters}
    for name, fn in cases + cases[::-1]:
        ms = median_ms(fn, args.iters)
        key = f"{name}_us"
        out[key] = min(out.get(key, 1e30), round(1e3 * ms["median"], 1))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img-size", type=int, default=224, choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, default=256)
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
            raise SystemExit("time_beit_teacher.py needs the GPU: a CPU run says nothing about it")
        (child_forward if args.child == "forward" else child_kernel)(args)
        return
    # the parent never touches the GPU: every measurement is a fresh child under its own time limit, and the first
    # child that fails, faults or runs out of time ends the run
    base = [sys.executable, os.path.abspath(__file__), "--img-size", str(args.img_size), "--batch", str(args.batch),
            "--iters", str(args.iters)]
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

"""The frozen dinov2_vitg14_reg teacher (ViT-g/14, 4 register tokens, SwiGLU MLP) at 224 px, bf16, in one process.

Default: ``extract_intermediates`` (the forward with every block's token and importance taps) with the fused dispatch --
the SiLU gate in the w12 GEMM's epilogue (basd_gemm_bf16_swiglu), token assembly with registers in one kernel
(basd_vit_embed_reg_bf16) -- against the SAME model with that dispatch switched off (models/vit.py,
_FUSED_DINOV2_DISPATCH: bias-only w12 GEMM + the gate as torch ops, torch cat + add + cat).  The two sides alternate for
``--rounds`` rounds of ``--iters`` device-event brackets each; every round prints one JSON line with the medians (the raw
lines of profiles/dinov2_teacher_ab.txt).  The spread between the rounds of one side is the yardstick for the other.

``--kernel``: also the two launches alone at M = batch * 257, K = 1536, H = 4096: the gated GEMM against the bias-only
GEMM over [M, 2 H] followed by the torch gate, and the register assembly against torch's cat + add + cat.

    python scripts/time_dinov2_teacher.py [--kernel] [--batch 256] [--iters 20] [--rounds 3] [--model dinov2_vitg14_reg]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, iters, warmup=3):
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


def forward(args):
    import basd_amd.models.vit as V
    from basd_amd.models.teacher import extract_intermediates, load_teacher
    teacher = load_teacher(args.model, 224, device="cuda")
    x = torch.randn(args.batch, 3, 224, 224, device="cuda").to(torch.bfloat16)

    def run(fused_dispatch):
        V._FUSED_DINOV2_DISPATCH = fused_dispatch
        try:
            toks, imps = extract_intermediates(teacher, x)
            return toks[max(toks)], imps[max(imps)]
        finally:
            V._FUSED_DINOV2_DISPATCH = True

    sides = {"fused": lambda: run(True), "unfused": lambda: run(False)}
    a, b = sides["fused"]()[0].float(), sides["unfused"]()[0].float()
    rel = float((a - b).norm() / b.norm())
    shape = list(a.shape)
    del a, b
    for r in range(max(args.rounds, 3)):
        out = {"model": args.model, "batch": args.batch, "iters": args.iters, "round": r, "last_tokens": shape,
               "fused_vs_unfused_rel_l2": rel}
        for name in (("fused", "unfused") if r % 2 == 0 else ("unfused", "fused")):
            out[f"{name}_ms"] = median_ms(sides[name], args.iters)
        out["unfused_over_fused"] = out["unfused_ms"]["median"] / out["fused_ms"]["median"]
        print(json.dumps(out), flush=True)


def kernels(args):
    import torch.nn.functional as F
    import basd_amd._native as nat
    M, K, H, D, N, R = args.batch * 257, 1536, 4096, 1536, 256, 4
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w12 = (torch.randn(2 * H, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    b12 = torch.randn(2 * H, device="cuda", generator=g).bfloat16()
    wp, bp = nat.swiglu_pack(w12, b12)
    patches = torch.randn(args.batch, N, D, device="cuda", generator=g).bfloat16()
    cls = torch.randn(1, 1, D, device="cuda", generator=g).bfloat16()
    reg = torch.randn(1, R, D, device="cuda", generator=g).bfloat16()
    pos = torch.randn(1, 1 + N, D, device="cuda", generator=g).bfloat16()

    def unfused_gate():
        x1, x2 = nat.gemm_bf16(x, w12, b12).chunk(2, dim=-1)
        return F.silu(x1) * x2

    def torch_assembly():
        t = torch.cat([cls.expand(args.batch, -1, -1), patches], dim=1) + pos
        return torch.cat([t[:, :1], reg.expand(args.batch, -1, -1), t[:, 1:]], dim=1)

    cases = [("swiglu_gemm", lambda: nat.gemm_bf16_swiglu(x, wp, bp)), ("bias_gemm_plus_torch_gate", unfused_gate),
             ("bias_gemm_alone", lambda: nat.gemm_bf16(x, w12, b12)),
             ("embed_reg_kernel", lambda: nat.vit_embed(patches, cls, pos, reg=reg)), ("embed_reg_torch", torch_assembly)]
    assert torch.equal(cases[3][1](), cases[4][1]())
    for r in range(max(args.rounds, 3)):
        out = {"M": M, "K": K, "H": H, "iters": args.iters, "round": r}
        for name, fn in (cases if r % 2 == 0 else cases[::-1]):
            out[f"{name}_us"] = {k: round(1e3 * v, 2) for k, v in median_ms(fn, args.iters).items()}
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--model", default="dinov2_vitg14_reg")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dinov2_teacher.py needs the GPU: a CPU run says nothing about it")
    if args.kernel or args.kernel_only:
        kernels(args)
    if not args.kernel_only:
        forward(args)


if __name__ == "__main__":
    main()

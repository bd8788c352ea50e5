"""forward_features of a frozen Swin teacher (default swin_tiny_patch4_window7_224 at 224 px), bf16: the fused trunk
(csrc/swin.hip, csrc/swin_wide.hip for the window-12 presets + basd_gemm_bf16 + the LayerNorm kernels) against the
plain-torch path of the same module (library GEMMs, torch softmax and index gathers), in one process.  The parent of
this model does not exist, so the library path of the same box is the only baseline.

Device events, warm-up, medians of N timed forwards per side; the two sides alternate for ``--rounds`` rounds and every
round prints one JSON line (the raw lines of profiles/swin_trunk_ab.txt and profiles/swin_384_teacher_ab.txt).

    python scripts/time_swin.py [--model NAME] [--img-size 224] [--batch 256] [--iters 10] [--rounds 3] [--once fused|library]
    python scripts/time_swin.py --model swin_base_patch4_window12_384 --img-size 384

``--once`` runs a few forwards of one side only (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="swin_tiny_patch4_window7_224")
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--once", choices=("fused", "library"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_swin.py needs the GPU: a CPU run says nothing about it")
    from basd_amd.models import load_teacher
    teacher = load_teacher(args.model, args.img_size, device="cuda")
    model = teacher.model
    assert model._fused is not None, model.fused_refusal()
    x = torch.randn(args.batch, 3, args.img_size, args.img_size, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def fused():
        with torch.no_grad():
            return model.forward_features(x)

    def library():
        with torch.no_grad():
            return model._forward_plain(x)

    if args.once:
        fn = fused if args.once == "fused" else library
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        return
    a, b = fused().float(), library().float()
    rel = float((a - b).norm() / b.norm())
    del a, b
    for r in range(max(args.rounds, 3)):
        out = {"model": args.model, "img_size": args.img_size, "batch": args.batch, "iters": args.iters, "round": r, "fused_vs_library_rel_l2": rel}
        for name in (("fused", "library") if r % 2 == 0 else ("library", "fused")):
            out[f"{name}_ms"] = median_ms(fused if name == "fused" else library, args.iters)
        out["library_over_fused"] = out["library_ms"]["median"] / out["fused_ms"]["median"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

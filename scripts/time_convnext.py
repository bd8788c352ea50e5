"""forward_features of the frozen convnextv2_tiny teacher at 224 px, bf16: the fused trunk (csrc/convnext.hip +
basd_gemm_bf16) against the plain-torch channels-last path of the same module (library convolutions), in one process.

Device events, warm-up, medians of N timed forwards per side, measured in both orders (fused first, then library
first).

    python scripts/time_convnext.py [--batch 256] [--iters 20] [--once fused|library]

``--once`` runs a few forwards of one side only (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, iters, warmup=5):
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
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model", default="convnextv2_tiny")
    ap.add_argument("--once", choices=("fused", "library"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_convnext.py needs the GPU: a CPU run says nothing about it")
    from basd_amd.models import load_teacher
    teacher = load_teacher(args.model, 224, device="cuda")
    model = teacher.model
    assert model._fused is not None, model.fused_refusal()
    x = torch.randn(args.batch, 3, 224, 224, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

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
    out = {"model": args.model, "batch": args.batch, "iters": args.iters, "fused_vs_library_rel_l2": rel}
    for order in (("fused", "library"), ("library", "fused")):
        for name in order:
            med, lo, hi = median_ms(fused if name == "fused" else library, args.iters)
            out[f"{name}_ms_{'first' if name == order[0] else 'second'}"] = {"median": med, "min": lo, "max": hi}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

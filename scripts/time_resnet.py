"""forward_features of the frozen resnet50 teacher at 224 px, bf16: the fused trunk (csrc/resnet.hip +
basd_gemm_bf16, BatchNorm folded) against the plain-torch channels-last path of the same module (library
convolutions, batch-norm and pooling), in one process.

Device events, warm-up, medians of N timed forwards per side, measured in both orders (fused first, then library
first).

    python scripts/time_resnet.py [--batch 256] [--iters 20] [--once fused|library]

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
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--once", choices=("fused", "library"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_resnet.py needs the GPU: a CPU run says nothing about it")
    from basd_amd.models import load_teacher
    teacher = load_teacher(args.model, 224, device="cuda")
    model = teacher.model
    # random BatchNorm statistics, as the accuracy tests use: the fold and the bias images carry weight in the printed
    # distances; the timing does not depend on the values
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.weight.shape
                m.weight.copy_(1.0 + 0.2 * torch.randn(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))
    assert model.prepare_fused(), model.fused_refusal()   # the weight images follow the statistics
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
    # which of the two bf16 paths is off: both against the fp32 forward of the same weights (library, 32 images at a time)
    import copy
    model32 = copy.deepcopy(model).float()
    with torch.no_grad():
        ref = torch.cat([model32._forward_plain(x[i:i + 32].float()) for i in range(0, args.batch, 32)])
    del model32
    out = {"model": args.model, "batch": args.batch, "iters": args.iters, "fused_vs_library_rel_l2": rel,
           "fused_vs_fp32_rel_l2": float((a - ref).norm() / ref.norm()),
           "library_vs_fp32_rel_l2": float((b - ref).norm() / ref.norm())}
    del a, b, ref
    for order in (("fused", "library"), ("library", "fused")):
        for name in order:
            med, lo, hi = median_ms(fused if name == "fused" else library, args.iters)
            out[f"{name}_ms_{'first' if name == order[0] else 'second'}"] = {"median": med, "min": lo, "max": hi}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

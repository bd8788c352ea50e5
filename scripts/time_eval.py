"""Evaluation-forward throughput of the c2 student (DeiT-Tiny/16, 224 x 224, 100 classes) at batch 256 and at a ragged
batch of 80, under the three evaluation precisions: "highest" (library fp32: hipBLASLt + SDPA), "high" (the split-bf16
kernels of csrc/eval_f32x3.hip) and bf16 autocast (the bf16 kernels).  Medians of CUDA-event brackets (GPU)."""
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from basd_amd.evaluation import matmul_precision
    from basd_amd.models.vit import create_vit
    torch.manual_seed(0)
    model = create_vit("deit_tiny_patch16_224", num_classes=100, img_size=224).cuda().eval()
    reps = int(os.environ.get("REPS", "20"))
    modes = {"highest": lambda: matmul_precision("highest"), "high": lambda: matmul_precision("high"),
             "bf16_autocast": lambda: torch.autocast("cuda", dtype=torch.bfloat16)}
    for batch in (256, 80):
        x = torch.randn(batch, 3, 224, 224, device="cuda")
        for name, ctx in modes.items():
            with ctx(), torch.no_grad():
                for _ in range(3):
                    model(x)
                times = []
                for _ in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    model(x)
                    b.record()
                    b.synchronize()
                    times.append(a.elapsed_time(b))
            times.sort()
            ms = times[len(times) // 2]
            print(f"batch {batch:4d} {name:14s} {ms:8.3f} ms  {batch / ms * 1e3:10.1f} img/s", flush=True)


if __name__ == "__main__":
    with contextlib.suppress(KeyboardInterrupt):
        main()

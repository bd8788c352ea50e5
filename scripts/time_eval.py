"""Evaluation-forward throughput of the c2 student (DeiT-Tiny/16, 224 x 224, 100 classes) at batch 256 and at a ragged
batch of 80, under the three evaluation precisions: "highest" (library fp32: hipBLASLt + SDPA), "high" (the split-bf16
kernels of csrc/eval_f32x3.hip) and bf16 autocast (the bf16 kernels).  Medians of CUDA-event brackets (GPU).

--img-size / --patch-size / --batch time another geometry (384 px: 577 tokens; --patch-size 14 at 384 px: 27 x 27
patches + CLS = 730 tokens on the 378 px the grid covers).  --no-long switches the tiled "high" attention off
in-process: a model with more than 272 tokens then takes the library fp32 path under "high", the route before the
tiled kernel existed, so both routes can be timed alternately in one session."""
import argparse
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--patch-size", type=int, default=16)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--no-long", action="store_true")
    args = ap.parse_args()
    from basd_amd.evaluation import matmul_precision
    from basd_amd.models.vit import create_vit
    torch.manual_seed(0)
    default = (args.img_size, args.patch_size, args.batch, args.no_long) == (224, 16, None, False)
    kw = {} if args.patch_size == 16 else {"patch_size": args.patch_size}
    model = create_vit("deit_tiny_patch16_224", num_classes=100, img_size=args.img_size, **kw).cuda().eval()
    side = args.img_size // args.patch_size * args.patch_size
    if args.no_long:
        import basd_amd._native as native
        native.attention_fwd_f32x3_long_supported = lambda t, hd: False
    if not default:
        print(f"img {args.img_size} (input {side} x {side}) patch {args.patch_size} tokens {model.pos_embed.shape[1]} "
              f"long kernel {'off' if args.no_long else 'on'}", flush=True)
    reps = int(os.environ.get("REPS", "20"))
    modes = {"highest": lambda: matmul_precision("highest"), "high": lambda: matmul_precision("high"),
             "bf16_autocast": lambda: torch.autocast("cuda", dtype=torch.bfloat16)}
    for batch in ((256, 80) if args.batch is None else (args.batch,)):
        x = torch.randn(batch, 3, side, side, device="cuda")
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
            spread = "" if default else f"  (min {times[0]:.3f} max {times[-1]:.3f} ms)"
            print(f"batch {batch:4d} {name:14s} {ms:8.3f} ms  {batch / ms * 1e3:10.1f} img/s{spread}", flush=True)


if __name__ == "__main__":
    with contextlib.suppress(KeyboardInterrupt):
        main()

"""MixUp / CutMix + soft targets of one batch (GPU): the torch chain of training/mixup.py (two lerps, or a copy and two
box pastes, then one_hot / float / roll / lerp) against basd_mixup_cutmix (csrc/mixup.hip), on the metric's batch
[256, 3, 224, 224] fp32 with 1000 classes, MixUp at lam = 0.3 and CutMix with the box of lam = 0.5 (158 x 158 pixels).

Both are enqueued ITERS times between two device events, torch and kernel alternately, ROUNDS times, after a warm-up of
each; the figure is the median of the rounds in microseconds per call, with the spread.  The host column is the enqueue
time alone (host clock around the same loop, no synchronise inside it): the chain runs outside the captured step, so
this is what it costs the step's host thread.  Achieved bytes / s are the ALGORITHMIC bytes over the device time: MixUp
two reads and one write of the batch, CutMix one read and one write, plus the labels and the target rows.  The launch
counts come from a torch profiler pass of one call each, after the timing; the results of the two are compared first."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as native  # noqa: E402
from basd_amd.training.mixup import _torch_chain  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
ROUNDS = int(os.environ.get("ROUNDS", "21"))


def kernel_chain(x, y, k, mode, lam, box, out, out_t):
    native.mixup_cutmix(x, y, k, mode, lam, box or (0, 0, 0, 0), out, out_t)


def bracket(fn, args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(ITERS):
        fn(*args)
    b.record()
    host = (time.perf_counter() - t0) / ITERS * 1e6
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3, host


def launches(fn, args):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(*args)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_mixup.py needs the GPU: there is nothing to time without one")
    torch.manual_seed(0)
    b, c, s, k = 256, 3, 224, 1000
    x = torch.randn(b, c, s, s, device="cuda")
    y = torch.randint(0, k, (b,), device="cuda")
    batch_bytes = x.numel() * x.element_size()
    small = y.numel() * 8 + b * k * 4
    cases = (("MixUp  lam 0.3", 0, 0.3, None, 3 * batch_bytes + small),
             ("CutMix lam 0.5", 1, 1.0 - 158 * 158 / float(s * s), (33, 191, 33, 191), 2 * batch_bytes + small))
    print(f"images [{b}, {c}, {s}, {s}] fp32 ({batch_bytes / 1e6:.1f} MB), {k} classes; ITERS {ITERS}, ROUNDS {ROUNDS}", flush=True)
    for name, mode, lam, box, algo in cases:
        outs = {n: (torch.empty_like(x), torch.empty(b, k, device="cuda")) for n in ("torch", "kernel")}
        chains = {"torch": _torch_chain, "kernel": kernel_chain}
        args = {n: (x, y, k, mode, lam, box, *outs[n]) for n in chains}
        for n in chains:
            for _ in range(5):
                chains[n](*args[n])
        torch.cuda.synchronize()
        d_img = float((outs["torch"][0] - outs["kernel"][0]).abs().max())
        d_tgt = float((outs["torch"][1] - outs["kernel"][1]).abs().max())
        print(f"{name}: images bitwise equal {torch.equal(outs['torch'][0], outs['kernel'][0])} (max |diff| {d_img:.3e}), "
              f"targets max |diff| {d_tgt:.3e}; algorithmic bytes {algo / 1e6:.1f} MB", flush=True)
        times = {n: [] for n in chains}
        for _ in range(ROUNDS):
            for n in chains:
                times[n].append(bracket(chains[n], args[n]))
        for n in chains:
            dev = sorted(t[0] for t in times[n])
            host = sorted(t[1] for t in times[n])
            med = dev[len(dev) // 2]
            try:
                count = str(launches(chains[n], args[n]))
            except Exception as exc:                                                    # a profiler that does not start
                count = f"not measured ({type(exc).__name__})"
            print(f"  {n:6s} device {med:8.2f} us / call (min {dev[0]:.2f} max {dev[-1]:.2f})  {algo / med / 1e6:6.2f} TB/s algorithmic   "
                  f"host enqueue {host[len(host) // 2]:7.2f} us / call (min {host[0]:.2f} max {host[-1]:.2f})   "
                  f"device launches per call: {count}", flush=True)


if __name__ == "__main__":
    main()

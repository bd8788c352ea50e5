"""Per-batch cost of evaluate_model's accounting behind the forward (GPU): the torch chain it ran before the fused
tally (float / index_select / topk / eq / any / sums / cross-entropy / fp64 adds) against basd_cls_tally
(csrc/eval_tally.hip), on fp32 logits [256, 1000], all classes and a 200-class subset.

Both are enqueued ITERS times between two device events (one batch is far below a timing window), torch and kernel
alternately, ROUNDS times; the figure is the median of the rounds in microseconds per batch, with the spread.  A third
column gives the host-side enqueue time alone (no synchronise inside the window): the loop of evaluate_model never waits
for the device, so whichever of the two is larger is what a batch costs.  The launch counts come from a torch profiler
pass of one batch each, after the timing.

--model adds evaluate_model end to end on the c2 student (DeiT-Tiny/16, 224 x 224, 1000 classes) over 8 device batches
of 256, under fp32 "high" and bf16 autocast: img/s with the torch accounting (a provider without the fused tally) and
with the kernel, alternately, medians of 7 (host clock around the call, which ends in the tally's read-back)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as native  # noqa: E402

ITERS = int(os.environ.get("ITERS", "200"))
ROUNDS = int(os.environ.get("ROUNDS", "11"))


def torch_chain(logits, y, keep, tally, criterion, num_classes):
    """the accounting of evaluate_model before the fused tally, line by line"""
    logits = logits.float()
    if keep is not None:
        logits = logits.index_select(1, keep)
    top = logits.topk(min(5, num_classes, logits.shape[1]), dim=1).indices
    hit = top.eq(y.unsqueeze(1))
    tally[0] += hit[:, 0].sum()
    tally[1] += hit.any(dim=1).sum()
    tally[2] += criterion(logits, y).double() * y.numel()
    tally[3] += y.numel()


def kernel_chain(logits, y, keep, tally, criterion, num_classes):
    k = logits.shape[1] if keep is None else keep.numel()
    native.cls_tally(logits, y, tally, keep=keep, top_k=min(5, num_classes, k), smoothing=criterion.label_smoothing)


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
    torch.manual_seed(0)
    criterion = torch.nn.CrossEntropyLoss()
    b, c = 256, 1000
    logits = 3.0 * torch.randn(b, c, device="cuda")
    for name, keep in (("all 1000 classes", None), ("200-class subset", torch.randperm(c, device="cuda")[:200])):
        k = c if keep is None else keep.numel()
        y = torch.randint(0, k, (b,), device="cuda")
        tallies = {"torch": torch.zeros(4, dtype=torch.float64, device="cuda"),
                   "kernel": torch.zeros(4, dtype=torch.float64, device="cuda")}
        chains = {"torch": torch_chain, "kernel": kernel_chain}
        args = {n: (logits, y, keep, tallies[n], criterion, k) for n in chains}
        for n in chains:
            for _ in range(20):
                chains[n](*args[n])
        times = {n: [] for n in chains}
        for _ in range(ROUNDS):
            for n in chains:
                times[n].append(bracket(chains[n], args[n]))
        rows = tallies["torch"][3].item()
        assert rows == tallies["kernel"][3].item()
        same = (tallies["torch"][:2] == tallies["kernel"][:2]).all().item()        # tie-free random logits
        rel = abs(tallies["torch"][2].item() - tallies["kernel"][2].item()) / abs(tallies["kernel"][2].item())
        print(f"logits [{b}, {c}] fp32, {name}: hit counts equal {same}, summed loss differs by {rel:.2e} relative", flush=True)
        for n in chains:
            dev = sorted(t[0] for t in times[n])
            host = sorted(t[1] for t in times[n])
            try:
                count = str(launches(chains[n], args[n]))
            except Exception as exc:                                                    # a profiler that does not start
                count = f"not measured ({type(exc).__name__})"
            print(f"  {n:6s} device {dev[len(dev) // 2]:8.2f} us / batch (min {dev[0]:.2f} max {dev[-1]:.2f})   "
                  f"host enqueue {host[len(host) // 2]:8.2f} us / batch   device launches per batch: {count}", flush=True)


def evaluate_rate():
    import types

    from basd_amd.evaluation import evaluate_model, matmul_precision
    from basd_amd.losses import _ops
    from basd_amd.models.vit import create_vit
    torch.manual_seed(0)
    model = create_vit("deit_tiny_patch16_224", num_classes=1000, img_size=224).cuda().eval()
    batches = [{"pixel_values": torch.randn(256, 3, 224, 224, device="cuda"),
                "label": torch.randint(0, 1000, (256,), device="cuda")} for _ in range(8)]
    criterion = torch.nn.CrossEntropyLoss()
    without = types.SimpleNamespace(**{n: getattr(native, n) for n in dir(native)
                                       if not n.startswith("__") and n not in ("cls_tally", "cls_tally_supported")})
    modes = {"high": lambda: matmul_precision("high"),
             "bf16_autocast": lambda: torch.autocast("cuda", dtype=torch.bfloat16)}
    for mode, ctx in modes.items():
        times, results = {"torch": [], "kernel": []}, {}
        with ctx():
            for r in range(8):                                   # the first round warms both up
                for name, provider in (("torch", without), ("kernel", None)):
                    _ops.set_ops(provider)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    results[name] = evaluate_model(model, batches, criterion, num_classes=1000)
                    if r:
                        times[name].append(time.perf_counter() - t0)
        _ops.set_ops(None)
        for name, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            print(f"evaluate_model {mode:14s} {name:6s} {2048 / med:9.1f} img/s  ({med / 8 * 1e3:.3f} ms / batch, "
                  f"min {ts[0] / 8 * 1e3:.3f} max {ts[-1] / 8 * 1e3:.3f})  {results[name]}", flush=True)


if __name__ == "__main__":
    main()
    if "--model" in sys.argv[1:]:
        evaluate_rate()

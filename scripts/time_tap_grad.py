"""Gradient of the tapped student tokens (GPU): the torch chains of the parent against the two entries of
csrc/tap_grad.hip, at the shapes of c2 (B 256, N 196, T 197, D_s 192, E 4) and c4 (B 128, D_s 384).

  selector   per tap s.float(), mean, 1 x D x D product, fp32 addmm, cast     vs  basd_selector_token_grad (all taps)
  tap        per tap g_a + g_b, zeros, strided copy into [:, 1:, :], + g_out   vs  basd_tap_grad_scatter (per tap)

Both sides are enqueued ITERS times between two device events, torch and kernel alternately, ROUNDS times, after a
warm-up of each; the figure is the median of the rounds in microseconds per call (all E taps), with the spread.  The
launch counts come from a torch profiler pass of one call each.  ``--resources`` prints the compiler's resource report
of the three kernels instead (needs hipcc, no GPU)."""
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import basd_amd._native as native  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
ROUNDS = int(os.environ.get("ROUNDS", "15"))


def resources():
    src = os.path.join(native.CSRC, "tap_grad.hip")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull], capture_output=True, text=True)
    keep = ("Function Name", "VGPRs:", "AGPRs:", "ScratchSize", "Occupancy", "LDS Size")
    for line in res.stderr.splitlines():
        if any(k in line for k in keep):
            print(line.split("remark:")[-1].rstrip().replace(" [-Rpass-analysis=kernel-resource-usage]", ""))


def torch_selector(toks, w):
    out = []
    for i, s in enumerate(toks):
        sf = s.float().reshape(-1, s.shape[-1])
        row = -(sf.mean(dim=0, keepdim=True) @ w[i])
        out.append(torch.addmm(row, sf, w[i]).reshape(s.shape).to(s.dtype))
    return out


def torch_tap(g_out, g_a, g_b):
    out = []
    for go, ga, gb in zip(g_out, g_a, g_b):
        r = ga + gb
        z = torch.zeros_like(go)
        z[:, 1:, :].copy_(r)
        out.append(go + z)
    return out


def kernel_tap(g_out, g_a, g_b):
    return [native.tap_grad_scatter(go, ga, gb, tuple(go.shape), 1) for go, ga, gb in zip(g_out, g_a, g_b)]


def bracket(fn, args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ITERS):
        fn(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3


def launches(fn, args):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(*args)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def compare(name, torch_fn, kernel_fn, args, nbytes):
    for fn in (torch_fn, kernel_fn):
        for _ in range(3):
            fn(*args)
    t_us, k_us = [], []
    for _ in range(ROUNDS):
        t_us.append(bracket(torch_fn, args))
        k_us.append(bracket(kernel_fn, args))
    tm, km = statistics.median(t_us), statistics.median(k_us)
    print(f"  {name:9s} torch {tm:8.1f} us [{min(t_us):.1f} .. {max(t_us):.1f}] {launches(torch_fn, args):3d} launches | "
          f"kernel {km:8.1f} us [{min(k_us):.1f} .. {max(k_us):.1f}] {launches(kernel_fn, args):3d} launches | "
          f"x{tm / km:.2f}, {nbytes / km / 1e6:.2f} TB/s of the necessary bytes")


def main():
    if "--resources" in sys.argv:
        return resources()
    if not torch.cuda.is_available():
        raise SystemExit("time_tap_grad.py needs the GPU: there is nothing to time without one")
    torch.manual_seed(0)
    for label, b, d, e in (("c2", 256, 192, 4), ("c4", 128, 384, 4)):
        n, t = 196, 197
        outs = [torch.randn(b, t, d, device="cuda").bfloat16() for _ in range(e)]
        toks = [o[:, 1:, :] for o in outs]
        w = torch.randn(e, d, d, device="cuda") / d ** 0.5
        g_out = [torch.randn(b, t, d, device="cuda").bfloat16() for _ in range(e)]
        g_a = [torch.randn(b, n, d, device="cuda").bfloat16() for _ in range(e)]
        g_b = [torch.randn(b, n, d, device="cuda").bfloat16() for _ in range(e)]
        got, want = native.selector_token_grad(toks, w), torch_selector(toks, w)
        worst = max(float((x.float() - y.float()).abs().max()) for x, y in zip(got, want))
        same = all(torch.equal(x, y) for x, y in zip(kernel_tap(g_out, g_a, g_b), torch_tap(g_out, g_a, g_b)))
        print(f"{label}: B {b} N {n} T {t} D_s {d} E {e}; selector kernel vs torch chain max |diff| {worst:.3g}, "
              f"scatter bit-equal: {same}")
        tok_bytes = b * n * d * 2
        compare("selector", torch_selector, native.selector_token_grad, (toks, w), e * 2 * tok_bytes)
        compare("tap", torch_tap, kernel_tap, (g_out, g_a, g_b), e * (2 * tok_bytes + 2 * b * t * d * 2))


if __name__ == "__main__":
    main()

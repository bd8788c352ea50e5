"""The way back from the Procrustes backward's (g_t on the student grid, g_a) to the caller's teacher tokens and
importance (GPU): the parent's torch chain of ``_ProcrustesFn.backward`` (dense resample matrix with fp64 taps and two
index_put_, three library products, four pointwise / reduction launches) against the two entries of
csrc/resample.hip (basd_resample_tokens_adjoint + basd_procrustes_importance_bwd), at

  default    E B = 1024, 256 -> 196, D_t =  768   (a /16 student against dinov2_vitb14)
  c5         E B = 1024, 256 -> 196, D_t = 1280   (ViT-B/16 student, ViT-H/14 teacher)
  cross-arch E B =  512,  49 -> 196, D_t =  768   (ConvNeXt-V2 map of 7 x 7 tokens)

Both sides are enqueued ITERS times between two device events, torch and entries alternately, ROUNDS times, after a
warm-up of each; the figure is the median of the rounds in microseconds per call with the spread.  The adjoint alone is
bracketed the same way and reported with its achieved bytes / s over the algorithmic bytes batch (n_in + n_out) d 4.
The launch counts come from a torch profiler pass of one call each.  ``--resources`` prints the compiler's resource
report of the kernels instead (needs hipcc, no GPU)."""
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import basd_amd._native as native  # noqa: E402
from basd_amd.losses.functional import resample_matrix  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
ROUNDS = int(os.environ.get("ROUNDS", "15"))


def resources():
    src = os.path.join(native.CSRC, "resample.hip")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull], capture_output=True, text=True)
    keep = ("Function Name", "VGPRs:", "AGPRs:", "ScratchSize", "Occupancy", "LDS Size")
    for line in res.stderr.splitlines():
        if any(k in line for k in keep):
            print(line.split("remark:")[-1].rstrip().replace(" [-Rpass-analysis=kernel-resource-usage]", ""))


def torch_chain(g_t, g_a, a, imp, n_t):
    n_s = g_t.shape[1]
    r = resample_matrix(n_t, n_s, g_t.device)
    tot = (imp @ r.t()).sum(-1, keepdim=True)
    g_raw = (g_a - (a * g_a).sum(-1, keepdim=True)) / tot
    return torch.matmul(r.t(), g_t), g_raw @ r


def entries(g_t, g_a, a, imp, n_t):
    return native.resample_tokens_adjoint(g_t, n_t), native.procrustes_importance_bwd(g_a, a, imp)


def adjoint_only(g_t, g_a, a, imp, n_t):
    return native.resample_tokens_adjoint(g_t, n_t)


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


def main():
    if "--resources" in sys.argv:
        return resources()
    if not torch.cuda.is_available():
        raise SystemExit("time_resample_bwd.py needs the GPU: there is nothing to time without one")
    torch.manual_seed(0)
    for label, batch, n_t, n_s, d in (("default", 1024, 256, 196, 768), ("c5", 1024, 256, 196, 1280),
                                      ("cross-arch", 512, 49, 196, 768)):
        g_t = torch.randn(batch, n_s, d, device="cuda")
        g_a = torch.randn(batch, n_s, device="cuda")
        imp = torch.rand(batch, n_t, device="cuda") + 0.1
        v = imp @ resample_matrix(n_t, n_s, "cuda").t()
        a = (v / v.sum(-1, keepdim=True)).contiguous()
        args = (g_t, g_a, a, imp, n_t)
        want, got = torch_chain(*args), entries(*args)
        worst_t = float((got[0] - want[0]).abs().max() / want[0].abs().max())
        worst_i = float((got[1] - want[1]).abs().max() / want[1].abs().max())
        print(f"{label}: E B {batch}, {n_t} -> {n_s}, D_t {d}; entries vs torch chain, max |diff| / max |value|: "
              f"g_t {worst_t:.3g}, g_imp {worst_i:.3g}")
        for fn in (torch_chain, entries, adjoint_only):
            for _ in range(3):
                fn(*args)
        t_us, k_us, a_us = [], [], []
        for _ in range(ROUNDS):
            t_us.append(bracket(torch_chain, args))
            k_us.append(bracket(entries, args))
            a_us.append(bracket(adjoint_only, args))
        tm, km, am = (statistics.median(x) for x in (t_us, k_us, a_us))
        nbytes = batch * (n_t + n_s) * d * 4
        print(f"  torch chain {tm:8.1f} us [{min(t_us):.1f} .. {max(t_us):.1f}] {launches(torch_chain, args):3d} launches | "
              f"entries {km:8.1f} us [{min(k_us):.1f} .. {max(k_us):.1f}] {launches(entries, args):3d} launches | "
              f"x{tm / km:.2f}")
        print(f"  adjoint alone {am:8.1f} us [{min(a_us):.1f} .. {max(a_us):.1f}]: {nbytes / 1e6:.0f} MB algorithmic, "
              f"{nbytes / am / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()

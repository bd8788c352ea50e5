"""Short attention backward (basd_attention_bwd_bf16): time per launch from device events (GPU).

    python scripts/time_attention_bwd.py [--reps 3] [--iters 200]

Prints, per shape, the median launch time of each repetition, the effective bandwidth over the algorithmic bytes (qkv,
O, dO read once, dqkv written once, LSE) and the rel-L2 error of dQ / dK / dV against fp64 autograd on the first two
images.  A bracket around one launch from Python cannot resolve a kernel of about 10 us (the host's launch cadence is
longer: the bracket then holds the wait for the next submission), so every repetition also times a captured graph of
GRAPH_LAUNCHES launches, replayed, per launch; a kernel trace (rocprofv3 --kernel-trace --stats -- python
scripts/time_attention_bwd.py --reps 1) gives the same figure per dispatch.  A/B of two builds: run once per library
with BASD_LIB pointing at the other build, alternating the two."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat
from tests import _attn_regimes as R

SHAPES = [(256, 197, 3), (64, 65, 3)]     # the headline student, configuration c1's student
GRAPH_LAUNCHES = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    hd, scale = 64, 64 ** -0.5
    print(f"library {nat.LIB_PATH}")
    for B, T, H in SHAPES:
        g = torch.Generator().manual_seed(B * 1000 + T)
        qkv = torch.randn(B, T, 3 * H * hd, generator=g).bfloat16().cuda()
        dout = torch.randn(B, T, H * hd, generator=g).bfloat16().cuda()
        out, _, lse = nat.attention_fwd(qkv, H, hd, scale, want_lse=True)
        run = lambda: nat.attention_bwd(qkv, out, dout, lse, H, hd, scale)
        for _ in range(20):
            dqkv = run()
        torch.cuda.synchronize()
        ref = R.bwd_autograd(qkv[:2], dout[:2], H, hd, scale)
        errs = [R.rel(a, b) for a, b in zip(R.dqkv_parts(dqkv[:2], H, hd), ref)]
        mb = (2 * qkv.numel() + 2 * out.numel()) * 2 / 1e6 + lse.numel() * 4 / 1e6
        meds = []
        for _ in range(args.reps):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
            for a, b in ev:
                a.record()
                run()
                b.record()
            torch.cuda.synchronize()
            meds.append(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(GRAPH_LAUNCHES):
                run()
        graph.replay()
        torch.cuda.synchronize()
        gmeds = []
        for _ in range(args.reps):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for a, b in ev:
                a.record()
                graph.replay()
                b.record()
            torch.cuda.synchronize()
            gmeds.append(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3 / GRAPH_LAUNCHES)
        print(f"B {B} T {T} H {H}: medians " + " ".join(f"{m:.1f}" for m in meds) + " us, in a graph "
              + " ".join(f"{m:.1f}" for m in gmeds) + f" us  {mb:.1f} MB  "
              f"{mb / min(gmeds):.2f} MB/us at the best  rel L2 dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")


if __name__ == "__main__":
    main()

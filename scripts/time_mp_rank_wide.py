"""The start-up Marchenko-Pastur rank past 1024 channels: ``marchenko_pastur_rank_wide`` at the ViT-H/14 calibration
shape (16 896 x 1280) and at 20 482 x 2048, split into its three stages (fp64 Gram, Householder tridiagonal reduction,
Sturm count), and at 5000 x 1024 next to ``marchenko_pastur_rank`` (the full-spectrum route: the only one before).
Medians of device-event brackets; the two whole calls include their one synchronising ``.item()``.

    python scripts/time_mp_rank_wide.py [--reps 5] > profiles/mp_rank_wide.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat                                                   # noqa: E402
from basd_amd.losses import marchenko_pastur_rank, marchenko_pastur_rank_wide    # noqa: E402
from basd_amd.losses.layer_selector import _gram_slabs                           # noqa: E402


def bracket(f, reps):
    """median / min ms of ``reps`` device-event brackets around f(), after one warm-up call"""
    f()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def planted(m, d, r, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (3.0 * (torch.randn(m, r, device="cuda", generator=g) @ torch.randn(r, d, device="cuda", generator=g)) / r ** 0.5
            + torch.randn(m, d, device="cuda", generator=g))


def stages(x, reps):
    m, d = x.shape
    n = min(m, d)
    xt = x if m >= d else x.t()
    k = xt.shape[0]
    slabs = _gram_slabs(k)
    k_pad = -(-k // (4 * slabs)) * (4 * slabs)
    xs = torch.zeros(k_pad, n, device="cuda")
    xs[:k] = xt
    xs = xs.view(slabs, k_pad // slabs, n)

    def gram():
        g = nat.bgemm_f64(xs, xs, trans_a=True, symmetric=True)
        return g.sum(dim=0) if slabs > 1 else g[0]

    g0 = gram().contiguous()
    diag, off = nat.sym_tridiag(g0.clone())
    t_gram = bracket(gram, reps)
    scratch = g0.clone()

    def reduce():
        scratch.copy_(g0)                       # the reduction overwrites its input: one [n, n] copy inside the bracket
        nat.sym_tridiag(scratch)

    t_red = bracket(reduce, reps)
    t_cnt = bracket(lambda: nat.tridiag_mp_rank(diag, off, m, d, n), reps)
    return slabs, t_gram, t_red, t_cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; ms as median (min) of {args.reps} device-event brackets after one warm-up")
    for m, d, r in ((16896, 1280, 160), (20482, 2048, 200), (5000, 1024, 80)):
        x = planted(m, d, r, m + d)
        n = min(m, d)
        slabs, t_gram, t_red, t_cnt = stages(x, args.reps)
        ranks = []
        t_all = bracket(lambda: ranks.append(marchenko_pastur_rank_wide(x)), args.reps)
        print(f"{m} x {d}: marchenko_pastur_rank_wide rank {ranks[-1]}  whole call {t_all[0]:8.2f} ({t_all[1]:.2f}) ms")
        print(f"    Gram ({slabs} slab{'s' if slabs > 1 else ''} of bgemm_f64{' + sum' if slabs > 1 else ''}) "
              f"{t_gram[0]:8.2f} ({t_gram[1]:.2f}) ms")
        print(f"    sym_tridiag ({2 * (n - 2) + 1} launches)      {t_red[0]:8.2f} ({t_red[1]:.2f}) ms")
        print(f"    tridiag_mp_rank (one workgroup)   {t_cnt[0]:8.2f} ({t_cnt[1]:.2f}) ms")
        if n <= 1024:
            old = []
            t_old = bracket(lambda: old.append(marchenko_pastur_rank(x)), args.reps)
            print(f"{m} x {d}: marchenko_pastur_rank      rank {old[-1]}  whole call {t_old[0]:8.2f} ({t_old[1]:.2f}) ms"
                  "   (full spectrum: the route before)")
    nat.check_status("cuda")


if __name__ == "__main__":
    main()

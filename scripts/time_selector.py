"""Timing of the selector forward at c2 shapes (GPU): the torch composition of rounds 1 - 4 against the two C entries
(basd_selector_frames / basd_selector_weights).  Both run the same per-layer Gram kernels; the old composition is the
same package code with a provider that hides the two entries.  Medians of device-event brackets.

    python scripts/time_selector.py [--reps 30] [--batch 8]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat                                    # noqa: E402
from basd_amd.losses import _ops                                 # noqa: E402
from basd_amd.losses import functional as BF                     # noqa: E402


class _Composition:
    """the native provider without the selector entries: functional.py takes the torch composition"""

    def __getattr__(self, name):
        if name in ("selector_frames", "selector_weights"):
            raise AttributeError(name)
        return getattr(nat, name)


def bracket(fn, reps):
    out = []
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    B, N, D_s, D_t, L, E = args.batch, 196, 192, 768, 12, 4
    teacher = [torch.randn(B, N, D_t, device="cuda", generator=g).bfloat16() for _ in range(L)]
    students = [torch.randn(B, N, D_s, device="cuda", generator=g).bfloat16() for _ in range(E)]
    proj_s = torch.linalg.qr(torch.randn(D_s, D_s, device="cuda", generator=g))[0].contiguous()
    proj_t = torch.linalg.qr(torch.randn(D_t, D_s, device="cuda", generator=g))[0].t().contiguous()
    log_t = torch.full((E,), 0.5413, device="cuda")
    grams = [BF.teacher_gram(t, proj_t) for t in teacher]

    def frames():
        return BF.teacher_frames(teacher, proj_t, grams=grams), BF.student_frames(students, proj_s)

    def weights(fr):
        return lambda: BF.selector_weights(students, teacher, proj_s, proj_t, log_t, frames=fr[0], pre_student=fr[1])

    def whole():
        fr = frames()
        return weights(fr)()

    rows = {}
    for label, provider in (("composition", _Composition()), ("C entries", nat)):
        _ops.set_ops(provider)
        with torch.no_grad():
            fr = frames()
            rows[label] = (bracket(frames, args.reps), bracket(weights(fr), args.reps), bracket(whole, args.reps))
            w = weights(fr)()[0]
        torch.cuda.synchronize()
        rows[label] += (w.cpu(),)
    _ops.set_ops(None)
    print(f"selector forward, c2 shapes (B = {B}, L = {L}, E = {E}, D_s = {D_s}), ms: median [min, max] of {args.reps}")
    for label, (fr, wt, wh, _) in rows.items():
        fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}]"
        print(f"  {label:12s} frames (teacher from Grams + student) {fmt(fr)}   weights {fmt(wt)}   both {fmt(wh)}")
    print(f"  weights max |diff| {float((rows['composition'][3] - rows['C entries'][3]).abs().max()):.2e}")
    nat.check_status()


if __name__ == "__main__":
    main()

"""The frozen vit_base_patch16_clip_quickgelu_224 teacher at 224 px, bf16, two measurements in one process each.

``forward`` (default): forward_features with the fused dispatch -- QuickGELU in the fc1 GEMM's epilogue
(basd_gemm_bf16_act), token assembly + norm_pre in one kernel (basd_vit_embed_bf16) -- against the SAME model with that
dispatch switched off (models/vit.py, _FUSED_CLIP_DISPATCH: bias-only GEMM + QuickGELU as torch ops, torch cat + add +
the LayerNorm kernel).  The two sides alternate for ``--rounds`` rounds; every round prints one JSON line (the raw lines
of profiles/clip_teacher_ab.txt).

``fc1``: the fc1 GEMM of ViT-B at M = batch * 197 = 50 432, N = 3072, K = 768 with each activation epilogue, through the
C entries of the library named by BASD_LIB (default: the in-tree one).  A library without basd_gemm_bf16_act (the parent
commit's) times its erf-GELU epilogue only: run it twice for the parent's own spread, then the in-tree library.

Device events, warm-up, medians of N timed calls.

    python scripts/time_clip_teacher.py [forward|fc1] [--batch 256] [--iters 10] [--rounds 3]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = "vit_base_patch16_clip_quickgelu_224"


def median_ms(fn, iters, warmup=3):
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
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def forward(args):
    import basd_amd.models.vit as V
    from basd_amd.models import load_teacher
    model = load_teacher(MODEL, 224, device="cuda").model
    x = torch.randn(args.batch, 3, 224, 224, device="cuda").to(torch.bfloat16)

    def run(fused_dispatch):
        V._FUSED_CLIP_DISPATCH = fused_dispatch
        try:
            with torch.no_grad():
                return model.forward_features(x)
        finally:
            V._FUSED_CLIP_DISPATCH = True

    sides = {"fused": lambda: run(True), "unfused": lambda: run(False)}
    a, b = sides["fused"]().float(), sides["unfused"]().float()
    rel = float((a - b).norm() / b.norm())
    del a, b
    for r in range(max(args.rounds, 3)):
        out = {"model": MODEL, "batch": args.batch, "iters": args.iters, "round": r, "fused_vs_unfused_rel_l2": rel}
        for name in (("fused", "unfused") if r % 2 == 0 else ("unfused", "fused")):
            out[f"{name}_ms"] = median_ms(sides[name], args.iters)
        out["unfused_over_fused"] = out["unfused_ms"]["median"] / out["fused_ms"]["median"]
        print(json.dumps(out), flush=True)


def fc1(args):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.environ.get("BASD_LIB") or os.path.join(here, "vit-bias-aware-structural-distillation_amd", "libbasd_hip.so")
    lib = ctypes.CDLL(path)
    sig = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.basd_gemm_bf16.argtypes = sig
    has_act = hasattr(lib, "basd_gemm_bf16_act")
    if has_act:
        lib.basd_gemm_bf16_act.argtypes = sig
    M, N, K = args.batch * 197, 3072, 768
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, device="cuda", generator=g).bfloat16()
    y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)

    def call(entry, code):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = entry(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, code, 0, st)
        assert rc == 0, rc

    cases = [("erf_gelu_epilogue2", lib.basd_gemm_bf16, 2), ("bias_epilogue1", lib.basd_gemm_bf16, 1)]
    if has_act:
        cases += [("act1_erf", lib.basd_gemm_bf16_act, 1), ("act2_quick_gelu", lib.basd_gemm_bf16_act, 2),
                  ("act3_gelu_tanh", lib.basd_gemm_bf16_act, 3)]
    for r in range(max(args.rounds, 3)):
        out = {"lib": os.path.relpath(path, here), "M": M, "N": N, "K": K, "iters": args.iters, "round": r}
        for name, entry, code in (cases if r % 2 == 0 else cases[::-1]):
            out[f"{name}_us"] = {k: round(1e3 * v, 2) for k, v in
                                 median_ms(lambda: call(entry, code), args.iters).items()}
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", choices=("forward", "fc1"), default="forward")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_clip_teacher.py needs the GPU: a CPU run says nothing about it")
    (forward if args.what == "forward" else fc1)(args)


if __name__ == "__main__":
    main()

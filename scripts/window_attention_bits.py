"""Bit comparison of the two window attention entries (csrc/swin.hip, csrc/swin_wide.hip) between two builds of the
library loaded into one process: the in-tree one and --parent <libbasd_hip.so of the commit to compare with>.  Neither
kernel has atomics or an order that depends on the schedule, so a refactor of the two files has to reproduce the whole
[B, H, W, ld_out] buffer, pad columns included, bit for bit.  Inputs of tests/test_swin_kernels_gpu._qkv; every row of
WA_CASES and WIDE_CASES, then every window 1 .. 8 on a 2 ws x 3 ws grid and 9 .. 16 on a 2 ws x 2 ws grid at shift 0,
ws // 2 and ws - 1, logit gain 1 and 30, heads 2, ld_qkv 192, ld_out 64 and 96.  One line per call; exit status 1 if
any bit differs or a NaN of the fill is left.

    python scripts/window_attention_bits.py --parent /path/to/parent/libbasd_hip.so > profiles/<name>.txt"""
import argparse, ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat
from tests import _swin_ref as R
from tests.test_swin_kernels_gpu import WA_CASES, _qkv
from tests.test_swin_wide_kernels_gpu import WIDE_CASES
from time_attention import P, load_parent

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="the other build of libbasd_hip.so")
args = ap.parse_args()

NAMES = ("basd_window_attention_fwd_bf16", "basd_window_attention_fwd_wide_bf16")
new, old = nat.lib(), load_parent(args.parent, NAMES)
SCALE = 32 ** -0.5
bad = 0


def compare(label, qkv, bias_of, B, H, W, ws, shift, heads, ld_out):
    """one call of the window's entry on both builds into NaN-filled buffers"""
    global bad
    name, bias = NAMES[ws > 8], bias_of(ws > 8)
    res = []
    for lib in (old, new):
        out = torch.full((B, H, W, ld_out), float("nan"), dtype=torch.bfloat16, device="cuda")
        rc = getattr(lib, name)(P(qkv), P(bias), B, H, W, heads, 32 * heads, ws, shift, qkv.shape[3], ld_out,
                                ctypes.c_float(SCALE), P(out), nat._stream())
        assert rc == 0, (label, rc)
        torch.cuda.synchronize()
        res.append(out)
    ok = bool(torch.equal(res[0].view(torch.int16), res[1].view(torch.int16))) and not bool(torch.isnan(res[1].float()).any())
    bad += not ok
    print(f"{label}: {'identical' if ok else 'DIFFERS'}", flush=True)


def biases(ws, heads, seed):
    """-> bias_of(wide): the fp32 table for the wide entry, its [heads, 64, 64] image for the other"""
    table = 0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=torch.Generator().manual_seed(seed))
    return lambda wide: table.cuda() if wide else nat.window_bias_image(R.expand_bias(table, ws).cuda())


print(f"# window attention entries, the in-tree library against --parent {os.path.basename(args.parent)}, one process; "
      "inputs of tests/test_swin_kernels_gpu._qkv; the whole output buffer compared as integers")
for B, H, W, ws, shift, heads, ld_qkv, ld_out, gain in WA_CASES + WIDE_CASES:
    qkv = _qkv(B, H, W, heads, ld_qkv, gain, seed=H + W + ws).cuda()
    compare(f"case  B {B} grid {H:2d} x {W:2d} ws {ws:2d} shift {shift:2d} heads {heads:2d} ld_qkv {ld_qkv:4d} ld_out {ld_out:3d} "
            f"gain {gain:4.1f}", qkv, biases(ws, heads, H * W + heads), B, H, W, ws, shift, heads, ld_out)
B, heads, ld_qkv = 2, 2, 192
for ws in range(1, 17):
    H, W = 2 * ws, (3 if ws <= 8 else 2) * ws
    bias_of = biases(ws, heads, ws)
    for gain in (1.0, 30.0):
        qkv = _qkv(B, H, W, heads, ld_qkv, gain, seed=H + W + ws).cuda()
        for shift in sorted({0, ws // 2, ws - 1}):
            for ld_out in (64, 96):
                compare(f"sweep B {B} grid {H:2d} x {W:2d} ws {ws:2d} shift {shift:2d} heads {heads:2d} ld_qkv {ld_qkv:4d} "
                        f"ld_out {ld_out:3d} gain {gain:4.1f}", qkv, bias_of, B, H, W, ws, shift, heads, ld_out)
print("ALL IDENTICAL" if not bad else f"{bad} COMPARISONS DIFFER")
sys.exit(1 if bad else 0)

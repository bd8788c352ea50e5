"""The two window attention entries (csrc/swin.hip, csrc/swin_wide.hip), this build against --parent <another build of
libbasd_hip.so> in one process, at batch 256 on the eight shapes the presets launch: Swin-T at 224 px (window 7, grids
56 / 28 / 14 / 7, heads 3 / 6 / 12 / 24) and Swin-B window 12 at 384 px (grids 96 / 48 / 24 / 12, heads 4 / 8 / 16 /
32), row widths from the model (`_qkv_width`, `row_width`), shift ws // 2 where the grid is larger than the window.
Brackets of --iters calls between device events, alternated parent, this build, parent, ...; a shape passes when this
build's median lies inside the spread of the parent's own brackets or below it (time_attention.ab_row).

    python scripts/time_window_attention.py --parent /path/to/parent/libbasd_hip.so > profiles/<name>.txt"""
import argparse, ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basd_amd._native as nat
from basd_amd.models.fused_trunk import row_width
from basd_amd.models.swin import SWIN_PRESETS, relative_position_index
from time_attention import P, ab_row, load_parent

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="another build of libbasd_hip.so, loaded into the same process")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()

NAMES = ("basd_window_attention_fwd_bf16", "basd_window_attention_fwd_wide_bf16")
parent = load_parent(args.parent, NAMES)
B, scale, st = args.batch, ctypes.c_float(32 ** -0.5), nat._stream()
print(f"# window attention entries at batch {B}, the in-tree library against --parent {os.path.basename(args.parent)}; "
      f"{args.runs} + {args.runs + 1} alternated brackets of {args.iters} calls, ms per call")
for preset, img in (("swin_tiny_patch4_window7_224", 224), ("swin_base_patch4_window12_384", 384)):
    with torch.device("meta"):
        model = SWIN_PRESETS[preset]()                 # only its widths are read
    ws = model.window_size
    for i, (c, heads) in enumerate(zip(model.dims, model.heads)):
        grid, ld = img // (4 << i), row_width(c)
        ld_qkv, shift = model._qkv_width(c, ld), ws // 2 if grid > ws else 0
        qkv = torch.randn(B, grid, grid, ld_qkv, device="cuda").bfloat16()
        out = torch.empty(B, grid, grid, ld, dtype=torch.bfloat16, device="cuda")
        table = 0.5 * torch.randn((2 * ws - 1) ** 2, heads, device="cuda")
        index = relative_position_index(ws).reshape(-1).cuda()
        bias = table if ws > 8 else nat.window_bias_image(table[index].reshape(ws * ws, ws * ws, heads).permute(2, 0, 1))
        name = NAMES[ws > 8]
        ab_row(f"window {ws:2d} grid {grid:2d} heads {heads:2d} ld_qkv {ld_qkv:4d} ld_out {ld:4d} shift {shift}",
               lambda L: getattr(L, name)(P(qkv), P(bias), B, grid, grid, heads, c, ws, shift, ld_qkv, ld, scale, P(out), st),
               parent, args.iters, args.runs)
        del qkv, out

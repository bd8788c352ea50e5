"""Swin Transformer teacher: the hierarchical ViT behind the ``layers`` container and the ``nhwc`` feature map the
reference's probe understands (``src/models/teacher.py:42-110``; it takes any timm model and only ever calls
``forward_features`` on a non-token teacher, ``teacher.py:184-191``).

timm is not available offline, so the trunk is defined here from the published architecture (Liu et al. 2021) with the
parameter names of timm >= 0.9 (stated assumption; the architecture itself is pinned by
``tests/_swin_ref.py``):

* ``patch_embed.proj`` Conv2d 4x4 stride 4 + bias, ``patch_embed.norm`` LayerNorm(C0); activations are NHWC from here
* ``layers.{i}.downsample``: identity for i = 0, else patch merging AT THE START of the stage: the 2x2 neighbours
  concatenated in the order (2r, 2c), (2r+1, 2c), (2r, 2c+1), (2r+1, 2c+1), ``norm`` LayerNorm(4C), ``reduction``
  Linear(4C -> 2C, no bias)
* ``layers.{i}.blocks.{j}``: ``norm1``, ``attn.qkv`` (C -> 3C), ``attn.relative_position_bias_table``
  [(2 ws - 1)^2, heads], ``attn.proj``, ``norm2``, ``mlp.fc1``, exact GELU, ``mlp.fc2``; window attention over ws x ws
  windows, block j shifted by ws // 2 when j is odd; a stage whose grid is not larger than the window uses shift 0
* ``attn.relative_position_index`` [ws^2, ws^2] is a non-persistent buffer (as in timm >= 0.9): a state dict does not
  carry it, and the ``relative_position_index`` / ``attn_mask`` entries of older checkpoints are dropped on load.  The
  older layout with ``layers.{i}.downsample`` at the END of stage i (recognised by ``layers.0.downsample.reduction.weight``)
  is remapped to ``layers.{i+1}.downsample``.
* final ``norm`` LayerNorm(C_last) inside ``forward_features`` -> ``[B, H/32, W/32, C_last]`` (NHWC); LayerNorm eps 1e-5

Two forwards of the same parameters, under the protocol and with the image helpers of ``models/fused_trunk.py``:

* plain PyTorch: the CPU path, and on the device the path of whatever the kernels refuse -- reported through
  ``library_fallback``.  Its windows are a gather by the token index of every (window, slot); the mask is built from the
  labels of the slots' rolled coordinates;
* the fused inference path of a frozen bf16 model on the device (``prepare_fused`` once after the weights are loaded,
  and after ``probe_model``, whose hook needs the stage modules' forward): activations are rows ``[B H W, ld]`` (96
  channels in rows of 128, pad columns zero), every linear layer is ``basd_gemm_bf16`` (GELU in fc1's epilogue, the qkv
  width padded to one the GEMM tiles), window attention and patch merging + LayerNorm are ``csrc/swin.hip``, the other
  LayerNorms the existing kernels.  It enqueues no library GEMM, no convolution and no SDPA.  Windows up to 8 take
  ``basd_window_attention_fwd_bf16`` with the bias expanded to a [heads, 64, 64] image; windows 9 .. 16 (window 12 of
  the 384 px checkpoints) take ``basd_window_attention_fwd_wide_bf16`` (``csrc/swin_wide.hip``) with the fp32 bias
  table itself.  A window above 16 is refused.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..losses._ops import get_ops
from .fused_trunk import FusedTrunk, centre_tap_identity, norm_params, padded_image, patch_image, row_width

HEAD_DIM = 32
MASK_VALUE = -100.0
WINDOW_TILE = 8            # the largest window of basd_window_attention_fwd_bf16; 9 .. 16 is the wide entry's


def relative_position_index(ws: int) -> torch.Tensor:
    """[ws^2, ws^2] index into the bias table for (query slot, key slot)"""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)    # [2, N]
    rel = coords[:, :, None] - coords[:, None, :] + (ws - 1)                                              # [2, N, N]
    return rel[0] * (2 * ws - 1) + rel[1]


def window_tokens(h: int, w: int, ws: int, shift: int):
    """-> (token [nW, N], label [nW, N]): slot iy ws + ix of window (wy, wx) holds token
    ((wy ws + iy + shift) mod h) w + (wx ws + ix + shift) mod w -- the roll by -shift and the partition in one index --
    and carries the mask label of its rolled coordinate (all zero without a shift)."""
    ry = (torch.arange(h // ws)[:, None] * ws + torch.arange(ws)[None, :]).reshape(h // ws, 1, ws, 1)
    rx = (torch.arange(w // ws)[:, None] * ws + torch.arange(ws)[None, :]).reshape(1, w // ws, 1, ws)
    token = ((ry + shift) % h) * w + (rx + shift) % w
    if shift > 0:
        label = 3 * ((ry >= h - ws).long() + (ry >= h - shift).long()) + (rx >= w - ws).long() + (rx >= w - shift).long()
    else:
        label = torch.zeros_like(token)
    n = ws * ws
    return token.reshape(-1, n), label.expand_as(token).reshape(-1, n)


def _ln(norm: nn.LayerNorm, x):
    return F.layer_norm(x.float(), norm.normalized_shape, norm.weight, norm.bias, norm.eps).to(x.dtype)


class WindowAttention(nn.Module):
    def __init__(self, dim: int, num_heads: int, window_size: int):
        super().__init__()
        self.num_heads, self.window_size = num_heads, window_size
        self.scale = (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", relative_position_index(window_size), persistent=False)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def bias(self) -> torch.Tensor:
        """[heads, N, N] for (query slot, key slot)"""
        n = self.window_size ** 2
        return self.relative_position_bias_table[self.relative_position_index.reshape(-1)].reshape(n, n, -1).permute(2, 0, 1)

    def forward(self, x, mask=None):
        """x [B, nW, N, C], mask [nW, N, N] | None"""
        b, nw, n, c = x.shape
        qkv = self.qkv(x).reshape(b, nw, n, 3, self.num_heads, c // self.num_heads).permute(3, 0, 1, 4, 2, 5)
        attn = (qkv[0] * self.scale) @ qkv[1].transpose(-1, -2) + self.bias().to(x.dtype)                  # [B, nW, h, N, N]
        if mask is not None:
            attn = attn + mask[None, :, None].to(x.dtype)
        out = attn.softmax(dim=-1) @ qkv[2]
        return self.proj(out.transpose(2, 3).reshape(b, nw, n, c))


class _Mlp(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


def _stage_window(h: int, w: int, ws: int, shift: int):
    """window and shift a block uses on an h x w grid: a grid not larger than the window is one unshifted window"""
    if min(h, w) <= ws:
        if h != w or h != ws:
            raise ValueError(f"Swin: a {h}x{w} grid is smaller than the {ws}x{ws} window its bias table was built for")
        return ws, 0
    if h % ws or w % ws:
        raise ValueError(f"Swin: the {h}x{w} grid is not a multiple of the window {ws}")
    return ws, shift


class SwinBlock(nn.Module):
    def __init__(self, dim: int, num_heads: int, window_size: int, shift: int):
        super().__init__()
        self.window_size, self.shift = window_size, shift
        self.norm1 = nn.LayerNorm(dim, eps=1e-5)
        self.attn = WindowAttention(dim, num_heads, window_size)
        self.norm2 = nn.LayerNorm(dim, eps=1e-5)
        self.mlp = _Mlp(dim)

    def attend(self, y, h: int, w: int):
        """the attention branch on normalised rows y [B, h w, C] -> [B, h w, C]: gather the windows, attend, scatter"""
        ws, shift = _stage_window(h, w, self.window_size, self.shift)
        token, label = window_tokens(h, w, ws, shift)
        token = token.to(y.device)
        mask = None
        if shift > 0:
            mask = (label[:, :, None] != label[:, None, :]).to(y.device, torch.float32) * MASK_VALUE
        out = self.attn(y[:, token], mask)                                      # [B, nW, N, C]
        return torch.empty_like(y).index_copy_(1, token.reshape(-1), out.reshape(y.shape))

    def forward(self, x):
        b, h, w, c = x.shape
        rows = x.reshape(b, h * w, c)
        rows = rows + self.attend(_ln(self.norm1, rows), h, w)
        rows = rows + self.mlp(_ln(self.norm2, rows))
        return rows.reshape(b, h, w, c)


class PatchMerging(nn.Module):
    def __init__(self, dim: int, out_dim: int):
        super().__init__()
        self.norm = nn.LayerNorm(4 * dim, eps=1e-5)
        self.reduction = nn.Linear(4 * dim, out_dim, bias=False)

    def forward(self, x):
        b, h, w, c = x.shape
        x = x.reshape(b, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 4, 2, 5).flatten(3)   # (column parity, row parity, c)
        return self.reduction(_ln(self.norm, x))


class SwinStage(nn.Module):
    def __init__(self, in_dim: int, dim: int, depth: int, num_heads: int, window_size: int, first: bool):
        super().__init__()
        self.downsample = nn.Identity() if first else PatchMerging(in_dim, dim)
        self.blocks = nn.Sequential(*[SwinBlock(dim, num_heads, window_size, 0 if j % 2 == 0 else window_size // 2)
                                      for j in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class _PatchEmbed(nn.Module):
    def __init__(self, in_chans: int, dim: int):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, 4, stride=4)
        self.norm = nn.LayerNorm(dim, eps=1e-5)

    def forward(self, x):
        return _ln(self.norm, self.proj(x).permute(0, 2, 3, 1))                 # NHWC


class SwinTransformer(FusedTrunk, nn.Module):
    _fallback_name = "swin trunk"

    def __init__(self, depths=(2, 2, 6, 2), dims=(96, 192, 384, 768), heads=(3, 6, 12, 24), window_size: int = 7,
                 num_classes: int = 0, in_chans: int = 3):
        super().__init__()
        self.depths, self.dims, self.heads, self.window_size = tuple(depths), tuple(dims), tuple(heads), window_size
        self.patch_embed = _PatchEmbed(in_chans, dims[0])
        self.layers = nn.Sequential(*[SwinStage(dims[max(i - 1, 0)], dims[i], depths[i], heads[i], window_size, i == 0)
                                      for i in range(len(dims))])
        self.norm = nn.LayerNorm(dims[-1], eps=1e-5)
        self.num_features = self.embed_dim = dims[-1]
        self.head = nn.Linear(dims[-1], num_classes) if num_classes > 0 else nn.Identity()
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    # ------------------------------------------------------------------------------------------------- state dicts
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # runs before the children load: older timm checkpoints carry index / mask buffers and keep the patch merging
        # at the end of stage i
        for key in [k for k in state_dict if k.startswith(prefix) and
                    (k.endswith("attn_mask") or k.endswith("relative_position_index"))]:
            del state_dict[key]
        rows = (2 * self.window_size - 1) ** 2
        for key, table in state_dict.items():       # tables are not resampled: a checkpoint of another window is refused
            if key.startswith(prefix) and key.endswith("relative_position_bias_table") and table.shape[0] != rows:
                raise ValueError(f"Swin: {key} has {table.shape[0]} rows, window {self.window_size} needs "
                                 f"(2 ws - 1)^2 = {rows}; bias tables of another window size are not resampled")
        if prefix + "layers.0.downsample.reduction.weight" in state_dict:
            head = prefix + "layers."
            moved = {}
            for key in [k for k in state_dict if k.startswith(head) and ".downsample." in k]:
                stage, rest = key[len(head):].split(".", 1)
                moved[f"{head}{int(stage) + 1}.{rest}"] = state_dict.pop(key)
            state_dict.update(moved)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ------------------------------------------------------------------------------------------------- plain PyTorch
    def _forward_plain(self, x):
        return _ln(self.norm, self.layers(self.patch_embed(x)))

    # ------------------------------------------------------------------------------------------------- fused path
    def _qkv_width(self, c: int, ld: int):
        """the narrowest width >= 3 c the GEMM takes as N on rows of ld (288 -> 384), or None"""
        ops = get_ops()
        return next((n for n in range((3 * c + 127) // 128 * 128, 3 * c + 513, 128) if ops.gemm_supported(n, ld)), None)

    def _attend_entry(self) -> str:
        """the entry every block takes (one window per model, ``_stage_window`` never changes it): ``window_attention``
        with a [heads, 64, 64] bias image up to window 8, ``window_attention_wide`` with the fp32 bias table above"""
        return "window_attention_wide" if self.window_size > WINDOW_TILE else "window_attention"

    def fused_refusal(self) -> str | None:
        """Why the kernels do not take this architecture (None: they do)."""
        ops = get_ops()
        if not hasattr(ops, "window_attention"):
            return "the kernel provider has no Swin trunk entries"
        if self.patch_embed.proj.weight.shape[1] != 3:
            return f"the patch embedding takes 3 input channels (got {self.patch_embed.proj.weight.shape[1]})"
        ws = self.window_size                     # the window every block uses on any grid (``_stage_window``)
        entry = self._attend_entry()
        if not hasattr(ops, entry):
            return f"stage 0: window {ws} needs the wide window attention entry, which the kernel provider does not have"
        supported = getattr(ops, entry + "_supported")
        for i, (c, nh) in enumerate(zip(self.dims, self.heads)):
            ld = row_width(c)
            nq = self._qkv_width(c, ld)
            if c != HEAD_DIM * nh:
                return f"stage {i}: width {c} with {nh} heads is not head dim {HEAD_DIM}"
            if nq is None or not supported(ws, ws, ws, ws // 2, nh, c, nq, ld):
                return f"stage {i}: window {ws} / width {c} (rows of {ld}) is not tiled by the window attention kernel"
            if not (ops.gemm_supported(ld, ld) and ops.gemm_supported(4 * c, ld) and ops.gemm_supported(ld, 4 * c)
                    and (ops.layernorm_supported(c) if ld == c else ops.dwconv7_ln_supported(c, ld, ld))):
                return f"stage {i}: width {c} (rows of {ld}, hidden {4 * c}) is not tiled by the GEMM / LayerNorm kernels"
            if i > 0:
                c_in = self.dims[i - 1]
                if not (c == 2 * c_in and ops.patch_merge_ln_supported(c_in, row_width(c_in))
                        and ops.gemm_supported(ld, 4 * c_in)):
                    return f"stage {i}: merging {c_in} -> {c} is not tiled by the patch-merge kernel / the GEMM"
        if not ops.gemm_supported(row_width(self.dims[0]), 64):
            return f"the patch embedding to rows of {row_width(self.dims[0])} is not tiled by the GEMM"
        return None

    def _build_fused(self):
        """The weight images of ``prepare_fused``: zero-padded GEMM images, the patch embedding in the patch order of
        ``basd_patchify_bf16`` (48 columns in rows of 64), fp32 norm parameters, and per block the relative-position
        bias: expanded from the table into the fp32 [heads, 64, 64] image of ``basd_window_attention_fwd_bf16`` for
        windows up to 8, the fp32 table itself for ``basd_window_attention_fwd_wide_bf16`` (an expanded image of a
        window-12 model would be [heads, 144, 144] per block)."""
        ops = get_ops()
        entry = self._attend_entry()
        proj = self.patch_embed.proj
        lds = [row_width(c) for c in self.dims]

        def linear(m, n_ld, k_ld):
            return padded_image(m.weight, m.bias, n_ld, k_ld)

        fused = {"lds": lds, "stages": [], "attend": entry,
                 "ident": {c: centre_tap_identity(c, proj.weight.device) for c, ld in zip(self.dims, lds) if ld != c},
                 "embed": padded_image(patch_image(proj.weight), proj.bias, lds[0], 64),
                 "embed_norm": norm_params(self.patch_embed.norm), "norm": norm_params(self.norm)}
        for i, stage in enumerate(self.layers):
            c, ld = self.dims[i], lds[i]
            rec = {"merge": None, "blocks": []}
            if i > 0:
                down = stage.downsample
                rec["merge"] = norm_params(down.norm) + linear(down.reduction, ld, 4 * self.dims[i - 1])[:1]
            nq = self._qkv_width(c, ld)
            for blk in stage.blocks:
                rec["blocks"].append({
                    "norm1": norm_params(blk.norm1), "qkv": linear(blk.attn.qkv, nq, ld),
                    "bias": (ops.window_bias_image(blk.attn.bias()) if entry == "window_attention"
                             else blk.attn.relative_position_bias_table.to(torch.float32).contiguous()),
                    "scale": blk.attn.scale, "shift": blk.shift, "proj": linear(blk.attn.proj, ld, ld),
                    "norm2": norm_params(blk.norm2), "fc1": linear(blk.mlp.fc1, 4 * c, ld), "fc2": linear(blk.mlp.fc2, ld, 4 * c)})
            fused["stages"].append(rec)
        return fused

    def _forward_fused(self, x):
        """x [B, 3, H, W] bf16 (any strides) -> [B, H/32, W/32, C_last] bf16, a view of the last rows"""
        ops, fz = get_ops(), self._fused
        lds, ws, attend = fz["lds"], self.window_size, getattr(ops, fz["attend"])
        b, _, h, w = x.shape
        h, w = h // 4, w // 4
        t = ops.gemm_bf16(ops.patchify(x, 4, 64), *fz["embed"])                          # [B h w, ld0]
        t = self._norm_rows(ops, t, self.dims[0], *fz["embed_norm"])
        for i, rec in enumerate(fz["stages"]):
            c, ld, nh = self.dims[i], lds[i], self.heads[i]
            if rec["merge"] is not None:
                gamma, beta, eps, w_red = rec["merge"]
                y = ops.patch_merge_ln(t.view(b, h, w, lds[i - 1]), self.dims[i - 1], gamma, beta, eps)
                h, w = h // 2, w // 2
                t = ops.gemm_bf16(y.view(b * h * w, 4 * self.dims[i - 1]), w_red, None)   # [B h w, ld]
            for blk in rec["blocks"]:
                win, shift = _stage_window(h, w, ws, blk["shift"])
                y = self._norm_rows(ops, t, c, *blk["norm1"])
                qkv = ops.gemm_bf16(y, *blk["qkv"])
                a = attend(qkv.view(b, h, w, qkv.shape[1]), blk["bias"], win, shift, nh, blk["scale"], ld_out=ld)
                p = ops.gemm_bf16(a.view(b * h * w, ld), *blk["proj"])
                if ld == c:
                    t, y = ops.add_layernorm_fwd(p, t, *blk["norm2"])                    # t <- t + p, y = LayerNorm(t)
                else:
                    t.add_(p)
                    y = self._norm_rows(ops, t, c, *blk["norm2"])
                hid = ops.gemm_bf16(y, *blk["fc1"], gelu=True)
                t.add_(ops.gemm_bf16(hid, *blk["fc2"]))                                  # residual: one in-place add
        t = self._norm_rows(ops, t, self.dims[-1], *fz["norm"])
        return t.view(b, h, w, lds[-1])[..., :self.dims[-1]]

    def _grid_ok(self, h: int, w: int) -> bool:
        if h % 32 or w % 32 or h < 32 or w < 32:
            return False
        for i in range(len(self.dims)):
            gh, gw = h // (4 << i), w // (4 << i)
            try:
                _stage_window(gh, gw, self.window_size, 0)
            except ValueError:
                return False
        return True

    def check_image_size(self, img_size: int) -> None:
        """``load_teacher`` calls this before the first forward: a window that does not tile the token grids of the
        image size (window 12 at 224 px: grids 56, 28, 14, 7) is an error that names both"""
        grids = [img_size // (4 << i) for i in range(len(self.dims))]
        if not self._grid_ok(img_size, img_size):
            raise ValueError(f"Swin: image size {img_size} gives the token grids {grids}, which window "
                             f"{self.window_size} does not tile (every grid is a multiple of the window, or one window); "
                             f"window {self.window_size} takes image sizes that are multiples of {32 * self.window_size}")

    def _takes_fused(self, x) -> bool:
        return (self._fused is not None and not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 4
                and x.shape[1] == 3 and self.patch_embed.proj.weight.dtype == torch.bfloat16
                and self._grid_ok(x.shape[2], x.shape[3]))

    def forward(self, x):
        return self.head(self.forward_features(x).mean(dim=(1, 2)))


SWIN_PRESETS = {
    "swin_tiny_patch4_window7_224": lambda: SwinTransformer((2, 2, 6, 2), (96, 192, 384, 768), (3, 6, 12, 24)),
    "swin_small_patch4_window7_224": lambda: SwinTransformer((2, 2, 18, 2), (96, 192, 384, 768), (3, 6, 12, 24)),
    "swin_base_patch4_window7_224": lambda: SwinTransformer((2, 2, 18, 2), (128, 256, 512, 1024), (4, 8, 16, 32)),
    # Swin-L and the window-12 checkpoints of 384 px: depths, widths and heads written from memory of timm's model
    # table, without timm at hand (as the presets above; DESIGN sections 19 and 26)
    "swin_large_patch4_window7_224": lambda: SwinTransformer((2, 2, 18, 2), (192, 384, 768, 1536), (6, 12, 24, 48)),
    "swin_base_patch4_window12_384": lambda: SwinTransformer((2, 2, 18, 2), (128, 256, 512, 1024), (4, 8, 16, 32),
                                                             window_size=12),
    "swin_large_patch4_window12_384": lambda: SwinTransformer((2, 2, 18, 2), (192, 384, 768, 1536), (6, 12, 24, 48),
                                                              window_size=12),
}

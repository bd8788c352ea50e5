"""What the fused inference trunks of the one-feature-map teachers share (``ResNet`` in ``models/cnn.py``,
``ConvNeXtV2`` in ``models/convnext.py``, ``SwinTransformer`` in ``models/swin.py``): the state protocol of the weight
images and the layouts the kernels read them in.

A trunk has two forwards of the same parameters: plain PyTorch, and ``_forward_fused`` on the kernels of ``get_ops()``
with activations as rows ``[B H W, ld]``.  The fused one reads ``self._fused``, the weight images ``prepare_fused()``
builds once from a frozen model; any ``.to()`` or cast drops them.  A trunk inherits ``FusedTrunk`` in front of
``nn.Module`` and keeps what is its own: ``fused_refusal()``, ``_takes_fused(x)``, ``_build_fused()``,
``_forward_fused(x)``, ``_forward_plain(x)`` and the name it reports under.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ..losses._ops import get_ops, library_fallback


def row_width(c: int) -> int:
    """Row stride of a C-channel activation: C itself when the GEMM takes it as N and as K, else the next multiple of 128."""
    ops = get_ops()
    return c if ops.gemm_supported(c, c) else (c + 127) // 128 * 128


def padded_image(w2d, bias, n_ld: int, k_ld: int):
    """[N, K] weight (+ [N] bias | None) -> the bf16 GEMM image ([n_ld, k_ld], [n_ld] | None): zero rows and zero bias
    for the padded output channels, zero columns for the padded input channels; the one rounding to bf16 is here"""
    n, k = w2d.shape
    w = torch.zeros(n_ld, k_ld, dtype=torch.bfloat16, device=w2d.device)
    w[:n, :k] = w2d.to(torch.bfloat16)
    b = None
    if bias is not None:
        b = torch.zeros(n_ld, dtype=torch.bfloat16, device=w2d.device)
        b[:n] = bias.to(torch.bfloat16)
    return w, b


def patch_image(weight, c_in_ld: int | None = None):
    """[C_out, C_in, p, p] convolution weight -> [C_out, p p c_in_ld] with column (i p + j) c_in_ld + c, the order
    ``basd_patchify_bf16`` writes a patch in (and the tap-major order of the 3 x 3 and stem kernels); zero columns for
    input channels c_in_ld pads.  The dtype is kept: ``padded_image`` rounds."""
    c_out, c_in, p, _ = weight.shape
    c_in_ld = c_in if c_in_ld is None else c_in_ld
    return F.pad(weight.permute(0, 2, 3, 1), (0, c_in_ld - c_in)).reshape(c_out, p * p * c_in_ld)


def norm_params(m):
    """(gamma fp32, beta fp32, eps) of a LayerNorm, as the norm kernels take them"""
    return m.weight.to(torch.float32).contiguous(), m.bias.to(torch.float32).contiguous(), m.eps


def centre_tap_identity(c: int, device):
    """LayerNorm over C columns of rows of stride ld > C through basd_dwconv7_ln_bf16 at H = W = 1: the one-hot centre
    tap and a zero bias make the convolution an exact copy"""
    w49 = torch.zeros(49, c, dtype=torch.bfloat16, device=device)
    w49[24] = 1.0
    return w49, torch.zeros(c, dtype=torch.float32, device=device)


class FusedTrunk:
    """Mixin in front of ``nn.Module``; it adds no parameter, buffer or submodule."""

    _fused = None                      # the weight images of ``_build_fused()``, or None: not prepared
    _fallback_name = "fused trunk"     # what a forward that cannot take the fused path is reported as

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float() move or recast the parameters: the weight images no longer belong to them
        self._fused = None
        return super()._apply(fn, *args, **kwargs)

    @torch.no_grad()
    def prepare_fused(self) -> bool:
        """Build the weight images of the fused path once (frozen teacher: no refresh); False, and no images, for an
        architecture the kernels refuse or a model with gradients."""
        self._fused = None
        if self.fused_refusal() is not None or any(p.requires_grad for p in self.parameters()):
            return False
        self._fused = self._build_fused()
        return True

    def _reports(self, x) -> bool:
        """whether a forward of x that does not take the fused path is a library fallback"""
        return get_ops().handles(x)

    def _fallback_detail(self, x) -> str:
        return (f"dtype={x.dtype} size={tuple(x.shape[2:])} grad={torch.is_grad_enabled()} "
                f"prepared={self._fused is not None}")

    def forward_features(self, x):
        if self._reports(x):
            if self._takes_fused(x):
                return self._forward_fused(x)
            library_fallback(self._fallback_name, self.fused_refusal() or self._fallback_detail(x))
        return self._forward_plain(x)

    def _norm_rows(self, ops, x, c, gamma, beta, eps):
        """LayerNorm over the first c columns of x [rows, ld] -> [rows, ld] (pad columns zero); rows wider than c go
        through the ``ident`` table of ``centre_tap_identity`` images, keyed by c"""
        rows, ld = x.shape
        if ld == c:
            return ops.layernorm_fwd(x, gamma, beta, eps)[0]
        w49, zero = self._fused["ident"][c]
        return ops.dwconv7_ln(x.view(rows, 1, 1, ld), w49, zero, gamma, beta, eps).view(rows, ld)

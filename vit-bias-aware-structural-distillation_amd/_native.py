"""ctypes binding of ``libbasd_hip.so`` (C-ABI declared in include/basd_hip.h).

There is NO CPU fallback: if the library is missing or a call fails this
module raises.  torch is used only for device memory and streams.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# BASD_LIB: an alternative build of the same library (A/B timing of kernel variants from scripts/); still no CPU path
LIB_PATH = os.environ.get("BASD_LIB") or os.path.join(_HERE, "libbasd_hip.so")
CSRC = os.path.join(_HERE, "csrc")

DTYPE_F32, DTYPE_BF16, DTYPE_F64 = 0, 1, 2
JACOBI_LDS_BYTES = 163840

EXPORTS = (
    "basd_version", "basd_last_error", "basd_token_gram", "basd_token_gram_bf16x3", "basd_gram_f32_centred", "basd_pchol_f64", "basd_jacobi_svd",
    "basd_mp_rank", "basd_flag_if_exceeds_f64", "basd_angle_weights", "basd_ce_uwso",
    "basd_procrustes_workspace_bytes", "basd_procrustes_fwd", "basd_procrustes_bwd_side",
    "basd_procrustes_bwd_workspace_bytes", "basd_procrustes_bwd", "basd_angle_weights_bwd_workspace_bytes",
    "basd_angle_weights_bwd", "basd_mix_tokens", "basd_procrustes_prep", "basd_mix_grad_dots",
    "basd_sf_adamw_step", "basd_lerp", "basd_transpose_bf16_table", "basd_bgemm_f64", "basd_trinv_f64", "basd_bgemm_f64_masked", "basd_trinv_f64_masked", "basd_pchol_f64_masked", "basd_wgrad_bf16", "basd_wgrad_workspace_bytes", "basd_wgrad_bf16_ws", "basd_gemm_bf16",
    "basd_gemm_bf16_gelu_fwd", "basd_gemm_bf16_gelu_bwd", "basd_gemm_bf16x3_f32", "basd_layernorm_fwd_bf16", "basd_layernorm_bwd_bf16",
    "basd_cls_importance_bf16", "basd_add_layernorm_fwd_bf16", "basd_procrustes_bwd_rows", "basd_attention_fwd_bf16", "basd_attention_fwd_qmean_bf16", "basd_attention_bwd_bf16",
    "basd_split_bf16x2_table", "basd_split_patches_bf16x2", "basd_gemm_f32x3", "basd_attention_fwd_f32x3",
    "basd_add_layernorm_fwd_f32", "basd_selector_frames_workspace_bytes", "basd_selector_frames",
    "basd_selector_weights_workspace_bytes", "basd_selector_weights", "basd_attention_fwd_long_bf16",
    "basd_attention_bwd_long_workspace_bytes", "basd_attention_bwd_long_bf16", "basd_attention_fwd_f32x3_long",
    "basd_dwconv7_ln_bf16", "basd_grn_workspace_bytes", "basd_grn_bf16", "basd_patchify_bf16",
    "basd_resample_u8", "basd_ta_normalize_u8", "basd_cls_tally", "basd_resample_u8_packed",
    "basd_mixup_cutmix", "basd_selector_token_grad_workspace_bytes", "basd_selector_token_grad",
    "basd_tap_grad_scatter", "basd_resample_tokens", "basd_resample_tokens_adjoint", "basd_procrustes_importance_bwd",
    "basd_conv3x3_bf16", "basd_conv7x7s2_relu_bf16", "basd_maxpool3x3s2_bf16", "basd_add_relu_bf16",
    "basd_sym_tridiag_f64_workspace_bytes", "basd_sym_tridiag_f64", "basd_tridiag_mp_rank",
    "basd_window_attention_fwd_bf16", "basd_patch_merge_ln_bf16", "basd_gemm_bf16_act", "basd_vit_embed_bf16",
    "basd_attention_fwd_relbias_bf16", "basd_gemm_bf16_swiglu", "basd_vit_embed_reg_bf16",
    "basd_attention_fwd_rope_bf16", "basd_attention_fwd_long_rope_bf16", "basd_attention_fwd_long_relbias_bf16",
    "basd_window_attention_fwd_wide_bf16",
)


_P, _I, _I64, _F, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
# argument types of every export, in the order of include/basd_hip.h
_SIGNATURES = {
    "basd_version": (),
    "basd_last_error": (),
    "basd_token_gram": (_P, _I, _I64, _I, _I, _I64, _P, _I, _P, _P, _P),
    "basd_token_gram_bf16x3": (_P, _I64, _I, _I, _I64, _P, _I, _P, _P, _P),
    "basd_gram_f32_centred": (_P, _I64, _I, _P, _P, _P),
    "basd_pchol_f64": (_P, _I, _I, _D, _P, _P, _I, _P, _P, _P, _P),
    "basd_pchol_f64_masked": (_P, _I, _I, _D, _P, _P, _I, _P, _P, _P, _P, _P),
    "basd_trinv_f64": (_P, _P, _P, _I, _I, _P, _P),
    "basd_trinv_f64_masked": (_P, _P, _P, _I, _I, _P, _P, _P),
    "basd_jacobi_svd": (_P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _I, _P, _P),
    "basd_mp_rank": (_P, _I, _I, _I64, _I, _I, _P, _P, _P),
    "basd_flag_if_exceeds_f64": (_P, _I64, _D, _I, _P, _P),
    "basd_angle_weights": (_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P),
    "basd_mix_tokens": (_P, _I, _I, _I, _P, _I64, _I64, _I64, _P, _P),
    "basd_procrustes_prep": (_P, _I, _I64, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P),
    "basd_mix_grad_dots": (_P, _I, _I, _I, _P, _I64, _I64, _I64, _P, _P),
    "basd_procrustes_workspace_bytes": (_I, _I, _I, _I),
    "basd_procrustes_fwd": (_P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P, _I64, _P),
    "basd_procrustes_bwd_side": (_P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P),
    "basd_procrustes_bwd_workspace_bytes": (_I, _I),
    "basd_angle_weights_bwd_workspace_bytes": (_I, _I, _I),
    "basd_angle_weights_bwd": (_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I64, _P),
    "basd_selector_frames_workspace_bytes": (_I, _I),
    "basd_selector_frames": (_P, _P, _I, _I64, _I, _I, _P, _P, _P, _P, _P, _P, _I64, _P),
    "basd_selector_weights_workspace_bytes": (_I, _I, _I),
    "basd_selector_weights": (_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I64, _P),
    "basd_procrustes_bwd": (_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _I64, _P),
    "basd_ce_uwso": (_P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P),
    "basd_transpose_bf16_table": (_P, _P, _P, _I, _P),
    "basd_bgemm_f64": (_P, _I, _I64, _I, _I, _P, _I, _I64, _I, _I, _P, _I, _I64, _I, _I, _I, _I, _I, _I, _P),
    "basd_bgemm_f64_masked": (_P, _I, _I64, _I, _I, _P, _I, _I64, _I, _I, _P, _I, _I64, _I, _I, _I, _I, _I, _I, _P, _P),
    "basd_wgrad_bf16": (_P, _P, _I64, _I, _I, _P, _P, _P),
    "basd_wgrad_workspace_bytes": (_I64, _I, _I),
    "basd_wgrad_bf16_ws": (_P, _P, _I64, _I, _I, _P, _P, _P, _I64, _P),
    "basd_gemm_bf16": (_P, _P, _P, _P, _I64, _I, _I, _I, _I, _P),
    "basd_gemm_bf16_act": (_P, _P, _P, _P, _I64, _I, _I, _I, _I, _P),
    "basd_gemm_bf16_swiglu": (_P, _P, _P, _P, _I64, _I, _I, _I, _P),
    "basd_gemm_bf16_gelu_fwd": (_P, _P, _P, _P, _P, _I64, _I, _I, _I, _P),
    "basd_gemm_bf16x3_f32": (_P, _P, _P, _I64, _I, _I, _P),
    "basd_gemm_bf16_gelu_bwd": (_P, _P, _P, _P, _I64, _I, _I, _I, _P),
    "basd_layernorm_fwd_bf16": (_P, _P, _P, _I64, _I, _F, _P, _P, _P, _P),
    "basd_add_layernorm_fwd_bf16": (_P, _P, _P, _P, _I64, _I, _F, _P, _P, _P, _P, _P, _I, _P),
    "basd_vit_embed_bf16": (_P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P),
    "basd_vit_embed_reg_bf16": (_P, _P, _P, _I, _P, _P, _P, _F, _I, _I, _I, _P, _P),
    "basd_layernorm_bwd_bf16": (_P, _P, _P, _P, _P, _I64, _I, _P, _P, _P, _P, _P, _P, _I, _P),
    "basd_procrustes_bwd_rows": (_P, _P, _P, _P, _I64, _I, _I, _P, _I, _P, _P),
    "basd_cls_importance_bf16": (_P, _I, _I, _I, _I, _F, _P, _P),
    "basd_attention_fwd_bf16": (_P, _I, _I, _I, _I, _F, _P, _P, _P, _P),
    "basd_attention_fwd_qmean_bf16": (_P, _I, _I, _I, _I, _F, _P, _P, _P),
    "basd_attention_fwd_relbias_bf16": (_P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P),
    "basd_attention_fwd_rope_bf16": (_P, _P, _I, _I, _I, _I, _F, _P, _P, _P),
    "basd_attention_fwd_long_rope_bf16": (_P, _P, _I, _I, _I, _I, _F, _P, _P, _P),
    "basd_attention_fwd_long_relbias_bf16": (_P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P),
    "basd_attention_bwd_bf16": (_P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P),
    "basd_attention_fwd_long_bf16": (_P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P),
    "basd_attention_bwd_long_workspace_bytes": (_I, _I, _I, _I),
    "basd_attention_bwd_long_bf16": (_P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _I64, _P),
    "basd_sf_adamw_step": (_P, _P, _P, _P, _I64, _D, _D, _D, _D, _D, _D, _D, _P),
    "basd_lerp": (_P, _P, _I64, _F, _P),
    "basd_split_bf16x2_table": (_P, _I, _P),
    "basd_split_patches_bf16x2": (_P, _I, _I, _I, _I, _I, _I, _P, _P),
    "basd_gemm_f32x3": (_P, _P, _P, _P, _I64, _I, _I, _I, _P),
    "basd_attention_fwd_f32x3": (_P, _I, _I, _I, _I, _F, _P, _P),
    "basd_attention_fwd_f32x3_long": (_P, _I, _I, _I, _I, _F, _P, _P),
    "basd_add_layernorm_fwd_f32": (_P, _P, _P, _P, _P, _I64, _I, _F, _P, _P, _P, _P),
    "basd_dwconv7_ln_bf16": (_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P),
    "basd_grn_workspace_bytes": (_I, _I, _I),
    "basd_grn_bf16": (_P, _P, _P, _I, _I, _I, _F, _P, _I64, _P),
    "basd_patchify_bf16": (_P, _I, _I, _I, _I, _I64, _I64, _I64, _I64, _I, _I, _P, _P),
    "basd_resample_u8": (_P, _P, _I, _I, _I, _I, _P, _P),
    "basd_resample_u8_packed": (_P, _I64, _P, _P, _I, _I, _P, _P),
    "basd_ta_normalize_u8": (_P, _P, _P, _I, _I, _F, _F, _F, _F, _F, _F, _P, _P),
    "basd_cls_tally": (_P, _I, _I64, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P),
    "basd_mixup_cutmix": (_P, _I, _I, _I, _I, _I, _P, _I, _I, _F, _I, _I, _I, _I, _P, _P, _P),
    "basd_selector_token_grad_workspace_bytes": (_I, _I),
    "basd_selector_token_grad": (_P, _I, _I, _I, _I, _I64, _P, _P, _P, _I64, _P),
    "basd_tap_grad_scatter": (_P, _P, _P, _I, _I, _I, _I, _P, _P),
    "basd_resample_tokens": (_P, _I, _I, _I, _I, _I, _P, _P),
    "basd_resample_tokens_adjoint": (_P, _I, _I, _I, _I, _I, _P, _P),
    "basd_procrustes_importance_bwd": (_P, _P, _P, _I, _I, _I, _P, _P),
    "basd_conv3x3_bf16": (_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P),
    "basd_conv7x7s2_relu_bf16": (_P, _P, _P, _I, _I, _I, _I64, _I64, _I64, _I64, _I, _I, _P, _P),
    "basd_maxpool3x3s2_bf16": (_P, _I, _I, _I, _I, _I, _I, _P, _P),
    "basd_add_relu_bf16": (_P, _P, _I64, _I, _I, _I, _P),
    "basd_sym_tridiag_f64_workspace_bytes": (_I,),
    "basd_sym_tridiag_f64": (_P, _I, _P, _P, _P, _P),
    "basd_tridiag_mp_rank": (_P, _P, _I, _I64, _I, _I, _P, _P, _P),
    "basd_window_attention_fwd_bf16": (_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P),
    "basd_window_attention_fwd_wide_bf16": (_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P),
    "basd_patch_merge_ln_bf16": (_P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P),
}


class BasdNativeError(RuntimeError):
    pass


class BasdLinAlgError(torch.linalg.LinAlgError):
    """Data-dependent failure of a linear-algebra kernel (non-finite input, Jacobi without convergence, a rank-0
    teacher layer): the counterpart of the ``torch._C._LinAlgError`` the reference's ``torch.linalg`` calls raise."""


STATUS_NONCONVERGED, STATUS_NONFINITE, STATUS_RANK0 = 1, 2, 4
_STATUS_TEXT = {
    STATUS_NONCONVERGED: "a Jacobi SVD used all its sweeps without converging",
    STATUS_NONFINITE: "non-finite values reached a Jacobi SVD / the Marchenko-Pastur rank (NaN or Inf in the tokens)",
    STATUS_RANK0: "a teacher layer has Marchenko-Pastur rank 0 (pure-noise tokens): the reference's weights are NaN here",
}


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into the in-tree shared library."""
    res = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if res.returncode != 0:
        raise BasdNativeError(f"building libbasd_hip.so failed:\n{res.stdout}\n{res.stderr}")
    if verbose:
        print(res.stdout)
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BasdNativeError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the BASD kernels)")
        L = ctypes.CDLL(LIB_PATH)
        for name in EXPORTS:
            if not hasattr(L, name):
                raise BasdNativeError(f"{LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes = list(_SIGNATURES[name])      # explicit: no default int conversion of 64-bit sizes / pointers
            fn.restype = (ctypes.c_char_p if name == "basd_last_error" else
                          ctypes.c_int64 if name.endswith("_workspace_bytes") else ctypes.c_int)
        _lib = L
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().basd_last_error().decode()
        raise BasdNativeError(f"{what} failed with status {rc}: {msg}")


def _ptr(t: torch.Tensor | None) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return DTYPE_F32
    if t.dtype == torch.bfloat16:
        return DTYPE_BF16
    raise BasdNativeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def handles(t: torch.Tensor) -> bool:
    """The kernels of this provider take device tensors only (module code asks before choosing the fused path)."""
    return t.is_cuda


def _need_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise BasdNativeError("BASD kernels need tensors on an MI355X device (no CPU path)")


_STATUS: dict = {}


def status_word(device) -> torch.Tensor:
    """The per-device int32 health word the data-dependent kernels OR their flags into (allocated once; kernels
    captured in a hipGraph keep writing to it)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    buf = _STATUS.get(key)
    if buf is None:
        buf = _STATUS[key] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
    return buf


def raise_for_status(value: int) -> None:
    if value:
        what = "; ".join(text for bit, text in _STATUS_TEXT.items() if value & bit)
        if value >> 8:        # diagnostics of a non-converged Jacobi solve (csrc/jacobi.hip, report_status)
            what += f" [kernel variant {(value >> 8) & 15}, matrix {(value >> 12) & 0xffff}]"
        raise BasdLinAlgError(f"BASD kernels reported status {value & 255}: {what}")


def check_status(device=None) -> None:
    """Read (synchronising) and clear the health word of ``device``; raises BasdLinAlgError if a kernel flagged a
    failure since the last check."""
    buf = status_word(device if device is not None else torch.cuda.current_device())
    value = int(buf.item())
    if value:
        buf.zero_()
    raise_for_status(value)


def jacobi_ld(m_rows: int) -> int:
    """Column stride used for Jacobi inputs (multiple of 4, not of 32)."""
    ld = (m_rows + 3) // 4 * 4
    if ld % 32 == 0:
        ld += 4
    return ld


# --------------------------------------------------------------------------- #
_SPLIT_CACHE: dict = {}


def split_bf16x3(proj: torch.Tensor) -> torch.Tensor:
    """fp32 [d_out, d_in] -> bf16 [3, d_out, d_in] with proj == hi + mid + lo to 2^-24 (cached per buffer)."""
    key = (proj.data_ptr(), proj._version, tuple(proj.shape))
    hit = _SPLIT_CACHE.get(key, (None, None))[0]
    if hit is None:
        p = proj.detach().float()
        hi = p.bfloat16()
        r1 = p - hi.float()
        mid = r1.bfloat16()
        lo = (r1 - mid.float()).bfloat16()
        hit = torch.stack([hi, mid, lo]).contiguous()
        if len(_SPLIT_CACHE) > 16:
            _SPLIT_CACHE.clear()
        _SPLIT_CACHE[key] = (hit, proj)            # holds proj: its address cannot be handed to another tensor meanwhile
    return hit


def split_bf16x3_rows(proj: torch.Tensor) -> torch.Tensor:
    """fp32 [d_out, d_in] -> bf16 [ceil(d_out / 256) * 256, 3 * d_in]: row n = (hi | mid | lo) of proj[n] side by side,
    zero rows behind d_out (operand layout of basd_gemm_bf16x3_f32; cached per buffer)."""
    key = ("rows", proj.data_ptr(), proj._version, tuple(proj.shape))
    hit = _SPLIT_CACHE.get(key, (None, None))[0]
    if hit is None:
        d_out, d_in = proj.shape
        s3 = split_bf16x3(proj)                                                     # [3, d_out, d_in]
        hit = torch.zeros((d_out + 255) // 256 * 256, 3 * d_in, dtype=torch.bfloat16, device=proj.device)
        hit[:d_out] = s3.permute(1, 0, 2).reshape(d_out, 3 * d_in)
        _SPLIT_CACHE[key] = (hit, proj)
    return hit


def gemm_bf16x3_f32_supported(m: int, n: int, k: int) -> bool:
    return m > 7 * 256 and k % 64 == 0 and k >= 128 and n % 8 == 0


def gemm_bf16x3_f32(x: torch.Tensor, proj: torch.Tensor) -> torch.Tensor:
    """x [M, K] bf16, proj [N, K] fp32 -> x proj^T [M, N] fp32: ONE persistent bf16-MFMA GEMM of depth 3 K over the
    (hi | mid | lo) bf16 splits of proj, fp32 accumulation across all three (x is exact in bf16, proj to 2^-24)."""
    _need_cuda(x, proj)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and proj.dim() == 2 and x.shape[1] == proj.shape[1]
    x = x.contiguous()
    m, k = x.shape
    n = proj.shape[0]
    w3 = split_bf16x3_rows(proj.contiguous().float())
    z = torch.empty(m, n, dtype=torch.float32, device=x.device)
    _check(lib().basd_gemm_bf16x3_f32(_ptr(x), _ptr(w3), _ptr(z), ctypes.c_int64(m), n, k, _stream()),
           "basd_gemm_bf16x3_f32")
    return z


def _token_view(x: torch.Tensor):
    """[B, N, D] (possibly a batch-strided view such as out[:, 1:, :]) or [M, D] ->
    (tensor to take the pointer from, rows, d, rows_per_batch, batch_stride) without copying when possible."""
    if x.dim() == 3:
        b, n, d = x.shape
        if x.stride(2) == 1 and x.stride(1) == d and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0:
            return x, b * n, d, n, x.stride(0)
        x = x.contiguous()
        return x, b * n, d, n, n * d
    x = x.contiguous()
    return x, x.shape[0], x.shape[1], x.shape[0], 0


def _mirror_lower(gram: torch.Tensor) -> torch.Tensor:
    """The kernels accumulate the lower 16x16 tiles only (diagonal tiles are complete)."""
    low = torch.tril(gram)
    return low + torch.tril(gram, -1).t()


def _split_rows(m: int) -> int:
    """Number of K-slabs for the split-K Gram of a tall [m, d] matrix (slab rows stay a multiple of 4)."""
    for s in (64, 32, 16, 8, 4, 2):
        if m % (4 * s) == 0 and m // s >= 256:
            return s
    return 1


# BASD_WIDE_GRAM=f64: the split-K fp64-MFMA Gram of rounds 2 - 3 instead of basd_gram_f32_centred (A/B timing)
WIDE_GRAM_FP32 = os.environ.get("BASD_WIDE_GRAM", "f32c") != "f64"


def _token_gram_wide(x: torch.Tensor, proj: torch.Tensor):
    """d_out > 256 (student widths 384 / 768, BASELINE c4 / c5): the fused one-pass kernel keeps a [128, d_out] z tile
    and d_out^2 / 256 fp64 accumulator tiles on chip, which stops at 256 columns.  Here z = X P^T is materialised in
    fp32 and z^T z runs on the fp64 matrix cores as a split-K batched GEMM (basd_bgemm_f64, symmetric tiles only)
    followed by the slab sum.  z = X P^T is an own kernel either way (a library GEMM here would be the only one of the
    teacher branch, i.e. the only reason not to run that branch on its own stream: trainer.py, _ensure_stream_policy):
    bf16 tokens at training sizes take the bf16x3 persistent GEMM (basd_gemm_bf16x3_f32: 24 x 0.1 ms at BASELINE c4;
    the fp64-MFMA batched GEMM at batch 1 needed 2.6 ms per layer there), anything else the fp64-MFMA one."""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.dtype == torch.bfloat16 and gemm_bf16x3_f32_supported(x2.shape[0], proj.shape[0], x2.shape[1]):
        z = gemm_bf16x3_f32(x2, proj)
    else:
        z = bgemm_f64(x2.float().unsqueeze(0), proj.unsqueeze(0), trans_b=True, out_dtype=torch.float32)[0]
    m, d = z.shape
    if WIDE_GRAM_FP32 and d % 16 == 0:
        # round 4: tile-centred Gram on the fp32 matrix cores, fp64 across the 64-row tiles (basd_gram_f32_centred)
        z = z.contiguous()
        gram = torch.zeros(d, d, dtype=torch.float64, device=z.device)
        colsum = torch.zeros(d, dtype=torch.float64, device=z.device)
        _check(lib().basd_gram_f32_centred(_ptr(z), ctypes.c_int64(m), d, _ptr(gram), _ptr(colsum), _stream()),
               "basd_gram_f32_centred")
        return _mirror_lower(gram), colsum
    s = _split_rows(m)
    zs = z.view(s, m // s, d)
    gram = bgemm_f64(zs, zs, trans_a=True, symmetric=True).sum(dim=0)              # [d, d] fp64
    return gram, z.sum(dim=0, dtype=torch.float64)


def token_gram(x: torch.Tensor, proj: torch.Tensor, mirror: bool = True, out=None):
    """x [M, d_in] or [B, N, d_in] view (f32/bf16), proj [d_out, d_in] f32 ->
    gram [d_out, d_out] f64, colsum [d_out] f64.  ``mirror=False`` leaves the strict upper triangle
    unspecified (the kernels fill lower tiles only; ``pchol`` reads nothing else).
    ``out`` = (gram, colsum) ZEROED fp64 buffers to accumulate into (e.g. slices of one per-step allocation: a
    16-layer step otherwise spends 32 launches on zero-fills); requires ``mirror=False``."""
    _need_cuda(x, proj)
    if proj.shape[0] > 256 or proj.shape[0] % 16 or x.shape[-1] % 32:
        g, c = _token_gram_wide(x, proj.contiguous().float())
        if out is not None:
            out[0].copy_(g)
            out[1].copy_(c)
            return out
        return g, c
    x, m, d_in, rpb, bstride = _token_view(x)
    proj = proj.contiguous().float()
    d_out = proj.shape[0]
    if out is not None:
        assert not mirror
        gram, colsum = out
        assert gram.shape == (d_out, d_out) and colsum.shape == (d_out,) and gram.dtype == torch.float64
        assert gram.is_contiguous() and colsum.is_contiguous()
    else:
        gram = torch.zeros(d_out, d_out, dtype=torch.float64, device=x.device)
        colsum = torch.zeros(d_out, dtype=torch.float64, device=x.device)
    i64 = ctypes.c_int64
    if x.dtype == torch.bfloat16 and d_out in (32, 64, 128, 192) and d_in % 32 == 0:
        ps = split_bf16x3(proj)
        _check(lib().basd_token_gram_bf16x3(_ptr(x), i64(m), d_in, rpb, i64(bstride), _ptr(ps), d_out, _ptr(gram),
                                            _ptr(colsum), _stream()), "basd_token_gram_bf16x3")
        return (_mirror_lower(gram) if mirror else gram), colsum
    _check(lib().basd_token_gram(_ptr(x), _dtype_code(x), i64(m), d_in, rpb, i64(bstride), _ptr(proj), d_out,
                                 _ptr(gram), _ptr(colsum), _stream()), "basd_token_gram")
    return (_mirror_lower(gram) if mirror else gram), colsum


def _skip_mask(skip, batch: int):
    """int32 [batch] device mask of the *_masked entries (non-zero = leave the problem's outputs untouched) | None"""
    if skip is None:
        return None
    assert skip.dtype == torch.int32 and skip.numel() == batch and skip.is_contiguous()
    return skip


def pchol(a: torch.Tensor, tol: float = 1e-13, dmax_ref: torch.Tensor | None = None, skip: torch.Tensor | None = None):
    """a [batch, n, n] f64 PSD -> (w0 [batch, n, ld] f32, lwork [batch, n, n] f64, piv, rank).
    ``dmax_ref`` (fp64 [batch], optional): the stop test is ``pivot > tol * dmax_ref[b]`` instead of relative to the
    matrix's own largest diagonal entry (panels of a blocked factorisation).  ``skip`` (int32 [batch] on the device,
    optional): the outputs of problems with a non-zero entry are left uninitialised (basd_pchol_f64_masked)."""
    _need_cuda(a)
    a = a.contiguous()
    if dmax_ref is not None:
        dmax_ref = dmax_ref.contiguous()
        assert dmax_ref.dtype == torch.float64 and dmax_ref.numel() == a.shape[0]
    batch, n, _ = a.shape
    ld = jacobi_ld(n)
    w0 = torch.empty(batch, n, ld, dtype=torch.float32, device=a.device)
    lwork = torch.empty(batch, n, n, dtype=torch.float64, device=a.device)
    piv = torch.empty(batch, n, dtype=torch.int32, device=a.device)
    rank = torch.empty(batch, dtype=torch.int32, device=a.device)
    _check(lib().basd_pchol_f64_masked(_ptr(a), batch, n, ctypes.c_double(tol), _ptr(dmax_ref), _ptr(w0), ld, _ptr(lwork),
                                       _ptr(piv), _ptr(rank), _ptr(_skip_mask(skip, batch)), _stream()),
           "basd_pchol_f64_masked")
    return w0, lwork, piv, rank


def jacobi_svd(w: torch.Tensor, m_rows: int, norm_rows: int | None = None, *, tol: float | None = None,
               max_sweeps: int = 60, sort: bool = True, active: torch.Tensor | None = None,
               active_rows: bool = False, flag_status: bool = True):
    """In-place one-sided Jacobi on w [batch, n_cols, ld] (column-major matrices).

    Returns (sigma [batch, n_cols], sweeps [batch]); w's columns become sigma_c * u_c.
    ``flag_status=False``: do not report non-convergence / non-finite values into the health word (single-sweep
    visits of a block tournament stop early on purpose).
    """
    _need_cuda(w)
    assert w.is_contiguous() and w.dtype == torch.float32
    batch, n_cols, ld = w.shape
    if norm_rows is None:
        norm_rows = m_rows
    if tol is None:
        tol = (m_rows ** 0.5) * 5.96e-8
    sigma = torch.empty(batch, n_cols, dtype=torch.float32, device=w.device)
    sweeps = torch.empty(batch, dtype=torch.int32, device=w.device)
    _check(lib().basd_jacobi_svd(_ptr(w), batch, m_rows, n_cols, ld, norm_rows, ctypes.c_float(tol),
                                 max_sweeps, int(sort), _ptr(sigma), _ptr(sweeps),
                                 _ptr(None if active is None else active.contiguous().int()), int(active_rows),
                                 _ptr(status_word(w.device) if flag_status else None), _stream()),
           "basd_jacobi_svd")
    return sigma, sweeps


def jacobi_fits(n_cols: int, m_rows: int) -> bool:
    """Size rule of the host code (layouts, which Procrustes side is taken): the matrix with its padded columns fits
    160 KiB.  It was the bound of an LDS-resident kernel that no longer exists; the value is kept because changing it
    changes results.  basd_jacobi_svd has its own, narrower shape check."""
    return n_cols <= 256 and n_cols * jacobi_ld(m_rows) * 4 + 520 * 4 <= JACOBI_LDS_BYTES


JACOBI_TALL_ROWS = 384       # register-resident variant for block pairs: n_cols <= 192 columns of up to 384 rows


def mp_rank(evals: torch.Tensor, rows: int, d: int, cap: int) -> torch.Tensor:
    """evals [batch, n] (eigenvalues of X^T X) -> int32 ranks [batch], on device."""
    _need_cuda(evals)
    evals = evals.contiguous().float()
    batch, n = evals.shape
    ranks = torch.empty(batch, dtype=torch.int32, device=evals.device)
    _check(lib().basd_mp_rank(_ptr(evals), batch, n, ctypes.c_int64(rows), d, cap, _ptr(ranks),
                              _ptr(status_word(evals.device)), _stream()), "basd_mp_rank")
    return ranks


TRIDIAG_MAX_N = 2048         # largest order basd_sym_tridiag_f64 / basd_tridiag_mp_rank take (diag + off^2 in LDS)


def sym_tridiag(a64: torch.Tensor):
    """a64 [n, n] fp64, symmetric with both triangles valid, 2 <= n <= 2048 -> (diag [n], off [n - 1]) fp64 of a
    tridiagonal matrix with the same eigenvalues (unblocked Householder, 2 (n - 2) + 1 launches on the current stream,
    no host sync).  ``a64`` is SCRATCH: it is overwritten by the reduction."""
    _need_cuda(a64)
    assert a64.dtype == torch.float64 and a64.dim() == 2 and a64.shape[0] == a64.shape[1] and a64.is_contiguous()
    n = a64.shape[0]
    diag = torch.empty(n, dtype=torch.float64, device=a64.device)
    off = torch.empty(max(n - 1, 0), dtype=torch.float64, device=a64.device)
    work = torch.empty(lib().basd_sym_tridiag_f64_workspace_bytes(n) // 8, dtype=torch.float64, device=a64.device)
    _check(lib().basd_sym_tridiag_f64(_ptr(a64), n, _ptr(diag), _ptr(off), _ptr(work), _stream()), "basd_sym_tridiag_f64")
    return diag, off


def tridiag_mp_rank(diag: torch.Tensor, off: torch.Tensor, rows: int, d: int, cap: int) -> torch.Tensor:
    """(diag [n], off [n - 1]) fp64 of a tridiagonal matrix with the spectrum of the smaller-side Gram of an [rows, d]
    matrix (n <= min(rows, d)) -> int32 [1] Marchenko-Pastur rank on the device, by Sturm counts (no spectrum)."""
    _need_cuda(diag, off)
    assert diag.dtype == torch.float64 and off.dtype == torch.float64 and off.numel() == diag.numel() - 1
    diag, off = diag.contiguous(), off.contiguous()
    rank = torch.empty(1, dtype=torch.int32, device=diag.device)
    _check(lib().basd_tridiag_mp_rank(_ptr(diag), _ptr(off), diag.numel(), ctypes.c_int64(rows), d, cap, _ptr(rank),
                                      _ptr(status_word(diag.device)), _stream()), "basd_tridiag_mp_rank")
    return rank


def flag_if_exceeds(values: torch.Tensor, tol: float, bit: int) -> None:
    """OR ``bit`` into the device health word if any entry of ``values`` (fp64) is not <= tol (NaN included): atomic,
    no host sync."""
    _need_cuda(values)
    v = values.detach().reshape(-1).to(torch.float64).contiguous()
    _check(lib().basd_flag_if_exceeds_f64(_ptr(v), ctypes.c_int64(v.numel()), ctypes.c_double(tol), int(bit),
                                          _ptr(status_word(v.device)), _stream()), "basd_flag_if_exceeds_f64")


def angle_weights(sigma: torch.Tensor, sw: torch.Tensor, log_temp: torch.Tensor, unnormalised: bool):
    """sigma [E, L, D] cosines, sw [L, D] masked teacher singular values, log_temp [E] ->
    (d2 [E, L], pre [E, L], weights [E, L], coef [E, L, D]) fp32; see basd_angle_weights."""
    _need_cuda(sigma, sw, log_temp)
    sigma, sw, log_temp = sigma.contiguous().float(), sw.contiguous().float(), log_temp.detach().contiguous().float()
    e, l, d = sigma.shape
    assert sw.shape == (l, d) and log_temp.numel() == e
    d2 = torch.empty(e, l, dtype=torch.float32, device=sigma.device)
    pre, wts = torch.empty_like(d2), torch.empty_like(d2)
    coef = torch.empty(e, l, d, dtype=torch.float32, device=sigma.device)
    _check(lib().basd_angle_weights(_ptr(sigma), _ptr(sw), _ptr(log_temp), e, l, d, int(unnormalised), _ptr(d2), _ptr(pre),
                                    _ptr(wts), _ptr(coef), _stream()), "basd_angle_weights")
    return d2, pre, wts, coef


def angle_weights_bwd(g_w, g_pre_out, wts, d2, log_temp, t_seed, v_s, lam_s, proj_s):
    """Backward of the selector weights as ONE C call (basd_angle_weights_bwd): -> (g_log_temp [E] fp32,
    w_tok [E, D_s, D_s] fp32 with d loss / d s_i = (s_i - column mean) w_tok[i])."""
    _need_cuda(g_w, wts, d2, log_temp, t_seed, v_s, lam_s, proj_s)
    f32 = lambda t_: t_.detach().contiguous().float()
    g_w, wts, d2, log_temp, t_seed, v_s, proj_s = map(f32, (g_w, wts, d2, log_temp, t_seed, v_s, proj_s))
    g_pre_out = None if g_pre_out is None else f32(g_pre_out)
    lam_s = lam_s.detach().contiguous().double()
    e, l, d, _ = t_seed.shape
    d_s = proj_s.shape[1]
    assert proj_s.shape[0] == d and v_s.shape == (e, d, d) and lam_s.shape == (e, d) and g_w.shape == (e, l)
    g_lt = torch.empty(e, dtype=torch.float32, device=g_w.device)
    w_tok = torch.empty(e, d_s, d_s, dtype=torch.float32, device=g_w.device)
    ws = torch.empty(int(lib().basd_angle_weights_bwd_workspace_bytes(e, d, d_s)), dtype=torch.uint8, device=g_w.device)
    _check(lib().basd_angle_weights_bwd(_ptr(g_w), _ptr(g_pre_out), _ptr(wts), _ptr(d2), _ptr(log_temp), _ptr(t_seed),
                                        _ptr(v_s), _ptr(lam_s), _ptr(proj_s), e, l, d, d_s, _ptr(g_lt), _ptr(w_tok),
                                        _ptr(ws), ctypes.c_int64(ws.numel()), _stream()), "basd_angle_weights_bwd")
    return g_lt, w_tok


SELECTOR_MAX_D = 192         # widest frame the selector entries take (the LDS-resident eigensolver)


def selector_frames(unc: torch.Tensor, csum: torch.Tensor, m_rows: int, with_ranks: bool):
    """Selector frames of one side as ONE C call (basd_selector_frames): unc [n, D, D] fp64 uncentred Grams (lower
    triangles), csum [n, D] fp64 column sums, m_rows tokens per layer -> (ranks int32 [n] | None, sigma [n, D] fp32,
    lam [n, D] fp64, v [n, D, D] fp32); with ranks, sigma and the rows of v are masked at the rank."""
    _need_cuda(unc, csum)
    unc = unc.detach().contiguous().double()
    csum = csum.detach().contiguous().double()
    n, d, _ = unc.shape
    assert csum.shape == (n, d)
    dev = unc.device
    ranks = torch.empty(n, dtype=torch.int32, device=dev) if with_ranks else None
    sigma = torch.empty(n, d, dtype=torch.float32, device=dev)
    lam = torch.empty(n, d, dtype=torch.float64, device=dev)
    v = torch.empty(n, d, d, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib().basd_selector_frames_workspace_bytes(n, d)), dtype=torch.uint8, device=dev)
    _check(lib().basd_selector_frames(_ptr(unc), _ptr(csum), n, ctypes.c_int64(m_rows), d, int(with_ranks), _ptr(ranks),
                                      _ptr(sigma), _ptr(lam), _ptr(v), _ptr(status_word(dev)), _ptr(ws),
                                      ctypes.c_int64(ws.numel()), _stream()), "basd_selector_frames")
    return ranks, sigma, lam, v


def selector_weights(v_s: torch.Tensor, ranks: torch.Tensor, vm_t: torch.Tensor, sw: torch.Tensor,
                     log_temp: torch.Tensor):
    """Selector weights as ONE C call (basd_selector_weights): v_s [E, D, D] student frames, ranks [L] int32, vm_t
    [L, D, D] / sw [L, D] rank-masked teacher frames, log_temp [E] -> (weights, pre, d2 [E, L] fp32,
    t_seed [E, L, D, D] fp32: the seeds basd_angle_weights_bwd takes)."""
    _need_cuda(v_s, ranks, vm_t, sw, log_temp)
    f32 = lambda t_: t_.detach().contiguous().float()
    v_s, vm_t, sw, log_temp = map(f32, (v_s, vm_t, sw, log_temp))
    ranks = ranks.detach().contiguous().int()
    e, d, _ = v_s.shape
    l = vm_t.shape[0]
    assert vm_t.shape == (l, d, d) and sw.shape == (l, d) and ranks.numel() == l and log_temp.numel() == e
    dev = v_s.device
    wts = torch.empty(e, l, dtype=torch.float32, device=dev)
    pre, d2 = torch.empty_like(wts), torch.empty_like(wts)
    t_seed = torch.empty(e, l, d, d, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib().basd_selector_weights_workspace_bytes(e, l, d)), dtype=torch.uint8, device=dev)
    _check(lib().basd_selector_weights(_ptr(v_s), _ptr(ranks), _ptr(vm_t), _ptr(sw), _ptr(log_temp), e, l, d, _ptr(wts),
                                       _ptr(pre), _ptr(d2), _ptr(t_seed), _ptr(status_word(dev)), _ptr(ws),
                                       ctypes.c_int64(ws.numel()), _stream()), "basd_selector_weights")
    return wts, pre, d2, t_seed


def _ptr_table(layers: list[torch.Tensor]):
    """Host array of device pointers (handed to the kernel by value: no H2D copy, graph-capturable)."""
    return (ctypes.c_void_p * len(layers))(*[t.data_ptr() for t in layers])


def _layer_views(layers):
    """Common (per_batch, batch_stride) of same-shape layers; copies only layers that are not
    dense-per-sample views."""
    shape = layers[0].shape
    assert all(t.shape == shape and t.dtype == layers[0].dtype for t in layers)
    per_batch = layers[0][0].numel()
    def dense_per_sample(t):
        return t[0].is_contiguous() and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0
    strides = {t.stride(0) for t in layers}
    if len(strides) == 1 and all(dense_per_sample(t) for t in layers):
        return list(layers), per_batch, layers[0].stride(0)
    return [t.contiguous() for t in layers], per_batch, per_batch


def mix_tokens(layers: list[torch.Tensor], w: torch.Tensor) -> torch.Tensor:
    """layers: L same-shape [B, ...] tensors (batch-strided views allowed); w [E, L] f32 -> [E, *shape] f32."""
    _need_cuda(*layers, w)
    code = _dtype_code(layers[0])
    layers, per_batch, bstride = _layer_views(layers)
    E, L = w.shape
    assert L == len(layers)
    elems = layers[0].numel()
    out = torch.empty((E,) + tuple(layers[0].shape), dtype=torch.float32, device=w.device)
    table = _ptr_table(layers)
    i64 = ctypes.c_int64
    _check(lib().basd_mix_tokens(table, code, L, E, _ptr(w.contiguous().float()), i64(elems), i64(per_batch),
                                 i64(bstride), _ptr(out), _stream()), "basd_mix_tokens")
    return out


def mix_grad_dots(layers: list[torch.Tensor], g: torch.Tensor) -> torch.Tensor:
    """dots[i, j] = <g[i], layers[j]>; g [E, *shape] f32 -> [E, L] f64."""
    _need_cuda(*layers, g)
    code = _dtype_code(layers[0])
    layers, per_batch, bstride = _layer_views(layers)
    E, L = g.shape[0], len(layers)
    elems = layers[0].numel()
    assert g.numel() == E * elems and g.dtype == torch.float32
    dots = torch.zeros(E, L, dtype=torch.float64, device=g.device)
    table = _ptr_table(layers)
    i64 = ctypes.c_int64
    _check(lib().basd_mix_grad_dots(table, code, L, E, _ptr(g.contiguous()), i64(elems), i64(per_batch),
                                    i64(bstride), _ptr(dots), _stream()), "basd_mix_grad_dots")
    return dots


def procrustes_prep(s: torch.Tensor, t: torch.Tensor, imp: torch.Tensor, out=None):
    """s [B,N_s,D_s] (f32/bf16, batch-strided view allowed), t [B,N_t,D_t] f32, imp [B,N_t] f32
    -> s_w, t_w, a, tr[B,2]  (written into ``out`` = (s_w, t_w, a, tr) when given: contiguous fp32 views)."""
    _need_cuda(s, t, imp)
    if not (s[0].is_contiguous() and s.data_ptr() % 16 == 0):
        s = s.contiguous()
    t = t.contiguous().float()
    imp = imp.contiguous().float()
    B, N_s, D_s = s.shape
    _, N_t, D_t = t.shape
    dev = s.device
    if out is None:
        s_w = torch.empty(B, N_s, D_s, dtype=torch.float32, device=dev)
        t_w = torch.empty(B, N_s, D_t, dtype=torch.float32, device=dev)
        a = torch.empty(B, N_s, dtype=torch.float32, device=dev)
        tr = torch.empty(B, 2, dtype=torch.float32, device=dev)
    else:
        s_w, t_w, a, tr = out
        assert s_w.shape == (B, N_s, D_s) and t_w.shape == (B, N_s, D_t) and a.shape == (B, N_s) and tr.shape == (B, 2)
        for o in out:
            assert o.dtype == torch.float32 and o.is_contiguous()
    _check(lib().basd_procrustes_prep(_ptr(s), _dtype_code(s), ctypes.c_int64(s.stride(0)), _ptr(t), _ptr(imp), B, N_s,
                                      N_t, D_s, D_t, _ptr(s_w), _ptr(t_w), _ptr(a), _ptr(tr), _stream()),
           "basd_procrustes_prep")
    return s_w, t_w, a, tr


def procrustes_bwd_rows(r: torch.Tensor, w: torch.Tensor, a: torch.Tensor, gl: torch.Tensor, out_dtype=torch.float32):
    """r = (other side) G^T, w [B, N, D] fp32, a [B, N], gl [B] -> with R = w - r:
    (2 gl sqrt(a) R  [B, N, D] in out_dtype, 2 gl <R, w>_d  [B, N]).  With out_dtype fp32 the result overwrites ``r``."""
    _need_cuda(r, w, a, gl)
    for t_ in (r, w, a, gl):
        assert t_.dtype == torch.float32 and t_.is_contiguous()
    B, N, D = r.shape
    assert w.shape == r.shape and a.shape == (B, N) and gl.numel() == B
    out = r if out_dtype == torch.float32 else torch.empty(B, N, D, dtype=out_dtype, device=r.device)
    rowdot = torch.empty(B, N, dtype=torch.float32, device=r.device)
    code = DTYPE_F32 if out_dtype == torch.float32 else DTYPE_BF16
    _check(lib().basd_procrustes_bwd_rows(_ptr(r), _ptr(w), _ptr(a), _ptr(gl), ctypes.c_int64(B * N), N, D, _ptr(out),
                                          code, _ptr(rowdot), _stream()), "basd_procrustes_bwd_rows")
    return out, rowdot


def sf_adamw_step(y, g, z, v, *, lr, beta1, beta2, eps, weight_decay, ckp1, bias_correction2) -> None:
    """In-place fused Schedule-Free AdamW step on flat fp32 buffers (all same length)."""
    _need_cuda(y, g, z, v)
    n = y.numel()
    assert g.numel() == n and z.numel() == n and v.numel() == n
    for t in (y, g, z, v):
        assert t.dtype == torch.float32 and t.is_contiguous()
    f = ctypes.c_double
    _check(lib().basd_sf_adamw_step(_ptr(y), _ptr(g), _ptr(z), _ptr(v), ctypes.c_int64(n), f(lr), f(beta1),
                                    f(beta2), f(eps), f(weight_decay), f(ckp1), f(bias_correction2), _stream()),
           "basd_sf_adamw_step")


def lerp_(y, z, w: float) -> None:
    _need_cuda(y, z)
    assert y.dtype == torch.float32 and z.dtype == torch.float32 and y.numel() == z.numel()
    _check(lib().basd_lerp(_ptr(y), _ptr(z), ctypes.c_int64(y.numel()), ctypes.c_float(w), _stream()), "basd_lerp")


# Scratch buffers of the workspace entries (basd_procrustes_fwd, basd_wgrad_bf16_ws): one per (kind, device), grown on
# demand.  A buffer that has been handed out is NEVER freed -- a captured hipGraph keeps replaying into the address it
# was captured with, so an outgrown buffer is parked in ``_RETIRED`` instead of being released -- and a call from a
# stream other than the buffer's last user is ordered behind that user (event wait), so two streams (or two trainers)
# sharing a device never write the same scratch concurrently.
_SCRATCH: dict = {}
_RETIRED: list = []


class _Scratch:
    __slots__ = ("buf", "stream", "event", "shared")

    def __init__(self, buf, stream):
        self.buf, self.stream, self.event, self.shared = buf, stream, None, False


def _scratch(kind: str, device: torch.device, nbytes: int, min_bytes: int = 0) -> "_Scratch":
    key = (kind, device.index)
    cur = torch.cuda.current_stream(device)
    rec = _SCRATCH.get(key)
    if rec is None or rec.buf.numel() < nbytes:
        if rec is not None:
            _RETIRED.append(rec.buf)
        rec = _SCRATCH[key] = _Scratch(torch.empty(max(nbytes, min_bytes), dtype=torch.uint8, device=device), cur)
    elif rec.stream.cuda_stream != cur.cuda_stream:
        if rec.event is not None:
            cur.wait_event(rec.event)
        else:
            cur.wait_stream(rec.stream)
        rec.shared = True                       # from now on every use leaves an event behind
        rec.stream = cur
    return rec


def _scratch_used(rec: "_Scratch") -> None:
    if rec.shared:
        rec.event = torch.cuda.Event()
        rec.event.record(rec.stream)



def procrustes_fwd(s_w: torch.Tensor, t_w: torch.Tensor, tol: float = 1e-13):
    """s_w [batch, n, d_s], t_w [batch, n, d_t] fp32 (weighted, centred tokens from ``procrustes_prep``) ->
    (nuc [batch], fac_s, a_t [batch, n, n]) fp32; fac_s = t_w G^T [batch, n, d_s] if n > d_s else a_s [batch, n, n]
    (see basd_procrustes_fwd).  One C call; the scratch comes from ``_scratch`` (per device, never freed once used)."""
    _need_cuda(s_w, t_w)
    assert s_w.dtype == torch.float32 and t_w.dtype == torch.float32 and s_w.shape[:2] == t_w.shape[:2]
    s_w, t_w = s_w.contiguous(), t_w.contiguous()
    batch, n, d_s = s_w.shape
    d_t = t_w.shape[2]
    need = int(lib().basd_procrustes_workspace_bytes(batch, n, d_s, d_t))
    rec = _scratch("procrustes", s_w.device, need)
    ws = rec.buf
    nuc = torch.empty(batch, dtype=torch.float32, device=s_w.device)
    fac_s = torch.empty(batch, n, d_s if n > d_s else n, dtype=torch.float32, device=s_w.device)
    a_t = torch.empty(batch, n, n, dtype=torch.float32, device=s_w.device)
    _check(lib().basd_procrustes_fwd(_ptr(s_w), _ptr(t_w), batch, n, d_s, d_t, ctypes.c_double(tol), _ptr(nuc),
                                     _ptr(fac_s), _ptr(a_t), _ptr(status_word(s_w.device)), _ptr(ws),
                                     ctypes.c_int64(ws.numel()), _stream()), "basd_procrustes_fwd")
    _scratch_used(rec)
    return nuc, fac_s, a_t


def procrustes_bwd_supported(n: int, d_s: int, d_t: int) -> bool:
    # n <= 256 with n % 4 == 0: one workgroup per matrix; everything else up to 1024 rows: the row-tiled kernel
    return 4 <= n <= 1024 and d_t % 16 == 0 and d_t >= 16 and (n > d_s or (d_s % 16 == 0 and d_s >= 16)) and d_s % 4 == 0


def procrustes_bwd(s_w: torch.Tensor, t_w: torch.Tensor, a: torch.Tensor, gl: torch.Tensor, fac_s: torch.Tensor,
                   a_t: torch.Tensor, s_dtype=torch.float32):
    """Backward of ``procrustes_fwd`` as ONE C call (basd_procrustes_bwd): -> (g_s [batch, n, d_s] in ``s_dtype``,
    g_t [batch, n, d_t] fp32, g_a [batch, n] fp32).  The big product a_t t_w runs as a bf16 three-product split with the
    residual / scaling / row dots in its epilogue."""
    _need_cuda(s_w, t_w, a, gl, fac_s, a_t)
    for t_ in (s_w, t_w, a, gl, fac_s, a_t):
        assert t_.dtype == torch.float32 and t_.is_contiguous()
    batch, n, d_s = s_w.shape
    d_t = t_w.shape[2]
    assert a_t.shape == (batch, n, n) and fac_s.shape == (batch, n, n if n <= d_s else d_s) and gl.numel() == batch
    g_s = torch.empty(batch, n, d_s, dtype=s_dtype, device=s_w.device)
    g_t = torch.empty(batch, n, d_t, dtype=torch.float32, device=s_w.device)
    g_a = torch.empty(batch, n, dtype=torch.float32, device=s_w.device)
    ws = torch.empty(int(lib().basd_procrustes_bwd_workspace_bytes(batch, n)), dtype=torch.uint8, device=s_w.device)
    code = DTYPE_F32 if s_dtype == torch.float32 else DTYPE_BF16
    _check(lib().basd_procrustes_bwd(_ptr(s_w), _ptr(t_w), _ptr(a), _ptr(gl), _ptr(fac_s), _ptr(a_t), batch, n, d_s, d_t,
                                     _ptr(g_s), code, _ptr(g_t), _ptr(g_a), _ptr(ws), ctypes.c_int64(ws.numel()),
                                     _stream()), "basd_procrustes_bwd")
    return g_s, g_t, g_a


def ce_uwso(logits: torch.Tensor, targets: torch.Tensor, smoothing: float, geo: torch.Tensor | None):
    """logits [B, C] fp32; targets [B, C] float (soft) or [B] int64; geo: 0-d fp32 device tensor | None ->
    (out4 = [total, ce, w_ce, w_geo] fp32 device, dlogits [B, C] = d total / d logits)."""
    _need_cuda(logits, targets, geo)
    assert logits.dtype == torch.float32 and logits.dim() == 2
    logits = logits.contiguous()
    b, c = logits.shape
    soft = labels = None
    if targets.dim() == 2:
        assert targets.shape == (b, c)
        soft = targets.float().contiguous()
    else:
        assert targets.shape == (b,)
        labels = targets.to(torch.int64).contiguous()
    if geo is not None:
        geo = geo.detach().float().reshape(1).contiguous()
    row = torch.empty(b, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits)
    out4 = torch.empty(4, dtype=torch.float32, device=logits.device)
    _check(lib().basd_ce_uwso(_ptr(logits), _ptr(soft), _ptr(labels), b, c, ctypes.c_float(smoothing), _ptr(geo), _ptr(row),
                              _ptr(dl), _ptr(out4), _stream()), "basd_ce_uwso")
    return out4, dl


def transpose_table(master: torch.Tensor, out: torch.Tensor, table) -> None:
    """table: list of (src offset, dst offset, rows, cols); out[dst + c rows + r] = bf16(master[src + r cols + c]) for
    every entry, one launch (weights^T for the input-gradient GEMMs, refreshed once per step)."""
    _need_cuda(master, out)
    assert master.dtype == torch.float32 and out.dtype == torch.bfloat16
    if not table:
        return
    for src, dst, rows, cols in table:
        assert 0 <= src and src + rows * cols <= master.numel() and 0 <= dst and dst + rows * cols <= out.numel()
    flat = (ctypes.c_int64 * (4 * len(table)))(*[int(v) for e in table for v in e])
    _check(lib().basd_transpose_bf16_table(_ptr(master), _ptr(out), ctypes.cast(flat, ctypes.c_void_p), len(table),
                                           _stream()), "basd_transpose_bf16_table")


def bgemm_f64(a: torch.Tensor, b: torch.Tensor, *, trans_a: bool = False, trans_b: bool = False,
              out_dtype=torch.float64, symmetric: bool = False, skip: torch.Tensor | None = None) -> torch.Tensor:
    """Batched op(a) @ op(b) with fp64 accumulation; a, b [batch, r, c] fp32/fp64 contiguous.  An operand with batch
    1 is broadcast over the other one's batch (batch stride 0: no copies).  ``skip``: see ``pchol``."""
    _need_cuda(a, b)
    a, b = a.contiguous(), b.contiguous()
    code = {torch.float32: DTYPE_F32, torch.float64: DTYPE_F64}
    batch = max(a.shape[0], b.shape[0])
    M, K = (a.shape[2], a.shape[1]) if trans_a else (a.shape[1], a.shape[2])
    K2, N = (b.shape[2], b.shape[1]) if trans_b else (b.shape[1], b.shape[2])
    assert K == K2 and a.shape[0] in (1, batch) and b.shape[0] in (1, batch), (a.shape, b.shape, trans_a, trans_b)
    c = torch.empty(batch, M, N, dtype=out_dtype, device=a.device)
    i64 = ctypes.c_int64
    sa = a.shape[1] * a.shape[2] if a.shape[0] == batch else 0
    sb = b.shape[1] * b.shape[2] if b.shape[0] == batch else 0
    _check(lib().basd_bgemm_f64_masked(_ptr(a), code[a.dtype], i64(sa), a.shape[2], int(trans_a),
                                       _ptr(b), code[b.dtype], i64(sb), b.shape[2], int(trans_b),
                                       _ptr(c), code[out_dtype], i64(M * N), N, batch, M, N, K, int(symmetric),
                                       _ptr(_skip_mask(skip, batch)), _stream()),
           "basd_bgemm_f64_masked")
    return c


def trinv(lwork: torch.Tensor, piv: torch.Tensor, rank: torch.Tensor, skip: torch.Tensor | None = None) -> torch.Tensor:
    """(lwork, piv, rank) from pchol -> L_p^-1 P  [batch, n, n] fp64 (see basd_trinv_f64).  ``skip``: see ``pchol``."""
    _need_cuda(lwork, piv, rank)
    batch, n, _ = lwork.shape
    out = torch.empty(batch, n, n, dtype=torch.float64, device=lwork.device)
    _check(lib().basd_trinv_f64_masked(_ptr(lwork.contiguous()), _ptr(piv.contiguous()), _ptr(rank.contiguous()), batch, n,
                                       _ptr(out), _ptr(_skip_mask(skip, batch)), _stream()), "basd_trinv_f64_masked")
    return out


# Tiles a workgroup of the persistent GEMM kernel multiplies before it retires (basd_gemm_bf16's ``tile_run``): 0 = its
# whole share, the fastest form when the GEMM has the GPU to itself (the default: inference, eager / single-stream steps);
# the Trainer sets basd.gemm_tile_run (default 1) while its two-stream pipelined step is in use (a persistent launch holds
# every CU until it ends and the other stream's short kernels queue behind it: measured 41.3 vs 39.5 ms per c2 step with
# 2; training/trainer.py has the later measurements that made 1 the default).
GEMM_TILE_RUN = 0
# The same for the GEMMs of the TRAINED model that take the persistent kernel (fc1 + GELU forward, fc2 input gradient +
# GELU backward: basd_gemm_bf16_gelu_fwd / _bwd): they are on the step's own chain, not on the side stream.
# Fully persistent (0) whatever the scope above says: pipelined c2 step 32.54 / 32.54 ms against 32.77 / 32.82 with one
# tile per workgroup and 32.65 / 32.60 with two (same box).  BASD_GEMM_TILE_RUN_STUDENT overrides (A/B runs).
GEMM_TILE_RUN_STUDENT = int(os.environ.get("BASD_GEMM_TILE_RUN_STUDENT", "0"))


def _student_tile_run() -> int:
    return GEMM_TILE_RUN_STUDENT


@contextlib.contextmanager
def gemm_tile_run(k: int):
    """``with gemm_tile_run(2):`` -- the GEMM entries called inside retire their workgroups every k tiles (0: fully
    persistent, the fastest form when the launch has the GPU to itself).  Scoped: the Trainer wraps only the steps that
    really run two streams; evaluation, inference and any other model in the process keep the default."""
    global GEMM_TILE_RUN
    prev, GEMM_TILE_RUN = GEMM_TILE_RUN, int(k)
    try:
        yield
    finally:
        GEMM_TILE_RUN = prev


def gemm_supported(n: int, k: int) -> bool:
    return k % 64 == 0 and k >= 64 and n >= 128 and (n % 256 == 0 or n % 192 == 0 or n % 128 == 0)


# activation names of gemm_bf16(act=...) -> ``act`` of basd_gemm_bf16_act (nn.GELU(), QuickGELU, nn.GELU("tanh"))
GEMM_ACTS = {"gelu": 1, "quick_gelu": 2, "gelu_tanh": 3}


def gemm_bf16(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, gelu: bool = False,
              act: str | None = None) -> torch.Tensor:
    """x [..., K], w [N, K], bias [N] | None (all bf16) -> epi(x w^T + bias) [..., N] bf16; epi = exact-erf GELU if
    ``gelu`` or ``act == "gelu"``, QuickGELU / tanh-GELU for ``act`` "quick_gelu" / "gelu_tanh" (basd_gemm_bf16_act).
    Inference / explicit-backward building block (no autograd)."""
    _need_cuda(x, w, bias)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and (bias is None or bias.dtype == torch.bfloat16)
    if act is not None and act not in GEMM_ACTS:
        raise BasdNativeError(f"gemm_bf16: unknown activation {act!r} (known: {sorted(GEMM_ACTS)})")
    k = x.shape[-1]
    n = w.shape[0]
    assert w.shape[1] == k and gemm_supported(n, k), (tuple(w.shape), k)
    x2 = x.reshape(-1, k)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    w = w.contiguous()
    y = torch.empty(x2.shape[0], n, dtype=torch.bfloat16, device=x.device)
    b = None if bias is None else bias.contiguous()
    if act is not None and act != "gelu":
        _check(lib().basd_gemm_bf16_act(_ptr(x2), _ptr(w), _ptr(b), _ptr(y), ctypes.c_int64(x2.shape[0]), n, k,
                                        GEMM_ACTS[act], GEMM_TILE_RUN, _stream()), "basd_gemm_bf16_act")
        return y.view(*x.shape[:-1], n)
    epi = 2 if gelu or act == "gelu" else (1 if bias is not None else 0)
    _check(lib().basd_gemm_bf16(_ptr(x2), _ptr(w), _ptr(b), _ptr(y),
                                ctypes.c_int64(x2.shape[0]), n, k, epi, GEMM_TILE_RUN, _stream()), "basd_gemm_bf16")
    return y.view(*x.shape[:-1], n)


def gemm_swiglu_supported(h: int, k: int) -> bool:
    """shapes basd_gemm_bf16_swiglu takes: only the 256-column tiles pair the two halves (2 H % 256 == 0)"""
    return h >= 128 and h % 128 == 0 and k >= 64 and k % 64 == 0


def swiglu_pack_index(h: int) -> torch.Tensor:
    """source row of every packed row (int64 [2 H], CPU): packed row p = 64 * (i // 32) + 32 * s + i % 32 holds row
    s * H + i of the hub layout (s = 0: the x1 / w1 half, rows 0 .. H - 1; s = 1: the x2 / w2 half) -- the row map in
    the header of basd_gemm_bf16_swiglu."""
    assert h % 32 == 0, h
    p = torch.arange(2 * h)
    return ((p // 32) % 2) * h + (p // 64) * 32 + p % 32


def swiglu_pack(w12: torch.Tensor, b12: torch.Tensor | None = None):
    """hub ``w12.weight`` [2 H, K] (+ ``w12.bias`` [2 H]) -> the packed operands of basd_gemm_bf16_swiglu: blocks of
    32 w1 rows alternating with the 32 w2 rows of the same outputs.  Pure torch (any device, any dtype): a row
    permutation, built once per frozen layer."""
    idx = swiglu_pack_index(w12.shape[0] // 2).to(w12.device)
    return w12.index_select(0, idx).contiguous(), (None if b12 is None else b12.index_select(0, idx).contiguous())


def gemm_bf16_swiglu(x: torch.Tensor, w12p: torch.Tensor, b12p: torch.Tensor | None) -> torch.Tensor:
    """x [..., K], w12p [2 H, K], b12p [2 H] | None (bf16; the PACKED forms of swiglu_pack) -> bf16(silu(x1) * x2)
    [..., H] with x1, x2 the two halves of the hub's w12(x): one GEMM with the gate in its epilogue
    (basd_gemm_bf16_swiglu).  Inference building block (no autograd)."""
    _need_cuda(x, w12p, b12p)
    assert x.dtype == torch.bfloat16 and w12p.dtype == torch.bfloat16 and (b12p is None or b12p.dtype == torch.bfloat16)
    k, h = x.shape[-1], w12p.shape[0] // 2
    assert w12p.shape == (2 * h, k) and gemm_swiglu_supported(h, k), (tuple(w12p.shape), k)
    assert b12p is None or b12p.numel() == 2 * h
    x2 = x.reshape(-1, k)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = torch.empty(x2.shape[0], h, dtype=torch.bfloat16, device=x.device)
    _check(lib().basd_gemm_bf16_swiglu(_ptr(x2), _ptr(w12p.contiguous()), _ptr(None if b12p is None else b12p.contiguous()),
                                       _ptr(y), ctypes.c_int64(x2.shape[0]), h, k, GEMM_TILE_RUN, _stream()),
           "basd_gemm_bf16_swiglu")
    return y.view(*x.shape[:-1], h)


def gemm_gelu_fwd(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None):
    """x [..., K], w [N, K], bias [N] | None (bf16) -> (pre, act) [..., N] bf16: pre = x w^T + bias rounded to bf16,
    act = gelu(pre) -- fc1 + nn.GELU of a trained block in one launch, ``pre`` saved for ``gemm_gelu_bwd``."""
    _need_cuda(x, w, bias)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and (bias is None or bias.dtype == torch.bfloat16)
    k, n = x.shape[-1], w.shape[0]
    assert w.shape[1] == k and gemm_supported(n, k), (tuple(w.shape), k)
    x2 = x.reshape(-1, k)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    pre = torch.empty(x2.shape[0], n, dtype=torch.bfloat16, device=x.device)
    act = torch.empty_like(pre)
    _check(lib().basd_gemm_bf16_gelu_fwd(_ptr(x2), _ptr(w.contiguous()), _ptr(None if bias is None else bias.contiguous()),
                                         _ptr(pre), _ptr(act), ctypes.c_int64(x2.shape[0]), n, k, _student_tile_run(),
                                         _stream()),
           "basd_gemm_bf16_gelu_fwd")
    return pre.view(*x.shape[:-1], n), act.view(*x.shape[:-1], n)


def gemm_gelu_bwd(dy: torch.Tensor, wt: torch.Tensor, pre: torch.Tensor) -> torch.Tensor:
    """dy [..., K], wt [N, K] (= fc2.weight^T, contiguous), pre [..., N] (bf16) -> (dy wt^T) * gelu'(pre) [..., N] bf16:
    the input gradient of fc2 and the GELU backward in one launch."""
    _need_cuda(dy, wt, pre)
    assert dy.dtype == torch.bfloat16 and wt.dtype == torch.bfloat16 and pre.dtype == torch.bfloat16
    k, n = dy.shape[-1], wt.shape[0]
    assert wt.shape[1] == k and pre.shape[-1] == n and gemm_supported(n, k), (tuple(wt.shape), tuple(pre.shape), k)
    dy2 = dy.reshape(-1, k)
    if not dy2.is_contiguous():
        dy2 = dy2.contiguous()
    pre2 = pre.reshape(-1, n)
    assert pre2.is_contiguous() and pre2.shape[0] == dy2.shape[0]
    out = torch.empty_like(pre2)
    _check(lib().basd_gemm_bf16_gelu_bwd(_ptr(dy2), _ptr(wt.contiguous()), _ptr(pre2), _ptr(out),
                                         ctypes.c_int64(dy2.shape[0]), n, k, _student_tile_run(), _stream()),
           "basd_gemm_bf16_gelu_bwd")
    return out.view(*pre.shape)


def wgrad_supported(n: int, k: int) -> bool:
    return n % 64 == 0 and k % 64 == 0 and n >= 64 and k >= 64


def wgrad_bf16(dy: torch.Tensor, x: torch.Tensor, need_bias: bool = True, out_w: torch.Tensor | None = None,
               out_b: torch.Tensor | None = None):
    """dy [M, N], x [M, K] bf16 -> (dw [N, K] fp32, db [N] fp32 | None).

    With ``out_w`` / ``out_b`` (fp32, contiguous, e.g. views of the flat gradient buffer) the kernel
    ACCUMULATES into them and they are returned as is."""
    _need_cuda(dy, x)
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
    dy, x = dy.contiguous(), x.contiguous()
    m, n = dy.shape
    k = x.shape[1]
    dw = out_w if out_w is not None else torch.zeros(n, k, dtype=torch.float32, device=dy.device)
    db = out_b if out_b is not None else (torch.zeros(n, dtype=torch.float32, device=dy.device) if need_bias else None)
    assert dw.is_contiguous() and dw.dtype == torch.float32 and dw.shape == (n, k)
    need = int(lib().basd_wgrad_workspace_bytes(ctypes.c_int64(m), n, k))
    if need > 0:
        rec = _scratch("wgrad", dy.device, need, min_bytes=256 * 192 * 192 * 4)
        _check(lib().basd_wgrad_bf16_ws(_ptr(dy), _ptr(x), ctypes.c_int64(m), n, k, _ptr(dw), _ptr(db), _ptr(rec.buf),
                                        ctypes.c_int64(rec.buf.numel()), _stream()), "basd_wgrad_bf16_ws")
        _scratch_used(rec)
    else:
        _check(lib().basd_wgrad_bf16(_ptr(dy), _ptr(x), ctypes.c_int64(m), n, k, _ptr(dw), _ptr(db), _stream()),
               "basd_wgrad_bf16")
    return dw, db


# Attention past the single-workgroup kernels (csrc/attention_long.hip): 1 <= T <= LONG_ATTENTION_MAX_T, hd 64 | 80.
# The entries below call the long kernels ONLY for shapes the short ones refuse.
LONG_ATTENTION_MAX_T = 1024


def _long_attention_ok(t: int, hd: int) -> bool:
    return hd in (64, 80) and 1 <= t <= LONG_ATTENTION_MAX_T


def _short_cls_importance_ok(t: int, hd: int) -> bool:
    return 2 <= t <= 320 and hd in (32, 64, 80)


def cls_importance_supported(t: int, hd: int) -> bool:
    return _short_cls_importance_ok(t, hd) or (t >= 2 and _long_attention_ok(t, hd))


def cls_importance(qkv: torch.Tensor, heads: int, head_dim: int, scale: float) -> torch.Tensor:
    """qkv [B, T, 3 * heads * head_dim] bf16 (CLS token first) -> head-averaged CLS attention [B, T-1] fp32."""
    _need_cuda(qkv)
    assert qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 3 * heads * head_dim
    qkv = qkv.contiguous()
    b, t = qkv.shape[0], qkv.shape[1]
    if not _short_cls_importance_ok(t, head_dim):
        imp = torch.empty(b, heads, t - 1, dtype=torch.float32, device=qkv.device)
        _check(lib().basd_attention_fwd_long_bf16(_ptr(qkv), b, t, heads, head_dim, ctypes.c_float(scale), _ptr(None),
                                                  _ptr(imp), _ptr(None), _ptr(None), _stream()),
               "basd_attention_fwd_long_bf16")
        return imp.sum(dim=1)
    out = torch.empty(b, t - 1, dtype=torch.float32, device=qkv.device)
    _check(lib().basd_cls_importance_bf16(_ptr(qkv), b, t, heads, head_dim, ctypes.c_float(scale), _ptr(out), _stream()),
           "basd_cls_importance_bf16")
    return out


def _short_attention_fwd_ok(t: int, hd: int) -> bool:
    return hd in (64, 80) and 1 <= t <= 272


def attention_fwd_supported(t: int, hd: int) -> bool:
    return _short_attention_fwd_ok(t, hd) or _long_attention_ok(t, hd)


def attention_fwd_f32x3_supported(t: int, hd: int) -> bool:
    """the range of the single-pass fp32 split-bf16 evaluation attention (``basd_attention_fwd_f32x3``)"""
    return _short_attention_fwd_ok(t, hd)


def attention_fwd_f32x3_long_supported(t: int, hd: int) -> bool:
    """the range of the tiled one (``basd_attention_fwd_f32x3_long``), which ``attention_fwd_f32x3`` calls past the
    short kernel's"""
    return hd in (64, 80) and 1 <= t <= 1024


def attention_fwd(qkv: torch.Tensor, heads: int, head_dim: int, scale: float, want_importance: bool = False,
                  want_lse: bool = False, query_mean: bool = False):
    """qkv [B, T, 3 * heads * head_dim] bf16 -> (out [B, T, heads * head_dim] bf16, importance | None) and, with
    ``want_lse``, additionally the log-sum-exp [B, heads, T] fp32 the backward kernel needs.  importance: the CLS row of
    the head-averaged attention map without its first entry, [B, T-1] fp32 -- or, with ``query_mean`` (teachers without a
    CLS token), that map averaged over the queries, [B, T].  No autograd here (the student wraps forward +
    ``attention_bwd`` in an autograd.Function)."""
    _need_cuda(qkv)
    assert qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 3 * heads * head_dim
    qkv = qkv.contiguous()
    b, t = qkv.shape[0], qkv.shape[1]
    out = torch.empty(b, t, heads * head_dim, dtype=torch.bfloat16, device=qkv.device)
    if not _short_attention_fwd_ok(t, head_dim):
        return _attention_fwd_long(qkv, out, heads, head_dim, scale, want_importance, want_lse, query_mean)
    if want_importance and query_mean:
        assert not want_lse
        imp = torch.empty(b, heads, t, dtype=torch.float32, device=qkv.device)
        _check(lib().basd_attention_fwd_qmean_bf16(_ptr(qkv), b, t, heads, head_dim, ctypes.c_float(scale), _ptr(out),
                                                   _ptr(imp), _stream()), "basd_attention_fwd_qmean_bf16")
        return out, imp.sum(dim=1)
    imp = torch.empty(b, heads, t - 1, dtype=torch.float32, device=qkv.device) if want_importance else None
    lse = torch.empty(b, heads, t, dtype=torch.float32, device=qkv.device) if want_lse else None
    _check(lib().basd_attention_fwd_bf16(_ptr(qkv), b, t, heads, head_dim, ctypes.c_float(scale), _ptr(out), _ptr(imp),
                                         _ptr(lse), _stream()), "basd_attention_fwd_bf16")
    imp = imp.sum(dim=1) if want_importance else None
    return (out, imp, lse) if want_lse else (out, imp)


def _attention_fwd_long(qkv, out, heads, head_dim, scale, want_importance, want_lse, query_mean):
    b, t = qkv.shape[0], qkv.shape[1]
    cls = qm = None
    if want_importance and query_mean:
        assert not want_lse
        qm = torch.empty(b, heads, t, dtype=torch.float32, device=qkv.device)
    elif want_importance:
        cls = torch.empty(b, heads, t - 1, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(b, heads, t, dtype=torch.float32, device=qkv.device) if (want_lse or qm is not None) else None
    _check(lib().basd_attention_fwd_long_bf16(_ptr(qkv), b, t, heads, head_dim, ctypes.c_float(scale), _ptr(out),
                                              _ptr(cls), _ptr(qm), _ptr(lse), _stream()), "basd_attention_fwd_long_bf16")
    if qm is not None:
        return out, qm.sum(dim=1)
    imp = cls.sum(dim=1) if cls is not None else None
    return (out, imp, lse) if want_lse else (out, imp)


def relbias_index(i: int, j: int, gh: int, gw: int) -> int:
    """Row of BEiT's ``relative_position_bias_table`` ([(2 gh - 1)(2 gw - 1) + 3, H]) that biases the logit of query
    token i and key token j (token 0 = CLS, patch p at (y, x) = ((p - 1) // gw, (p - 1) % gw)): the closed form the
    kernel of ``attention_fwd_relbias`` evaluates per logit (csrc/attention.hip, RELBIAS).  Written from memory of
    timm's ``beit.py`` (``gen_relative_position_index``), without timm at hand: check it against the
    ``relative_position_index`` buffer of the installed timm before loading real weights."""
    rows = (2 * gh - 1) * (2 * gw - 1) + 3
    if i == 0:
        return rows - 1 if j == 0 else rows - 3
    if j == 0:
        return rows - 2
    yi, xi = divmod(i - 1, gw)
    yj, xj = divmod(j - 1, gw)
    return (yi - yj + gh - 1) * (2 * gw - 1) + (xi - xj + gw - 1)


def _attention_fwd_table(entry: str, qkv, table, rows: tuple, align: int, dims: tuple, heads, head_dim, scale,
                         want_importance):
    """The body of the four entries that carry a position table (fp32, shape ``rows``, ``align``-byte aligned): checks,
    allocation, the call -- ``dims`` are the entry's integers between B and heads, (gh, gw) or (T,) -- and the head sum
    of the tap.  -> (out [B, T, heads * head_dim] bf16, importance [B, T-1] fp32 | None)"""
    _need_cuda(qkv, table)
    b, t = qkv.shape[0], qkv.shape[1]
    assert qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 3 * heads * head_dim
    assert table.dtype == torch.float32 and tuple(table.shape) == rows, (tuple(table.shape), rows)
    qkv, table = qkv.contiguous(), table.contiguous()
    assert table.data_ptr() % align == 0
    out = torch.empty(b, t, heads * head_dim, dtype=torch.bfloat16, device=qkv.device)
    imp = torch.empty(b, heads, t - 1, dtype=torch.float32, device=qkv.device) if want_importance else None
    _check(getattr(lib(), entry)(_ptr(qkv), _ptr(table), b, *dims, heads, head_dim, ctypes.c_float(scale), _ptr(out),
                                 _ptr(imp), _stream()), entry)
    return out, (imp.sum(dim=1) if want_importance else None)


def attention_fwd_relbias_supported(gh: int, gw: int, hd: int) -> bool:
    """the range of ``basd_attention_fwd_relbias_bf16``: the short kernel's token count, head dim 64"""
    return hd == 64 and gh >= 1 and gw >= 1 and gh * gw + 1 <= 272


def attention_fwd_relbias(qkv: torch.Tensor, table: torch.Tensor, gh: int, gw: int, heads: int, head_dim: int,
                          scale: float, want_importance: bool = False):
    """qkv [B, gh * gw + 1, 3 * heads * head_dim] bf16 (CLS token first), table [(2 gh - 1)(2 gw - 1) + 3, heads] fp32
    (timm's ``relative_position_bias_table``) -> (out [B, T, heads * head_dim] bf16, importance | None) with
    softmax(q k^T * scale + table[relbias_index(i, j)]) per head; importance: the CLS row of the head-averaged biased
    map without its first entry, [B, T-1] fp32.  The bias is gathered inside the kernel: nothing [T, T] is built."""
    assert qkv.shape[1] == gh * gw + 1
    return _attention_fwd_table("basd_attention_fwd_relbias_bf16", qkv, table, ((2 * gh - 1) * (2 * gw - 1) + 3, heads), 4,
                                (gh, gw), heads, head_dim, scale, want_importance)


def attention_fwd_long_relbias_supported(gh: int, gw: int, hd: int) -> bool:
    """the range of ``basd_attention_fwd_long_relbias_bf16``: the tiled kernel's token count from 2 up, head dim 64"""
    return hd == 64 and gh >= 1 and gw >= 1 and gh * gw + 1 <= LONG_ATTENTION_MAX_T


def attention_fwd_long_relbias(qkv: torch.Tensor, table: torch.Tensor, gh: int, gw: int, heads: int, head_dim: int,
                               scale: float, want_importance: bool = False):
    """``attention_fwd_relbias`` on the tiled kernels (csrc/attention_long.hip, RELBIAS), for the token counts the short
    entry refuses; arguments and results are the same.  The importance is the CLS tap of ``attention_fwd``'s long kernel
    (bf16-rounded logits) with the CLS row's bias added to the scaled logits."""
    assert qkv.shape[1] == gh * gw + 1
    return _attention_fwd_table("basd_attention_fwd_long_relbias_bf16", qkv, table, ((2 * gh - 1) * (2 * gw - 1) + 3, heads), 4,
                                (gh, gw), heads, head_dim, scale, want_importance)


def rope_table(gh: int, gw: int, head_dim: int, *, ref_grid=None, temperature: float = 10000.0,
               prefix_tokens: int = 1) -> torch.Tensor:
    """fp32 [prefix_tokens + gh * gw, head_dim / 2, 2] on the CPU: (cos, sin) of the angle that rotates channel pair
    (2i, 2i + 1) of every token -- the table ``attention_fwd_rope`` reads; angles in fp64.  The rule is timm's
    ``RotaryEmbeddingCat`` with ``in_pixels=False`` (EVA-02), written from memory of timm 1.0.x ``pos_embed_sincos.py``
    without timm at hand: bands b_j = temperature^(-j / (hd / 4)), j = 0 .. hd / 4 - 1; coordinates y = arange(gh) *
    (ref_gh / gh), x likewise (plain arange when ``ref_grid`` is None or the grid itself); the hd / 2 angles of patch
    (y, x) are [y b_0 .. y b_last, x b_0 .. x b_last].  The prefix rows (CLS) are (1, 0): not rotated.  Check against
    the ``rope`` buffers of the installed timm before loading real weights."""
    if head_dim % 4 != 0 or gh < 1 or gw < 1 or prefix_tokens < 0:
        raise ValueError(f"rope_table: grid {gh} x {gw}, head_dim {head_dim} (a multiple of 4), prefix {prefix_tokens}")
    nb = head_dim // 4
    bands = float(temperature) ** (-torch.arange(nb, dtype=torch.float64) / nb)
    ref_gh, ref_gw = (gh, gw) if ref_grid is None else (int(ref_grid[0]), int(ref_grid[1]))
    y = torch.arange(gh, dtype=torch.float64) * (ref_gh / gh)
    x = torch.arange(gw, dtype=torch.float64) * (ref_gw / gw)
    ang = torch.cat([(y[:, None, None] * bands).expand(gh, gw, nb), (x[None, :, None] * bands).expand(gh, gw, nb)], dim=-1)
    table = torch.zeros(prefix_tokens + gh * gw, 2 * nb, 2, dtype=torch.float64)
    table[:prefix_tokens, :, 0] = 1.0
    table[prefix_tokens:, :, 0] = ang.reshape(gh * gw, 2 * nb).cos()
    table[prefix_tokens:, :, 1] = ang.reshape(gh * gw, 2 * nb).sin()
    return table.float()


def attention_fwd_rope_supported(t: int, hd: int) -> bool:
    """the range of ``basd_attention_fwd_rope_bf16``: the short kernel's token count from 2 up, head dim 64"""
    return hd == 64 and 2 <= t <= 272


def attention_fwd_rope(qkv: torch.Tensor, rope: torch.Tensor, heads: int, head_dim: int, scale: float,
                       want_importance: bool = False):
    """qkv [B, T, 3 * heads * head_dim] bf16, rope [T, head_dim / 2, 2] fp32 ((cos, sin) per token and channel pair:
    ``rope_table``) -> (out [B, T, heads * head_dim] bf16, importance | None) with softmax(q' k'^T * scale) v per head,
    q' / k' the pairwise rotations of q / k (fp32 arithmetic, one rounding to bf16) done inside the kernel; importance:
    the CLS row of the head-averaged map of that softmax without its first entry, [B, T-1] fp32."""
    t = qkv.shape[1]
    return _attention_fwd_table("basd_attention_fwd_rope_bf16", qkv, rope, (t, head_dim // 2, 2), 16, (t,), heads, head_dim,
                                scale, want_importance)


def attention_fwd_long_rope_supported(t: int, hd: int) -> bool:
    """the range of ``basd_attention_fwd_long_rope_bf16``: the tiled kernel's token count from 2 up, head dim 64"""
    return hd == 64 and 2 <= t <= LONG_ATTENTION_MAX_T


def attention_fwd_long_rope(qkv: torch.Tensor, rope: torch.Tensor, heads: int, head_dim: int, scale: float,
                            want_importance: bool = False):
    """``attention_fwd_rope`` on the tiled kernels (csrc/attention_long.hip, ROPE), for the token counts the short entry
    refuses; arguments and results are the same.  The importance is the CLS tap of ``attention_fwd``'s long kernel
    (bf16-rounded logits) on the rotated operands."""
    t = qkv.shape[1]
    return _attention_fwd_table("basd_attention_fwd_long_rope_bf16", qkv, rope, (t, head_dim // 2, 2), 16, (t,), heads, head_dim,
                                scale, want_importance)


def dinov3_rope_table(gh: int, gw: int, head_dim: int, base: float = 100.0, prefix_tokens: int = 5) -> torch.Tensor:
    """fp32 [prefix_tokens + gh * gw, head_dim / 2, 2] on the CPU: (cos, sin) of DINOv3's rotary angles, one per channel
    pair, in the layout ``attention_fwd_rope`` / ``attention_fwd_long_rope`` read; angles in fp64.  The rule is
    ``RopePositionEmbedding`` of facebookresearch/dinov3 (``base`` given, coordinates normalised "separate", no
    augmentation), written from memory without the hub code or timm at hand: periods p_j = base^(2 j / (hd / 2)),
    j = 0 .. hd / 4 - 1; coordinates y = (arange(gh) + 0.5) / gh * 2 - 1 in [-1, 1], x likewise; the hd / 2 angles of
    patch (y, x) are [2 pi y / p_0 .. 2 pi y / p_last, 2 pi x / p_0 .. 2 pi x / p_last].  DINOv3 tiles these hd / 2
    angles twice over the hd channels and rotates the half-split pairs (i, i + hd / 2): angle i belongs to that pair,
    which ``models/dinov3.py`` moves to the channels (2 i, 2 i + 1) in the weights.  The prefix rows (CLS and the
    registers) are (1, 0): not rotated.  Check against the checkpoint's ``rope_embed.periods`` before loading real
    weights."""
    if head_dim % 4 != 0 or gh < 1 or gw < 1 or prefix_tokens < 0:
        raise ValueError(f"dinov3_rope_table: grid {gh} x {gw}, head_dim {head_dim} (a multiple of 4), prefix "
                         f"{prefix_tokens}")
    nb = head_dim // 4
    periods = float(base) ** (2.0 * torch.arange(nb, dtype=torch.float64) / (head_dim // 2))
    y = (torch.arange(gh, dtype=torch.float64) + 0.5) / gh * 2.0 - 1.0
    x = (torch.arange(gw, dtype=torch.float64) + 0.5) / gw * 2.0 - 1.0
    two_pi = 2.0 * math.pi
    ang = torch.cat([(two_pi * y[:, None, None] / periods).expand(gh, gw, nb),
                     (two_pi * x[None, :, None] / periods).expand(gh, gw, nb)], dim=-1).reshape(gh * gw, 2 * nb)
    table = torch.zeros(prefix_tokens + gh * gw, 2 * nb, 2, dtype=torch.float64)
    table[:prefix_tokens, :, 0] = 1.0
    table[prefix_tokens:, :, 0] = ang.cos()
    table[prefix_tokens:, :, 1] = ang.sin()
    return table.float()


def _short_attention_bwd_ok(t: int, hd: int) -> bool:
    return hd == 64 and 1 <= t <= 224


def attention_bwd_supported(t: int, hd: int) -> bool:
    return _short_attention_bwd_ok(t, hd) or _long_attention_ok(t, hd)


def attention_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, heads: int,
                  head_dim: int, scale: float) -> torch.Tensor:
    """-> dqkv [B, T, 3 * heads * head_dim] bf16 (gradient of the packed projection)."""
    _need_cuda(qkv, out, dout, lse)
    b, t = qkv.shape[0], qkv.shape[1]
    assert qkv.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert qkv.is_contiguous() and out.is_contiguous() and lse.is_contiguous() and lse.shape == (b, heads, t)
    dout = dout.to(torch.bfloat16).contiguous()
    dqkv = torch.empty_like(qkv)
    if not _short_attention_bwd_ok(t, head_dim):
        need = int(lib().basd_attention_bwd_long_workspace_bytes(b, t, heads, head_dim))
        rec = _scratch("attention_bwd_long", qkv.device, need)
        _check(lib().basd_attention_bwd_long_bf16(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), b, t, heads, head_dim,
                                                  ctypes.c_float(scale), _ptr(dqkv), _ptr(rec.buf),
                                                  ctypes.c_int64(rec.buf.numel()), _stream()),
               "basd_attention_bwd_long_bf16")
        _scratch_used(rec)
        return dqkv
    _check(lib().basd_attention_bwd_bf16(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), b, t, heads, head_dim,
                                         ctypes.c_float(scale), _ptr(dqkv), _stream()), "basd_attention_bwd_bf16")
    return dqkv


def layernorm_supported(d: int) -> bool:
    return d % 8 == 0 and 8 <= d <= 2048


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """x [..., D] bf16 contiguous, gamma/beta fp32 -> (y bf16, mean [rows] fp32, rstd [rows] fp32)."""
    _need_cuda(x, gamma, beta)
    assert x.dtype == torch.bfloat16 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    x = x.contiguous()
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _check(lib().basd_layernorm_fwd_bf16(_ptr(x), _ptr(gamma.contiguous()), _ptr(beta.contiguous()), ctypes.c_int64(rows),
                                         d, ctypes.c_float(eps), _ptr(y), _ptr(mean), _ptr(rstd), _stream()),
           "basd_layernorm_fwd_bf16")
    return y, mean, rstd


def vit_embed_supported(d: int) -> bool:
    return layernorm_supported(d)


def vit_embed(patches: torch.Tensor, cls: torch.Tensor | None, pos: torch.Tensor, gamma: torch.Tensor | None = None,
              beta: torch.Tensor | None = None, eps: float = 1e-5, reg: torch.Tensor | None = None) -> torch.Tensor:
    """patches [B, N, D], cls [D] (any shape with D elements) | None, pos [T, D] (or [1, T, D]), T = N + (cls given),
    all bf16 -> [B, T, D] bf16: the rows ``src + pos`` rounded to bf16 (torch's cat + add), layer-normalised when
    gamma / beta (fp32 [D]) are given.  One launch (basd_vit_embed_bf16).  ``reg`` [R, D] (or [1, R, D]): R register
    rows behind the CLS row, without a position row -> [B, T + R, D] (basd_vit_embed_reg_bf16)."""
    if reg is not None:
        return _vit_embed_reg(patches, cls, reg, pos, gamma, beta, eps)
    _need_cuda(patches, cls, pos, gamma, beta)
    assert patches.dtype == torch.bfloat16 and pos.dtype == torch.bfloat16 and patches.dim() == 3
    assert cls is None or cls.dtype == torch.bfloat16
    assert (gamma is None) == (beta is None)
    assert gamma is None or (gamma.dtype == torch.float32 and beta.dtype == torch.float32)
    b, n, d = patches.shape
    t = n + (cls is not None)
    assert pos.numel() == t * d and (cls is None or cls.numel() == d), (tuple(pos.shape), t, d)
    assert gamma is None or (gamma.numel() == d and beta.numel() == d)
    patches, pos = patches.contiguous(), pos.contiguous()
    out = torch.empty(b, t, d, dtype=torch.bfloat16, device=patches.device)
    _check(lib().basd_vit_embed_bf16(_ptr(patches), _ptr(None if cls is None else cls.contiguous()), _ptr(pos),
                                     _ptr(None if gamma is None else gamma.contiguous()),
                                     _ptr(None if beta is None else beta.contiguous()), ctypes.c_float(eps), b, n, d,
                                     _ptr(out), _stream()), "basd_vit_embed_bf16")
    return out


def _vit_embed_reg(patches, cls, reg, pos, gamma, beta, eps):
    _need_cuda(patches, cls, reg, pos, gamma, beta)
    assert patches.dtype == torch.bfloat16 and pos.dtype == torch.bfloat16 and patches.dim() == 3
    assert cls is not None and cls.dtype == torch.bfloat16 and reg.dtype == torch.bfloat16
    assert (gamma is None) == (beta is None)
    assert gamma is None or (gamma.dtype == torch.float32 and beta.dtype == torch.float32)
    b, n, d = patches.shape
    r = reg.numel() // d
    assert reg.numel() == r * d and pos.numel() == (n + 1) * d and cls.numel() == d, (tuple(reg.shape), tuple(pos.shape), n, d)
    assert gamma is None or (gamma.numel() == d and beta.numel() == d)
    patches, pos = patches.contiguous(), pos.contiguous()
    out = torch.empty(b, 1 + r + n, d, dtype=torch.bfloat16, device=patches.device)
    _check(lib().basd_vit_embed_reg_bf16(_ptr(patches), _ptr(cls.contiguous()), _ptr(reg.contiguous()), r, _ptr(pos),
                                         _ptr(None if gamma is None else gamma.contiguous()),
                                         _ptr(None if beta is None else beta.contiguous()), ctypes.c_float(eps), b, n, d,
                                         _ptr(out), _stream()), "basd_vit_embed_reg_bf16")
    return out


def add_layernorm_fwd(x: torch.Tensor, residual: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                      row_scale: torch.Tensor | None = None, want_stats: bool = False):
    """s = bf16(residual + row_scale[sample] * x) and y = LayerNorm(s): -> (s, y) or, with ``want_stats`` (a trained
    block: backward needs them), (s, y, mean, rstd).  ``row_scale`` fp32 [B] for x [B, T, D] (stochastic depth)."""
    _need_cuda(x, residual, gamma, beta)
    assert x.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16 and x.shape == residual.shape
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32
    x, residual = x.contiguous(), residual.contiguous()
    d = x.shape[-1]
    rows = x.numel() // d
    s = torch.empty_like(x)
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if want_stats else None
    rps = 1
    if row_scale is not None:
        row_scale = row_scale.contiguous().float()
        assert rows % row_scale.numel() == 0
        rps = rows // row_scale.numel()
    _check(lib().basd_add_layernorm_fwd_bf16(_ptr(x), _ptr(residual), _ptr(gamma.contiguous()), _ptr(beta.contiguous()),
                                             ctypes.c_int64(rows), d, ctypes.c_float(eps), _ptr(s), _ptr(y), _ptr(mean),
                                             _ptr(rstd), _ptr(row_scale), rps, _stream()), "basd_add_layernorm_fwd_bf16")
    return (s, y, mean, rstd) if want_stats else (s, y)


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                  dgamma: torch.Tensor | None, dbeta: torch.Tensor | None, dres: torch.Tensor | None = None,
                  row_scale: torch.Tensor | None = None, want_branch: bool = False):
    """-> dx bf16 (= LayerNorm backward + ``dres``); with ``want_branch`` -> (dx, row_scale[sample] * dx).
    dgamma / dbeta (fp32, may be None together) are accumulated into."""
    _need_cuda(dy, x, gamma)
    dy = dy.contiguous()
    d = x.shape[-1]
    rows = x.numel() // d
    dx = torch.empty_like(x)
    dbranch = torch.empty_like(x) if want_branch else None
    rps = 1
    if dres is not None:
        dres = dres.to(torch.bfloat16).contiguous()
    if row_scale is not None:
        row_scale = row_scale.contiguous().float()
        rps = rows // row_scale.numel()
    _check(lib().basd_layernorm_bwd_bf16(_ptr(dy), _ptr(x), _ptr(gamma.contiguous()), _ptr(mean), _ptr(rstd),
                                         ctypes.c_int64(rows), d, _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(dres),
                                         _ptr(dbranch), _ptr(row_scale), rps, _stream()), "basd_layernorm_bwd_bf16")
    return (dx, dbranch) if want_branch else dx


# ---- fp32 evaluation forward on split-bf16 (bf16x3) products: torch.set_float32_matmul_precision("high") --------------
# A split image of fp32 values [rows, k] is bf16 [rows, 2 k_pad]: (hi | lo), zero columns up to k_pad (include/basd_hip.h).

def f32x3_gemm_supported(n: int, k_pad: int) -> bool:
    return n >= 16 and n % 16 == 0 and k_pad >= 32 and k_pad % 32 == 0


def f32x3_layernorm_supported(d: int) -> bool:
    return d % 4 == 0 and 4 <= d <= 2048


def split_table(entries) -> list[torch.Tensor]:
    """entries: list of (fp32 matrix [rows, k] (any contiguous view), k_pad) -> their images [rows, 2 k_pad] bf16, carved
    from ONE allocation and written by one launch (per 64 entries)."""
    if not entries:
        return []
    dev = entries[0][0].device
    sizes = [w.shape[0] * 2 * kp for w, kp in entries]
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 7) // 8 * 8                       # 16-byte aligned images
    buf = torch.empty(total, dtype=torch.bfloat16, device=dev)
    flat, out = [], []
    for (w, kp), off, n in zip(entries, offs, sizes):
        _need_cuda(w)
        assert w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and kp >= w.shape[1] and w.device == dev
        img = buf[off:off + n].view(w.shape[0], 2 * kp)
        out.append(img)
        flat += [w.data_ptr(), img.data_ptr(), w.shape[0], w.shape[1], kp]
    arr = (ctypes.c_int64 * len(flat))(*[int(v) for v in flat])
    _check(lib().basd_split_bf16x2_table(ctypes.cast(arr, ctypes.c_void_p), len(entries), _stream()),
           "basd_split_bf16x2_table")
    return out


def split_patches(x: torch.Tensor, patch: int, k_pad: int) -> torch.Tensor:
    """x [B, C, H, W] fp32 -> image [B (H/p) (W/p), 2 k_pad] of the unfolded non-overlapping patches."""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    b, c, h, w = x.shape
    out = torch.empty(b * (h // patch) * (w // patch), 2 * k_pad, dtype=torch.bfloat16, device=x.device)
    _check(lib().basd_split_patches_bf16x2(_ptr(x), b, c, h, w, patch, k_pad, _ptr(out), _stream()),
           "basd_split_patches_bf16x2")
    return out


def gemm_f32x3(x_img: torch.Tensor, w_img: torch.Tensor, bias: torch.Tensor | None = None, gelu: bool = False,
               split_out: bool = False) -> torch.Tensor:
    """x_img [M, 2 k_pad], w_img [N, 2 k_pad] (images), bias fp32 [N] -> epi(x w^T + bias): fp32 [M, N] or, with
    ``split_out``, its image [M, 2 N]."""
    _need_cuda(x_img, w_img)
    assert x_img.dtype == torch.bfloat16 and w_img.dtype == torch.bfloat16
    assert x_img.is_contiguous() and w_img.is_contiguous() and x_img.shape[-1] == w_img.shape[-1]
    m, n, kp = x_img.shape[0], w_img.shape[0], w_img.shape[1] // 2
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == n
        bias = bias.contiguous()
    y = (torch.empty(m, 2 * n, dtype=torch.bfloat16, device=x_img.device) if split_out
         else torch.empty(m, n, dtype=torch.float32, device=x_img.device))
    _check(lib().basd_gemm_f32x3(_ptr(x_img), _ptr(w_img), _ptr(bias), _ptr(y), ctypes.c_int64(m), n, kp,
                                 int(gelu) + 2 * int(split_out), _stream()), "basd_gemm_f32x3")
    return y


def attention_fwd_f32x3(qkv: torch.Tensor, heads: int, head_dim: int, scale: float) -> torch.Tensor:
    """qkv [B, T, 3 * heads * head_dim] fp32 -> the image [B T, 2 heads head_dim] of softmax(q k^T scale) v."""
    _need_cuda(qkv)
    assert qkv.dtype == torch.float32 and qkv.shape[-1] == 3 * heads * head_dim
    qkv = qkv.contiguous()
    b, t = qkv.shape[0], qkv.shape[1]
    out = torch.empty(b * t, 2 * heads * head_dim, dtype=torch.bfloat16, device=qkv.device)
    name = "basd_attention_fwd_f32x3" if _short_attention_fwd_ok(t, head_dim) else "basd_attention_fwd_f32x3_long"
    _check(getattr(lib(), name)(_ptr(qkv), b, t, heads, head_dim, ctypes.c_float(scale), _ptr(out), _stream()), name)
    return out


def add_layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                      residual: torch.Tensor | None = None, xscale: torch.Tensor | None = None, want_s: bool = False,
                      want_y: bool = False, want_img: bool = True):
    """s = residual + xscale * x (no residual: s = x), y = LayerNorm(s), all fp32 -> tuple of the requested outputs in
    the order (s [..., D] fp32, y [..., D] fp32, image [rows, 2 D] bf16)."""
    _need_cuda(x, gamma, beta)
    assert x.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    x = x.contiguous()
    d = x.shape[-1]
    rows = x.numel() // d
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == x.shape
        residual = residual.contiguous()
    if xscale is not None:
        xscale = xscale.detach().float().contiguous()
        assert xscale.numel() == d
    s = torch.empty_like(x) if want_s else None
    y = torch.empty_like(x) if want_y else None
    img = torch.empty(rows, 2 * d, dtype=torch.bfloat16, device=x.device) if want_img else None
    _check(lib().basd_add_layernorm_fwd_f32(_ptr(x), _ptr(residual), _ptr(xscale), _ptr(gamma.contiguous()),
                                            _ptr(beta.contiguous()), ctypes.c_int64(rows), d, ctypes.c_float(eps),
                                            _ptr(s), _ptr(y), _ptr(img), _stream()), "basd_add_layernorm_fwd_f32")
    return tuple(t for t in (s, y, img) if t is not None)


# --------------------------------------------------------------------------- ConvNeXt-V2 teacher trunk (csrc/convnext.hip)
def dwconv7_ln_supported(c: int, ld_in: int, ld_out: int) -> bool:
    return (c % 8 == 0 and 8 <= c <= 2048 and ld_in % 8 == 0 and ld_out % 8 == 0 and c <= ld_in
            and c <= ld_out <= 2 * c)


def dwconv7_ln(x: torch.Tensor, w49: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               eps: float, ld_out: int | None = None) -> torch.Tensor:
    """x [B, H, W, ld_in] bf16 channels-last rows (columns C .. ld_in zero), w49 [49, C] bf16 tap-major, bias / gamma /
    beta fp32 [C] -> LayerNorm_C(depthwise 7x7 (x) + bias) [B, H, W, ld_out] bf16, columns C .. ld_out zero."""
    _need_cuda(x, w49, bias, gamma, beta)
    assert x.dtype == torch.bfloat16 and w49.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
    assert bias.dtype == gamma.dtype == beta.dtype == torch.float32
    b, h, w, ld_in = x.shape
    c = w49.shape[1]
    ld_out = ld_in if ld_out is None else ld_out
    assert w49.shape == (49, c) and w49.is_contiguous() and dwconv7_ln_supported(c, ld_in, ld_out), (c, ld_in, ld_out)
    y = torch.empty(b, h, w, ld_out, dtype=torch.bfloat16, device=x.device)
    _check(lib().basd_dwconv7_ln_bf16(_ptr(x), _ptr(w49), _ptr(bias.contiguous()), _ptr(gamma.contiguous()),
                                      _ptr(beta.contiguous()), b, h, w, c, ld_in, ld_out, ctypes.c_float(eps), _ptr(y),
                                      _stream()), "basd_dwconv7_ln_bf16")
    return y


def grn_supported(c: int) -> bool:
    return c % 8 == 0 and 8 <= c <= 4096


def grn_(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """GRN of ConvNeXt-V2 IN PLACE on x [B, HW, C] bf16 contiguous; weight / bias fp32 [C].  Returns x."""
    _need_cuda(x, weight, bias)
    assert x.dtype == torch.bfloat16 and x.dim() == 3 and x.is_contiguous() and grn_supported(x.shape[2])
    assert weight.dtype == torch.float32 and bias.dtype == torch.float32
    b, hw, c = x.shape
    need = int(lib().basd_grn_workspace_bytes(b, hw, c))
    rec = _scratch("grn", x.device, need)
    _check(lib().basd_grn_bf16(_ptr(x), _ptr(weight.contiguous()), _ptr(bias.contiguous()), b, hw, c, ctypes.c_float(eps),
                               _ptr(rec.buf), ctypes.c_int64(rec.buf.numel()), _stream()), "basd_grn_bf16")
    _scratch_used(rec)
    return x


def patchify(x: torch.Tensor, p: int, k_pad: int) -> torch.Tensor:
    """x [B, C, H, W] bf16 in any strides (NCHW, channels-last, or the NCHW view of padded channels-last rows) ->
    [B (H/p) (W/p), k_pad] bf16 rows with column (i p + j) C + c = x[b, c, oh p + i, ow p + j], zero behind C p p."""
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 4
    b, c, h, w = x.shape
    assert h % p == 0 and w % p == 0 and k_pad % 8 == 0 and k_pad >= c * p * p, (tuple(x.shape), p, k_pad)
    out = torch.empty(b * (h // p) * (w // p), k_pad, dtype=torch.bfloat16, device=x.device)
    sb, sc, sh, sw = x.stride()
    _check(lib().basd_patchify_bf16(_ptr(x), b, c, h, w, ctypes.c_int64(sb), ctypes.c_int64(sc), ctypes.c_int64(sh),
                                    ctypes.c_int64(sw), p, k_pad, _ptr(out), _stream()), "basd_patchify_bf16")
    return out


# --------------------------------------------------------------------------- ResNet teacher trunk (csrc/resnet.hip)
STEM_K_PAD = 160          # 7 x 7 x 3 = 147 columns of the stem's weight image, padded to whole k-blocks of 32


def conv3x3_supported(c: int, ld_in: int, ld_out: int, stride: int = 1) -> bool:
    return (c % 64 == 0 and 64 <= c <= 512 and stride in (1, 2) and ld_in % 8 == 0 and ld_out % 8 == 0 and c <= ld_in
            and c <= ld_out <= 2 * c)


def conv3x3(x: torch.Tensor, w9: torch.Tensor, bias: torch.Tensor, stride: int = 1, relu_in: bool = False,
            relu_out: bool = False, ld_out: int | None = None) -> torch.Tensor:
    """x [B, H, W, ld_in] bf16 channels-last rows, w9 [C, 9 C] bf16 tap-major (column (dy 3 + dx) C + c), bias [C] bf16
    -> epi(conv3x3(in(x), padding 1, stride) + bias) [B, Ho, Wo, ld_out] bf16, columns C .. ld_out zero; in / epi =
    ReLU if ``relu_in`` / ``relu_out``."""
    _need_cuda(x, w9, bias)
    assert x.dtype == w9.dtype == bias.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
    b, h, w, ld_in = x.shape
    c = w9.shape[0]
    ld_out = ld_in if ld_out is None else ld_out
    if not (w9.shape == (c, 9 * c) and bias.shape == (c,) and conv3x3_supported(c, ld_in, ld_out, stride)):
        raise BasdNativeError(f"conv3x3: C={c} ld_in={ld_in} ld_out={ld_out} stride={stride} w9={tuple(w9.shape)} is "
                              "not tiled (C % 64 == 0, 64 <= C <= 512, C <= ld_out <= 2 C, stride 1 or 2)")
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    y = torch.empty(b, ho, wo, ld_out, dtype=torch.bfloat16, device=x.device)
    _check(lib().basd_conv3x3_bf16(_ptr(x), _ptr(w9.contiguous()), _ptr(bias.contiguous()), b, h, w, c, stride, ld_in,
                                   ld_out, int(relu_in), int(relu_out), _ptr(y), _stream()), "basd_conv3x3_bf16")
    return y


def conv7x7s2_relu_supported(ld_out: int) -> bool:
    return ld_out % 8 == 0 and 64 <= ld_out <= 128


def conv7x7s2_relu(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, ld_out: int = 128) -> torch.Tensor:
    """x [B, 3, H, W] bf16 in any strides, w [64, K_pad] bf16 with column (dy 7 + dx) 3 + c (zero behind 147), bias [64]
    bf16 -> relu(conv7x7(x, padding 3, stride 2) + bias) [B, H1, W1, ld_out] bf16, columns 64 .. ld_out zero."""
    _need_cuda(x, w, bias)
    assert x.dtype == w.dtype == bias.dtype == torch.bfloat16 and x.dim() == 4
    b, c, h, wd = x.shape
    if not (c == 3 and w.dim() == 2 and w.shape[0] == 64 and w.shape[1] >= STEM_K_PAD and w.shape[1] % 8 == 0
            and bias.shape == (64,) and conv7x7s2_relu_supported(ld_out)):
        raise BasdNativeError(f"conv7x7s2_relu: x={tuple(x.shape)} w={tuple(w.shape)} ld_out={ld_out} is not tiled "
                              f"(3 input channels, w [64, K_pad >= {STEM_K_PAD}], 64 <= ld_out <= 128)")
    y = torch.empty(b, (h - 1) // 2 + 1, (wd - 1) // 2 + 1, ld_out, dtype=torch.bfloat16, device=x.device)
    sb, sc, sh, sw = x.stride()
    _check(lib().basd_conv7x7s2_relu_bf16(_ptr(x), _ptr(w.contiguous()), _ptr(bias.contiguous()), b, h, wd,
                                          ctypes.c_int64(sb), ctypes.c_int64(sc), ctypes.c_int64(sh), ctypes.c_int64(sw),
                                          w.shape[1], ld_out, _ptr(y), _stream()), "basd_conv7x7s2_relu_bf16")
    return y


def maxpool3x3s2_supported(c: int, ld_in: int, ld_out: int) -> bool:
    return c % 8 == 0 and c >= 8 and ld_in % 8 == 0 and ld_out % 8 == 0 and c <= ld_in and c <= ld_out


def maxpool3x3s2(x: torch.Tensor, c: int, ld_out: int | None = None) -> torch.Tensor:
    """x [B, H, W, ld_in] bf16 channels-last rows with c channels -> max_pool2d(3, stride 2, padding 1)
    [B, Ho, Wo, ld_out] bf16, columns c .. ld_out zero.  Exact."""
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
    b, h, w, ld_in = x.shape
    ld_out = ld_in if ld_out is None else ld_out
    if not maxpool3x3s2_supported(c, ld_in, ld_out):
        raise BasdNativeError(f"maxpool3x3s2: C={c} ld_in={ld_in} ld_out={ld_out} (multiples of 8, C <= ld)")
    y = torch.empty(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, ld_out, dtype=torch.bfloat16, device=x.device)
    _check(lib().basd_maxpool3x3s2_bf16(_ptr(x), b, h, w, c, ld_in, ld_out, _ptr(y), _stream()),
           "basd_maxpool3x3s2_bf16")
    return y


def add_relu_supported(c: int, ld_y: int, ld_r: int) -> bool:
    return c % 8 == 0 and c >= 8 and ld_y % 8 == 0 and ld_r % 8 == 0 and c <= ld_y and c <= ld_r


def add_relu_(y: torch.Tensor, r: torch.Tensor, c: int | None = None) -> torch.Tensor:
    """y <- bf16(max(0, y + r)) IN PLACE on the first c columns of the rows y [rows, ld_y], r [rows, ld_r] (bf16,
    contiguous; c defaults to the whole row).  Returns y."""
    _need_cuda(y, r)
    assert y.dtype == r.dtype == torch.bfloat16 and y.dim() == 2 and r.dim() == 2 and y.is_contiguous() and r.is_contiguous()
    assert y.shape[0] == r.shape[0]
    c = y.shape[1] if c is None else c
    if not add_relu_supported(c, y.shape[1], r.shape[1]):
        raise BasdNativeError(f"add_relu_: C={c} ld_y={y.shape[1]} ld_r={r.shape[1]} (multiples of 8, C <= ld)")
    _check(lib().basd_add_relu_bf16(_ptr(y), _ptr(r), ctypes.c_int64(y.shape[0]), c, y.shape[1], r.shape[1], _stream()),
           "basd_add_relu_bf16")
    return y


# --------------------------------------------------------------------------- Swin teacher trunk (csrc/swin.hip, csrc/swin_wide.hip)
WINDOW_SLOTS = 64          # slots of a window tile: ws <= 8; also the row / column count of a bias image
WINDOW_WIDE_MIN, WINDOW_WIDE_MAX = 9, 16      # windows of basd_window_attention_fwd_wide_bf16 (csrc/swin_wide.hip)
_WINDOW, _WINDOW_WIDE = (1, 8), (WINDOW_WIDE_MIN, WINDOW_WIDE_MAX)       # (lo, hi) of the two entries; 8^2 = WINDOW_SLOTS


def _window_supported(window, h: int, w: int, ws: int, shift: int, heads: int, c: int, ld_qkv: int, ld_out: int) -> bool:
    """the refusals of both entries (window_attention_check, csrc/window_attn.h) for the windows lo .. hi"""
    return (window[0] <= ws <= window[1] and 0 <= shift < ws and h >= ws and w >= ws and h % ws == 0 and w % ws == 0
            and heads >= 1 and c == 32 * heads and ld_qkv % 8 == 0 and ld_out % 8 == 0 and ld_qkv >= 3 * c and ld_out >= c)


def window_attention_supported(h: int, w: int, ws: int, shift: int, heads: int, c: int, ld_qkv: int, ld_out: int) -> bool:
    return _window_supported(_WINDOW, h, w, ws, shift, heads, c, ld_qkv, ld_out)


def window_attention_wide_supported(h: int, w: int, ws: int, shift: int, heads: int, c: int, ld_qkv: int,
                                    ld_out: int) -> bool:
    return _window_supported(_WINDOW_WIDE, h, w, ws, shift, heads, c, ld_qkv, ld_out)


def window_bias_image(bias: torch.Tensor) -> torch.Tensor:
    """bias [heads, ws^2, ws^2] (query slot, key slot) -> the image the kernel reads: fp32 [heads, 64, 64], zero behind
    ws^2 in both axes.  Built once per block of a frozen teacher."""
    heads, n, _ = bias.shape
    assert bias.shape == (heads, n, n) and n <= WINDOW_SLOTS
    img = torch.zeros(heads, WINDOW_SLOTS, WINDOW_SLOTS, dtype=torch.float32, device=bias.device)
    img[:, :n, :n] = bias.float()
    return img


def _window_attention(entry: str, window, qkv, bias, bias_shape, refusal: str, ws, shift, heads, scale, ld_out):
    """the body of both wrappers; ``window`` = (lo, hi), ``refusal`` the message with {call} and {shape} left open"""
    _need_cuda(qkv, bias)
    assert qkv.dtype == torch.bfloat16 and qkv.dim() == 4 and qkv.is_contiguous()
    assert bias.dtype == torch.float32 and bias.is_contiguous()
    b, h, w, ld_qkv = qkv.shape
    c = 32 * heads
    ld_out = c if ld_out is None else ld_out
    if not (_window_supported(window, h, w, ws, shift, heads, c, ld_qkv, ld_out) and bias.shape == bias_shape):
        raise BasdNativeError(refusal.format(call=f"grid {h}x{w} ws={ws} shift={shift} heads={heads} ld_qkv={ld_qkv} "
                                                  f"ld_out={ld_out}", shape=tuple(bias.shape)))
    out = torch.empty(b, h, w, ld_out, dtype=torch.bfloat16, device=qkv.device)
    _check(getattr(lib(), entry)(_ptr(qkv), _ptr(bias), b, h, w, heads, c, ws, shift, ld_qkv, ld_out, ctypes.c_float(scale),
                                 _ptr(out), _stream()), entry)
    return out


def window_attention(qkv: torch.Tensor, bias_img: torch.Tensor, ws: int, shift: int, heads: int, scale: float,
                     ld_out: int | None = None) -> torch.Tensor:
    """qkv [B, H, W, ld_qkv] bf16 rows (q | k | v in the first 3 C columns, each [heads, 32]), bias_img from
    ``window_bias_image`` -> (shifted-)window attention [B, H, W, ld_out] bf16, columns C .. ld_out zero.  Token
    (y, x) sits in slot ((y - shift) mod H, (x - shift) mod W) of the window partition; the mask of a shifted block is
    computed from the slot coordinates."""
    return _window_attention("basd_window_attention_fwd_bf16", _WINDOW, qkv, bias_img, (heads, WINDOW_SLOTS, WINDOW_SLOTS),
                             "window_attention: {call} bias={shape} is not tiled (ws <= 8, head dim 32, grid a multiple "
                             "of ws, bias image [heads, 64, 64])", ws, shift, heads, scale, ld_out)


def window_attention_wide(qkv: torch.Tensor, table: torch.Tensor, ws: int, shift: int, heads: int, scale: float,
                          ld_out: int | None = None) -> torch.Tensor:
    """``window_attention`` for windows 9 .. 16 (81 .. 256 slots; window 12 of the 384 px Swin checkpoints): the same
    rows, roll / partition arithmetic, mask and rounding points.  ``table`` is timm's ``relative_position_bias_table``
    itself, fp32 [(2 ws - 1)^2, heads]; the kernel computes the index per logit, no [N, N] image is built."""
    return _window_attention("basd_window_attention_fwd_wide_bf16", _WINDOW_WIDE, qkv, table, ((2 * ws - 1) ** 2, heads),
                             "window_attention_wide: {call} table={shape} is not tiled (9 <= ws <= 16, head dim 32, grid "
                             "a multiple of ws, bias table [(2 ws - 1)^2, heads])", ws, shift, heads, scale, ld_out)


def patch_merge_ln_supported(c: int, ld_in: int, h: int = 2, w: int = 2) -> bool:
    return c % 8 == 0 and 8 <= 4 * c <= 4096 and ld_in % 8 == 0 and c <= ld_in and h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0


def patch_merge_ln(x: torch.Tensor, c: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """x [B, H, W, ld_in] bf16 rows with c channels, gamma / beta fp32 [4 c] -> LayerNorm over the 4 c channels of
    concat(x[2r, 2c], x[2r+1, 2c], x[2r, 2c+1], x[2r+1, 2c+1]) [B, H/2, W/2, 4 c] bf16."""
    _need_cuda(x, gamma, beta)
    assert x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.shape == beta.shape == (4 * c,)
    b, h, w, ld_in = x.shape
    if not patch_merge_ln_supported(c, ld_in, h, w):
        raise BasdNativeError(f"patch_merge_ln: grid {h}x{w} C={c} ld_in={ld_in} is not tiled (even grid, C % 8 == 0, "
                              "4 C <= 4096)")
    y = torch.empty(b, h // 2, w // 2, 4 * c, dtype=torch.bfloat16, device=x.device)
    _check(lib().basd_patch_merge_ln_bf16(_ptr(x), _ptr(gamma.contiguous()), _ptr(beta.contiguous()), b, h, w, c, ld_in,
                                          ctypes.c_float(eps), _ptr(y), _stream()), "basd_patch_merge_ln_bf16")
    return y


# --------------------------------------------------------------------------- device-side dual views (csrc/dual_view.hip)
def dual_view_supported(image_size: int) -> bool:
    """output sizes basd_resample_u8 / basd_ta_normalize_u8 take (odd ones included)"""
    return 3 <= image_size <= 1024


def resample_u8(images: torch.Tensor, records: torch.Tensor, image_size: int) -> torch.Tensor:
    """images [B, 3, H, W] uint8, records [B, 9] int32 {top, left, h, w, nh, nw, off_y, off_x, flip} ->
    [B, 3, S, S] uint8: window -> antialiased bilinear resize to (nh, nw) -> S x S part at the offset -> flip."""
    _need_cuda(images, records)
    assert images.dtype == torch.uint8 and images.dim() == 4 and images.shape[1] == 3 and images.is_contiguous()
    b, _, h, w = images.shape
    assert records.dtype == torch.int32 and records.shape == (b, 9) and records.is_contiguous()
    assert dual_view_supported(image_size), image_size
    out = torch.empty(b, 3, image_size, image_size, dtype=torch.uint8, device=images.device)
    _check(lib().basd_resample_u8(_ptr(images), _ptr(records), b, h, w, image_size, _ptr(out), _stream()),
           "basd_resample_u8")
    return out


PACKED_BAND_ROWS = 16          # output rows per workgroup of basd_resample_u8_packed (PK_ROWS in csrc/dual_view.hip)


def resample_u8_packed(pixels: torch.Tensor, geometry: torch.Tensor, records: torch.Tensor, image_size: int) -> torch.Tensor:
    """pixels [N] uint8 (sample b: planar [3, h_b, w_b] from byte geometry[b, 0]), geometry [B, 3] int64 {offset, h, w},
    records [B, 9] int32 as for ``resample_u8`` with the sample's own size as the canvas -> [B, 3, S, S] uint8, per
    sample what ``resample_u8`` gives on it alone.  A sample that does not lie inside ``pixels`` comes out zero."""
    _need_cuda(pixels, geometry, records)
    assert pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.is_contiguous()
    b = geometry.shape[0]
    assert geometry.dtype == torch.int64 and geometry.shape == (b, 3) and geometry.is_contiguous()
    assert records.dtype == torch.int32 and records.shape == (b, 9) and records.is_contiguous()
    assert dual_view_supported(image_size), image_size
    out = torch.empty(b, 3, image_size, image_size, dtype=torch.uint8, device=pixels.device)
    _check(lib().basd_resample_u8_packed(_ptr(pixels), ctypes.c_int64(pixels.numel()), _ptr(geometry), _ptr(records), b,
                                         image_size, _ptr(out), _stream()), "basd_resample_u8_packed")
    return out


def ta_normalize_u8(images: torch.Tensor, ops: torch.Tensor | None, mags: torch.Tensor | None, mean, std) -> torch.Tensor:
    """images [B, 3, S, S] uint8, ops [B] int32 (index into TA_WIDE_OPS) and mags [B] fp64 (None, None: Identity), mean /
    std: three floats each -> ((op(image) / 255) - mean) / std as fp32 [B, 3, S, S]."""
    _need_cuda(images, ops, mags)
    assert images.dtype == torch.uint8 and images.dim() == 4 and images.shape[1] == 3 and images.is_contiguous()
    b, _, s, s2 = images.shape
    assert s == s2 and dual_view_supported(s), tuple(images.shape)
    assert (ops is None) == (mags is None) and len(mean) == 3 and len(std) == 3
    if ops is not None:
        assert ops.dtype == torch.int32 and ops.shape == (b,) and ops.is_contiguous()
        assert mags.dtype == torch.float64 and mags.shape == (b,) and mags.is_contiguous()
    out = torch.empty(b, 3, s, s, dtype=torch.float32, device=images.device)
    f = ctypes.c_float
    _check(lib().basd_ta_normalize_u8(_ptr(images), _ptr(ops), _ptr(mags), b, s, f(mean[0]), f(mean[1]), f(mean[2]),
                                      f(std[0]), f(std[1]), f(std[2]), _ptr(out), _stream()), "basd_ta_normalize_u8")
    return out


# --------------------------------------------------------------------------- evaluation tally (csrc/eval_tally.hip)
def cls_tally_supported(logits: torch.Tensor) -> bool:
    """logits basd_cls_tally reads in place: [B, C] fp32 / bf16 on the device, unit column stride, rows at least C
    elements apart (any padding behind a row is never read)"""
    return (logits.is_cuda and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16)
            and logits.shape[1] >= 1 and (logits.shape[1] == 1 or logits.stride(1) == 1)
            and (logits.shape[0] <= 1 or logits.stride(0) >= logits.shape[1]))


def cls_tally(logits: torch.Tensor, labels: torch.Tensor, tally: torch.Tensor, *, keep: torch.Tensor | None = None,
              top_k: int, smoothing: float = 0.0):
    """logits [B, C] fp32 / bf16 (read in place, any row stride >= C), labels [B] integer indices into the subset,
    keep: None | [K] int64 distinct columns, tally [4] fp64 = {hits@1, hits@top_k, summed loss, rows}, ADDED TO in place
    -> (row_rank [B] int32, row_loss [B] fp64); semantics in include/basd_hip.h.  No host sync."""
    _need_cuda(logits, labels, tally, keep)
    assert cls_tally_supported(logits), (tuple(logits.shape), logits.stride(), logits.dtype)
    b, c = logits.shape
    assert labels.shape == (b,) and not labels.dtype.is_floating_point, (tuple(labels.shape), labels.dtype)
    assert tally.dtype == torch.float64 and tally.shape == (4,) and tally.is_contiguous()
    labels = labels.to(torch.int64).contiguous()
    k = c
    if keep is not None:
        assert keep.dtype == torch.int64 and keep.dim() == 1 and keep.is_contiguous(), (keep.dtype, tuple(keep.shape))
        k = keep.shape[0]
    row_rank = torch.empty(b, dtype=torch.int32, device=logits.device)
    row_loss = torch.empty(b, dtype=torch.float64, device=logits.device)
    stride = logits.stride(0) if b > 1 else c
    _check(lib().basd_cls_tally(_ptr(logits), int(logits.dtype == torch.bfloat16), ctypes.c_int64(stride), _ptr(labels),
                                _ptr(keep), b, c, k, int(top_k), ctypes.c_float(smoothing), _ptr(row_rank),
                                _ptr(row_loss), _ptr(tally), _stream()), "basd_cls_tally")
    return row_rank, row_loss


# --------------------------------------------------------------------------- MixUp / CutMix + soft targets (csrc/mixup.hip)
MIXUP, CUTMIX = 0, 1


def mixup_supported(images: torch.Tensor) -> bool:
    """batches basd_mixup_cutmix takes: [B, C, H, W] fp32 / bf16, contiguous, on the device, at least one element"""
    return (images.is_cuda and images.dim() == 4 and images.dtype in (torch.float32, torch.bfloat16)
            and images.numel() > 0 and images.is_contiguous())


def mixup_cutmix(images: torch.Tensor, labels: torch.Tensor, num_classes: int, mode: int, lam: float, box,
                 out: torch.Tensor, out_targets: torch.Tensor):
    """images [B, C, H, W] fp32 / bf16, labels [B] int64, mode MIXUP | CUTMIX, lam the blend weight (MixUp) or the
    box-area-corrected weight of the targets (CutMix), box = (y0, y1, x0, x1) half-open and clipped (ignored for MixUp)
    -> out (like images, must not overlap them), out_targets [B, num_classes] fp32, both written in full by one launch;
    semantics in include/basd_hip.h.  No host sync."""
    _need_cuda(images, labels, out, out_targets)
    assert mixup_supported(images), (tuple(images.shape), images.stride(), images.dtype)
    b, c, h, w = images.shape
    assert labels.dtype == torch.int64 and labels.shape == (b,) and labels.is_contiguous(), (labels.dtype, tuple(labels.shape))
    assert out.shape == images.shape and out.dtype == images.dtype and out.is_contiguous(), (tuple(out.shape), out.dtype)
    assert out_targets.shape == (b, num_classes) and out_targets.dtype == torch.float32 and out_targets.is_contiguous(), \
        (tuple(out_targets.shape), out_targets.dtype)
    y0, y1, x0, x1 = (int(v) for v in box)
    _check(lib().basd_mixup_cutmix(_ptr(images), int(images.dtype == torch.bfloat16), b, c, h, w, _ptr(labels),
                                   int(num_classes), int(mode), ctypes.c_float(lam), y0, y1, x0, x1, _ptr(out),
                                   _ptr(out_targets), _stream()), "basd_mixup_cutmix")
    return out, out_targets


# --------------------------------------------------------------------------- #
# gradient of the tapped student tokens (csrc/tap_grad.hip)
def selector_token_grad_supported(d_s: int) -> bool:
    """student widths basd_selector_token_grad takes (column panels of 192); every other width keeps the torch chain"""
    return d_s in (192, 384, 768)


def selector_token_grad(student, w_tok: torch.Tensor, out=None):
    """student: E same-shape bf16 [B, N, D_s] token tensors (CLS-stripped views are read in place), w_tok [E, D_s, D_s]
    fp32 -> list of E contiguous bf16 [B, N, D_s] gradients (s_i - column mean) w_tok[i]: ONE C call, two launches.
    ``out``: E contiguous bf16 [B, N, D_s] tensors to write into instead of a fresh allocation."""
    _need_cuda(*student, w_tok)
    e = len(student)
    b, n, d = student[0].shape
    assert selector_token_grad_supported(d) and w_tok.shape == (e, d, d), (d, tuple(w_tok.shape))
    assert all(t.dtype == torch.bfloat16 for t in student)
    layers, _, bstride = _layer_views(list(student))
    w = w_tok.detach().contiguous().float()
    if out is None:
        buf = torch.empty(e, b, n, d, dtype=torch.bfloat16, device=w.device)
        outs = [buf[i] for i in range(e)]
    else:
        outs = list(out)
        assert len(outs) == e and all(o.shape == (b, n, d) and o.dtype == torch.bfloat16 and o.is_contiguous()
                                      for o in outs)
    ws = torch.empty(int(lib().basd_selector_token_grad_workspace_bytes(e, d)), dtype=torch.uint8, device=w.device)
    _check(lib().basd_selector_token_grad(_ptr_table(layers), e, b, n, d, ctypes.c_int64(bstride), _ptr(w),
                                          _ptr_table(outs), _ptr(ws), ctypes.c_int64(ws.numel()), _stream()),
           "basd_selector_token_grad")
    return outs


def tap_grad_scatter_supported(d_s: int) -> bool:
    return d_s > 0 and d_s % 64 == 0


def tap_grad_scatter(g_out, g_a, g_b, shape, offset: int, device=None) -> torch.Tensor:
    """Backward of the token tap out[:, offset:, :] of a [B, T, D_s] bf16 block output in one launch:
    g_out (+) pad(g_a (+) g_b) with autograd's bf16 roundings; any of the three may be None (basd_tap_grad_scatter)."""
    b, t, d = shape
    given = [g for g in (g_out, g_a, g_b) if g is not None]
    _need_cuda(*given)
    assert tap_grad_scatter_supported(d) and 0 <= offset < t
    if g_out is not None:
        assert g_out.dtype == torch.bfloat16 and tuple(g_out.shape) == (b, t, d)
        g_out = g_out.contiguous()
    tok = []
    for g in (g_a, g_b):
        if g is not None:
            assert g.dtype == torch.bfloat16 and tuple(g.shape) == (b, t - offset, d)
            g = g.contiguous()
        tok.append(g)
    device = given[0].device if given else device
    out = torch.empty(b, t, d, dtype=torch.bfloat16, device=device)
    _check(lib().basd_tap_grad_scatter(_ptr(g_out), _ptr(tok[0]), _ptr(tok[1]), b, t, d, int(offset), _ptr(out),
                                       _stream()), "basd_tap_grad_scatter")
    return out


# --------------------------------------------------------------------------- #
# token resampling, its adjoint and the importance backward (csrc/resample.hip)
RESAMPLE_MAX_N = 1024


def resample_supported(n_in: int, n_out: int, d: int, dtype) -> bool:
    """token counts, widths and dtypes basd_resample_tokens / _adjoint take; everything else keeps the torch chain"""
    return (1 <= n_in <= RESAMPLE_MAX_N and 1 <= n_out <= RESAMPLE_MAX_N and d >= 4 and d % 4 == 0
            and dtype in (torch.float32, torch.bfloat16))


def _resample_call(entry: str, x: torch.Tensor, n_to: int, n_in: int, n_out: int, out) -> torch.Tensor:
    _need_cuda(x, out)
    assert x.dim() == 3, tuple(x.shape)
    x = x.contiguous()
    b, _, d = x.shape
    if out is None:
        out = torch.empty(b, n_to, d, dtype=x.dtype, device=x.device)
    assert out.shape == (b, n_to, d) and out.dtype == x.dtype and out.is_contiguous()
    _check(getattr(lib(), entry)(_ptr(x), _dtype_code(x), b, n_in, n_out, d, _ptr(out), _stream()), entry)
    return out


def resample_tokens(x: torch.Tensor, n_out: int, out=None) -> torch.Tensor:
    """x [B, n_in, D] fp32 / bf16 -> [B, n_out, D] of the same dtype: F.interpolate(mode="linear",
    align_corners=False) along the token axis in one launch (basd_resample_tokens); written into ``out`` when given."""
    return _resample_call("basd_resample_tokens", x, n_out, x.shape[1], n_out, out)


def resample_tokens_adjoint(g: torch.Tensor, n_in: int, out=None) -> torch.Tensor:
    """g [B, n_out, D] fp32 / bf16 -> [B, n_in, D]: the transpose of ``resample_tokens`` (n_in -> n_out) applied to g,
    i.e. its gradient; gather form, bitwise reproducible (basd_resample_tokens_adjoint)."""
    return _resample_call("basd_resample_tokens_adjoint", g, n_in, n_in, g.shape[1], out)


def procrustes_importance_bwd(g_a: torch.Tensor, a: torch.Tensor, imp: torch.Tensor, out=None) -> torch.Tensor:
    """g_a, a [batch, n_s] (``procrustes_bwd`` / ``procrustes_prep`` outputs), imp [batch, n_t] (what the prep was given),
    all fp32 -> g_imp [batch, n_t]: the gradient through a = R imp / sum(R imp) (basd_procrustes_importance_bwd)."""
    _need_cuda(g_a, a, imp, out)
    for t_ in (g_a, a, imp):
        assert t_.dtype == torch.float32 and t_.is_contiguous() and t_.dim() == 2
    batch, n_s = a.shape
    n_t = imp.shape[1]
    assert g_a.shape == a.shape and imp.shape[0] == batch
    if out is None:
        out = torch.empty(batch, n_t, dtype=torch.float32, device=a.device)
    assert out.shape == (batch, n_t) and out.dtype == torch.float32 and out.is_contiguous()
    _check(lib().basd_procrustes_importance_bwd(_ptr(g_a), _ptr(a), _ptr(imp), batch, n_s, n_t, _ptr(out), _stream()),
           "basd_procrustes_importance_bwd")
    return out

"""The arithmetic contract of the Procrustes backward (basd_procrustes_bwd_side / basd_procrustes_bwd) restated with
plain torch fp32 ops on the CPU.  Written from the contract in include/basd_hip.h, not from the kernels:

* both fp32 operands of P = fac W are split into hi = bf16_rne(x), mid = bf16_rne(x - hi);
* P = fac_hi W_hi + fac_hi W_mid + fac_mid W_hi with fp32 accumulation (a product of two bf16 values is exact in fp32,
  so three fp32 matmuls of the halves are the same sum up to the order of the additions);
* R = W - P;  out = (2 gl sqrt(a)) R rounded to the output type;  rowdot = 2 gl <R, W>, all in fp32.

A kernel that keeps this contract may differ from these functions in the order of its fp32 additions only, so its error
against fp64 is this restatement's error on the same tensors up to a small factor: the yardstick of the GPU tests.
"""
import torch


def split(x):
    hi = x.to(torch.bfloat16).float()
    mid = (x - hi).to(torch.bfloat16).float()
    return hi, mid


def prod3(fac, w):
    fh, fm = split(fac)
    wh, wm = split(w)
    return (fh @ wh + fh @ wm) + fm @ wh


def _rows(p, w, a, gl, out_dtype):
    c2 = 2.0 * gl.view(-1, 1)
    r = w - p
    out = ((c2 * a.sqrt()).unsqueeze(-1) * r).to(out_dtype)
    return out, c2 * (r * w).sum(-1)


def procrustes_bwd_side(fac, w, a, gl, out_dtype=torch.float32):
    """fac [batch, n, n], w [batch, n, d], a [batch, n], gl [batch] (any device) -> (out [batch, n, d] in out_dtype,
    rowdot [batch, n] fp32) on the CPU"""
    fac, w, a, gl = (x.detach().float().cpu() for x in (fac, w, a, gl))
    return _rows(prod3(fac, w), w, a, gl, out_dtype)


def procrustes_bwd(s_w, t_w, a, gl, fac_s, a_t, s_dtype=torch.float32):
    """the whole backward: -> (g_s in s_dtype, g_t fp32, g_a fp32) on the CPU; the student side is the split product on
    the token side (n <= d_s, fac_s [batch, n, n]) and the plain residual of fac_s [batch, n, d_s] on the feature side"""
    s_w, t_w, a, gl, fac_s, a_t = (x.detach().float().cpu() for x in (s_w, t_w, a, gl, fac_s, a_t))
    g_t, dot_t = _rows(prod3(a_t, t_w), t_w, a, gl, torch.float32)
    p_s = prod3(fac_s, s_w) if s_w.shape[1] <= s_w.shape[2] else fac_s
    g_s, dot_s = _rows(p_s, s_w, a, gl, s_dtype)
    return g_s, g_t, (dot_s + dot_t) / (2.0 * a)


def reference_f64(s_w, t_w, a, gl, fac_s, a_t):
    """the same backward in fp64 on the CPU -> (g_s, g_t, g_a)"""
    sw, tw, a64, gl64, fs, at = (x.detach().cpu().double() for x in (s_w, t_w, a, gl, fac_s, a_t))
    p_t = at @ tw
    p_s = fs @ sw if sw.shape[1] <= sw.shape[2] else fs
    c = (2.0 * gl64).view(-1, 1, 1) * a64.sqrt().unsqueeze(-1)
    dot = (2.0 * gl64).view(-1, 1) * (((tw - p_t) * tw).sum(-1) + ((sw - p_s) * sw).sum(-1))
    return c * (sw - p_s), c * (tw - p_t), dot / (2.0 * a64)

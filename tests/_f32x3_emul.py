"""The arithmetic contract of the fp32 split-bf16 ("bf16x3") evaluation attention, restated with plain torch fp32 ops on
the CPU.  Written from the contract in include/basd_hip.h, not from the kernel:

* every fp32 operand v is split into hi = bf16_rne(v), lo = bf16_rne(v - hi);
* a product a b is a_lo b_hi + a_hi b_lo + a_hi b_hi with fp32 accumulation (the products of two bf16 values are exact
  in fp32, so three fp32 matmuls of the halves are the same sum up to the order of the additions);
* logits are scaled in fp32 and not rounded; the softmax runs online over blocks of 128 keys (running maximum, running
  sum, rescaled output); P is unnormalised in (0, 1] against the running maximum and split before P V;
* 1 / sum is applied once to the fp32 output, which is returned as its split image would reconstruct it (hi + lo).
"""
import torch


def split(x):
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def prod3(a, b):
    ah, al = split(a)
    bh, bl = split(b)
    return (al @ bh + ah @ bl) + ah @ bh


def attention_f32x3(qkv, heads, head_dim, scale, block=128):
    """qkv [B, T, 3 heads head_dim] fp32 (any device) -> [B, heads, T, head_dim] fp32 on the CPU"""
    b, t = qkv.shape[0], qkv.shape[1]
    q, k, v = qkv.detach().float().cpu().view(b, t, 3, heads, head_dim).permute(2, 0, 3, 1, 4).contiguous().unbind(0)
    m = torch.full((b, heads, t), float("-inf"))
    l = torch.zeros(b, heads, t)
    o = torch.zeros(b, heads, t, head_dim)
    for k0 in range(0, t, block):
        s = prod3(q, k[:, :, k0:k0 + block].transpose(-2, -1)) * scale
        m_new = torch.maximum(m, s.amax(dim=-1))
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new[..., None])
        l = l * alpha + p.sum(dim=-1)
        o = o * alpha[..., None] + prod3(p, v[:, :, k0:k0 + block])
        m = m_new
    hi, lo = split(o * (1.0 / l)[..., None])
    return hi + lo

"""Shared by the tests of the BEiT teacher past 272 tokens (basd_attention_fwd_long_relbias_bf16).  A plain helper module.

* ``tiny_beit_at(img, patch)``: the tiny model of ``tests/_beit_cases.py`` (D = 128, 2 heads of 64, depth 2, every
  parameter moved off its trivial initial value) on any grid.
* ``emulated_attention``: the arithmetic contract of the tiled kernels with the bias, restated in fp64 with the
  kernel's rounding points and nothing of its order of operations.  It is the accuracy yardstick of
  ``tests/test_attention_long_relbias_gpu.py``: the kernel may reach 1.5 times its error against the exact fp64 attention.
    output: q, k, v in bf16 as given; the dot exact; ``* scale + bias`` in fp32; softmax with P = exp(logit - row maximum)
            rounded to bf16 for the second product, the sum of the UNROUNDED P as the denominator; one rounding of the
            output to bf16.
    tap:    the CLS query's dot rounded to bf16, ``* scale``, ``+`` the two constants of the CLS row (table[R - 1] for
            key 0, table[R - 3] for every patch key), fp32 softmax, without the CLS column, ``/ H`` and summed over heads.
"""
import torch

from tests._beit_ref import meshgrid_index, seeded_table, table_rows

DIM, HEADS, DEPTH = 128, 2, 2


def tiny_beit_at(img: int, patch: int, seed: int = 7):
    """fp32 Beit on the CPU: norms off their identity init, a visible CLS token, q / v biases, LayerScale gammas around
    1 and a seeded bias table per block -- ``tests/_beit_cases.py::tiny_beit`` with the image and patch size given"""
    from basd_amd.models.beit import Beit
    torch.manual_seed(seed)
    model = Beit(img_size=img, patch_size=patch, num_classes=0, embed_dim=DIM, depth=DEPTH, num_heads=HEADS,
                 init_values=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    grid = (img // patch, img // patch)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name or name == "cls_token" or name.endswith("gamma"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("q_bias") or name.endswith("v_bias"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        for i, blk in enumerate(model.blocks):
            blk.attn.relative_position_bias_table.copy_(seeded_table(*grid, HEADS, seed=seed + 10 + i))
    return model.eval()


def _bf16(x):
    return x.to(torch.bfloat16).double()


def emulated_attention(qkv, table, gh: int, gw: int, heads: int, scale: float):
    """qkv [B, T, 3 * heads * hd] bf16, table [R, heads] fp32 -> (out [B, T, heads * hd], importance [B, T - 1]) as
    fp64 tensors holding the values the contract above produces"""
    assert qkv.dtype == torch.bfloat16 and table.dtype == torch.float32
    b, t = qkv.shape[0], qkv.shape[1]
    hd = qkv.shape[-1] // (3 * heads)
    rows = table_rows(gh, gw)
    assert t == gh * gw + 1 and tuple(table.shape) == (rows, heads)
    q, k, v = (qkv.cpu().double().reshape(b, t, 3, heads, hd)[:, :, j].transpose(1, 2) for j in range(3))
    dot = q @ k.transpose(-2, -1)                                   # [B, H, T, T]: bf16 products, exact in fp64
    s32 = torch.tensor(scale, dtype=torch.float32)
    bias = table.cpu()[meshgrid_index(gh, gw)].permute(2, 0, 1)     # [H, T, T] fp32
    logits = (dot.float() * s32 + bias).double()                    # the fp32 logit
    p = torch.exp(logits - logits.amax(dim=-1, keepdim=True))
    out = (_bf16(p) @ v) / p.sum(dim=-1, keepdim=True)
    out = _bf16(out.transpose(1, 2).reshape(b, t, heads * hd))
    row = _bf16(dot[:, :, 0, :]).float() * s32                      # [B, H, T]
    cls_bias = table.cpu()[rows - 3].reshape(1, heads, 1).expand(1, heads, t).clone()
    cls_bias[:, :, 0] = table.cpu()[rows - 1]
    tap = torch.softmax(row + cls_bias, dim=-1)[:, :, 1:] / float(heads)
    return out, tap.double().sum(dim=1)

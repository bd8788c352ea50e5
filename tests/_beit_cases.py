"""Shared by the CPU and GPU tests of the BEiT teacher: the tiny model (64 px, patch 16 -> a 4 x 4 grid, D = 128, 2 heads
of 64, depth 2) with every parameter that starts at a trivial value moved off it.  A plain helper module."""
import torch

from tests._beit_ref import seeded_table

IMG, PATCH, DIM, HEADS, DEPTH = 64, 16, 128, 2, 2
GRID = (IMG // PATCH, IMG // PATCH)


def tiny_beit(seed=7):
    """fp32 Beit on the CPU: norms off their identity init, a visible CLS token, q / v biases, LayerScale gammas around
    1 (not the 0.1 of a fresh BEiT: the blocks should move the tokens) and a seeded bias table per block"""
    from basd_amd.models.beit import Beit
    torch.manual_seed(seed)
    model = Beit(img_size=IMG, patch_size=PATCH, num_classes=0, embed_dim=DIM, depth=DEPTH, num_heads=HEADS,
                 init_values=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name or name == "cls_token" or name.endswith("gamma"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("q_bias") or name.endswith("v_bias"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        for i, blk in enumerate(model.blocks):
            blk.attn.relative_position_bias_table.copy_(seeded_table(*GRID, HEADS, seed=seed + 10 + i))
    return model.eval()


def timm_state_dict(model):
    """the model's weights under timm's Beit key names, with the keys a timm checkpoint carries on top"""
    state = {}
    for key, value in model.state_dict().items():
        key = key.replace(".ls1.gamma", ".gamma_1").replace(".ls2.gamma", ".gamma_2")
        state[key] = value.clone()
    for i, blk in enumerate(model.blocks):
        t = blk.attn.relative_position_index.shape[0]
        state[f"blocks.{i}.attn.relative_position_index"] = torch.zeros(t, t, dtype=torch.int64)
    state["fc_norm.weight"], state["fc_norm.bias"] = torch.ones(DIM), torch.zeros(DIM)
    state["head.weight"], state["head.bias"] = torch.zeros(10, DIM), torch.zeros(10)
    return state

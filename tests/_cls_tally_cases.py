"""Shared by tests/test_cls_tally_cpu.py and tests/test_cls_tally_gpu.py (not a test module): an fp64 torch restatement
of the row semantics of ``basd_cls_tally`` (include/basd_hip.h), the summation order of its second kernel, and the
case table.

Row semantics, with z_j = logits[b, keep[j]] (keep None: the identity), y = labels[b] an index into the SUBSET, s the
label smoothing, all in fp64 on the values as stored:
    rank = #{j : z_j > z_y} + #{j < y : z_j == z_y}       a tie goes to the lowest subset position (argmax's rule);
                                                          NaN orders above every number and equal to NaN (topk's rule)
    loss = lse(z) - (1 - s) z_y - (s / K) sum_j z_j       the last term only when s != 0
    lse(z) = m + log(sum_j exp(z_j - m)),  m = the largest non-NaN z_j, 0 where that is infinite
    a label outside [0, K): rank = K, loss = NaN.
"""
from __future__ import annotations

import math

import torch


def tally_rows(logits: torch.Tensor, labels: torch.Tensor, keep=None, smoothing: float = 0.0):
    """-> (rank [B] int64, loss [B] fp64) on the CPU, from the logits as stored (fp32 or bf16 widen exactly)."""
    z = logits.detach().cpu().double()
    labels = labels.detach().cpu().long()
    if keep is not None:
        z = z[:, torch.as_tensor(keep).cpu().long()]
    k = z.shape[1]
    ok = (labels >= 0) & (labels < k)
    y = labels.clamp(0, k - 1)
    zy = z.gather(1, y[:, None])
    nan, ynan = z.isnan(), zy.isnan()
    gt = torch.where(nan, ~ynan, z > zy)
    eq = torch.where(nan, ynan, z == zy)
    before = torch.arange(k)[None, :] < y[:, None]
    rank = (gt | (eq & before)).sum(1)
    m = torch.where(nan, torch.full_like(z, -math.inf), z).max(1).values
    m = torch.where(m.isinf(), torch.zeros_like(m), m)
    loss = m + torch.log(torch.exp(z - m[:, None]).sum(1)) - (1.0 - smoothing) * zy[:, 0]
    if smoothing != 0.0:
        loss = loss - smoothing / k * z.sum(1)
    rank = torch.where(ok, rank, torch.full_like(rank, k))
    loss = torch.where(ok, loss, torch.full_like(loss, math.nan))
    return rank, loss


def ordered_sum(values: torch.Tensor) -> float:
    """The sum of an fp64 vector in the order of the tally's second kernel: thread t of 256 adds b = t, t + 256, ... in
    turn (starting from 0.0), an xor butterfly (offsets 32 .. 1) over the 64 lanes of each wave, then the four waves left
    to right.  fp64 throughout, so the result is what the kernel adds to the tally, bit for bit."""
    v = values.detach().cpu().double().reshape(-1)
    pad = (-v.numel()) % 256
    v = torch.cat([v, torch.zeros(pad, dtype=torch.float64)]).reshape(-1, 256)      # x + 0.0 == x
    part = torch.zeros(256, dtype=torch.float64)
    for row in v:
        part = part + row
    part = part.reshape(4, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ off]
    w = part[:, 0]
    return float(((w[0] + w[1]) + w[2]) + w[3])


def f32(x: float) -> float:
    """the C entry takes the smoothing as a float: the value it computes with"""
    return float(torch.tensor(x, dtype=torch.float32))


def loss_close(got: torch.Tensor, want: torch.Tensor, zmax: torch.Tensor):
    """|got - want| <= 1e-12 |want| + 1e-12 max|z| of the row, where both are finite; the same NaN / infinity elsewhere.
    Both sides are fp64 sums of at most a few ten thousand terms, double exp / log: the bound follows from the
    arithmetic (n eps ~ 2e-12 is the worst case of a 21 843-term sum of one sign, scaled by s / K << 1 here)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    fin = want.isfinite()
    assert torch.equal(got.isfinite(), fin), (got, want)
    assert torch.equal(got[~fin].isnan(), want[~fin].isnan()) and torch.equal(got[~fin & ~want.isnan()],
                                                                               want[~fin & ~want.isnan()]), (got, want)
    err = (got[fin] - want[fin]).abs()
    bound = 1e-12 * want[fin].abs() + 1e-12 * zmax[fin]
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    return float(err.max()) if err.numel() else 0.0


def row_zmax(logits: torch.Tensor, keep=None) -> torch.Tensor:
    """largest finite |z_j| of every row (0 for a row without finite entries)"""
    z = logits.detach().cpu().double()
    if keep is not None:
        z = z[:, torch.as_tensor(keep).cpu().long()]
    return torch.where(z.isfinite(), z.abs(), torch.zeros_like(z)).max(1).values


# name -> dict(B, C, and optionally: dtype, pad (row_stride = C + pad, padding +inf), keep ("perm200" | list), special)
CASES = {
    "smallest":        dict(B=1, C=1),
    "idle_lanes":      dict(B=3, C=5),
    "stride_255":      dict(B=2, C=255),
    "stride_256":      dict(B=2, C=256),
    "stride_257":      dict(B=2, C=257),
    "classes_1000":    dict(B=37, C=1000, special="edge_labels"),
    "long_rows":       dict(B=4, C=21843),
    "ragged_batch":    dict(B=300, C=10),
    "padded_rows":     dict(B=5, C=100, pad=7),
    "bf16":            dict(B=37, C=1000, dtype=torch.bfloat16, special="edge_labels"),
    "bf16_padded":     dict(B=5, C=257, dtype=torch.bfloat16, pad=3),
    "keep_200":        dict(B=9, C=1000, keep="perm200"),
    "keep_3":          dict(B=6, C=40, keep=[31, 2, 17]),
    "keep_1":          dict(B=3, C=40, keep=[9]),
    "tie_whole_row":   dict(B=4, C=300, special="tie_whole_row"),
    "tie_target":      dict(B=4, C=300, special="tie_target"),
    "neg_inf":         dict(B=4, C=300, special="neg_inf"),
    "nan_row":         dict(B=5, C=300, special="nan_row"),
    "bad_label":       dict(B=5, C=300, special="bad_label"),
    "bad_label_keep":  dict(B=4, C=40, keep=[31, 2, 17], special="bad_label"),
}


def make_case(name: str):
    """-> (storage [B, C + pad], logits = storage[:, :C] (a view), labels [B] int64, keep (list | None), K), CPU tensors,
    seeded by the case's name."""
    spec = CASES[name]
    b, c, pad = spec["B"], spec["C"], spec.get("pad", 0)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    storage = torch.full((b, c + pad), math.inf)
    storage[:, :c] = 3.0 * torch.randn(b, c, generator=g)
    storage = storage.to(spec.get("dtype", torch.float32))
    logits = storage[:, :c]
    keep = spec.get("keep")
    if keep == "perm200":
        keep = torch.randperm(c, generator=g)[:200].tolist()
    k = c if keep is None else len(keep)
    sub = logits.double() if keep is None else logits.double()[:, keep]
    order = sub.argsort(dim=1, descending=True)
    labels = torch.randint(0, k, (b,), generator=g)
    for i in range(b):                                  # a mix of hits at 1, hits inside the top 5 and misses
        if i % 3 == 0:
            labels[i] = order[i, 0]
        elif i % 3 == 1:
            labels[i] = order[i, min(3, k - 1)]
    special = spec.get("special")
    if special == "edge_labels":                        # the target in the first and in the last column
        labels[0], labels[1] = 0, c - 1
    elif special == "tie_whole_row":                    # every rank is the label itself
        logits[:] = 1.25
        labels = torch.tensor([0, 1, 4, 5][:b])         # ranks 0, 1, 4 (the last hit at 5), 5 (the first miss)
    elif special == "tie_target":                       # the target tied with an earlier and a later column, on top
        for i in range(b):
            top = float(logits[i].max()) + 1.0
            logits[i, 7], logits[i, 100], logits[i, 299] = top, top, top
        labels = torch.tensor([100, 7, 299, 100][:b])   # ranks 1, 0, 2, 1
    elif special == "neg_inf":
        labels[:] = 5
        logits[:, 0] = -math.inf
        logits[1, 6:200] = -math.inf
        logits[2, :5] = -math.inf
        logits[2, 6:] = -math.inf                       # only the target is left: loss 0
    elif special == "nan_row":
        logits[2, 17] = math.nan
        logits[3, 17] = math.nan
        labels[3] = 17                                  # the NaN as the target: rank 0
        logits[4, 17] = math.nan
        logits[4, 250] = math.nan
        labels[4] = 250                                 # two NaNs tie: the earlier one wins, rank 1
    elif special == "bad_label":
        labels[1] = k
        labels[3] = -1
    return storage, logits, labels, keep, k

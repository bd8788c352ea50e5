"""Inputs and error figures shared by the tests of the resident Procrustes backward kernel
(tests/test_procrustes_bwd_resident_cpu.py, tests/test_procrustes_bwd_resident_gpu.py): one side of the backward,
basd_procrustes_bwd_side(fac [batch, n, n], w [batch, n, d], a [batch, n], gl [batch]) -> out, rowdot."""
import functools

import torch

from tests import _pbwd_emul

# (batch, n, d, bf16 output): every (n, d) range in which the kernel takes another path.
#   n: 196 = 7 + 6 m tiles in two row tiles, K tail 4, row tail 4 (the bench's shape); 256 = three row tiles of 6 / 5 / 5
#   (two tiles of 8 do not fit the LDS), exact tiles; 240 = three tiles of 5; 132 = 5 + 4; 128 = one tile of 8; 100 =
#   one tile of 7; 80 = one tile of 5, the fewest m tiles the resident kernel is dispatched for; 64 = the other side of
#   that boundary (the staged kernel).  Up to 128 rows the resident kernel needs d >= 112 as well: d = 96 and d = 16
#   at n = 80 / 100 are the other side of that boundary.  Up to 48 rows W is not staged (the direct kernel): 20 = two m
#   tiles with a K tail of 20 and a row tail of 4; 32 = two exact tiles, one K step; 48 = three tiles in the kernel for
#   four, with a ragged column group.
#   d: 16 = one strip for eight waves (n >= 132); 112 = a ragged group alone; 144 / 208 = a ragged group after a full
#   128-column one; 768 = six full groups.
#   batch: 300 matrices at n = 80 are more workgroups than the 256 CUs, so the grid's (matrix, tile) mapping wraps: at
#   d = 16 on the staged kernel, at d = 112 on the resident one; 3 is no multiple of the 8 matrices the mapping deals
#   out together.
CASES = [(1, 196, 768, False), (3, 196, 768, True), (2, 196, 112, False), (2, 196, 16, True), (1, 256, 768, True),
         (2, 256, 112, False), (2, 240, 208, False), (2, 132, 112, False), (2, 132, 16, True), (2, 128, 144, True),
         (2, 100, 112, True), (2, 100, 16, False), (300, 80, 16, False), (300, 80, 112, False), (2, 80, 112, True),
         (2, 80, 96, False), (2, 64, 112, False), (2, 64, 16, True), (2, 20, 16, False), (2, 32, 48, True),
         (2, 48, 112, False)]


def white(batch, n, d):
    """the construction of test_procrustes_bwd_entry_matches_the_unfused_chain (tests/test_kernels_gpu.py), one side"""
    g = torch.Generator().manual_seed(batch * 1000 + n + 7 * d)
    w = torch.randn(batch, n, d, generator=g)
    a = torch.rand(batch, n, generator=g) + 0.1
    a = (a / a.sum(-1, keepdim=True)).contiguous()
    gl = torch.randn(batch, generator=g)
    fac = torch.randn(batch, n, n, generator=g) / n ** 0.5
    return fac, w, a, gl


def trained(batch=2, n=196, d=768, rank=96, exact_rows=24):
    """The trained-network construction of DESIGN 5e at the bench's shape: 8 massive-activation channels of W (|mean|
    1e2 x their spread), 90 % of the importance on 5 % of the rows, and fac = an orthogonal projector of rank 96 plus
    1e-3 noise that is the identity on 24 scattered rows, so that P = fac W cancels W there down to the noise."""
    g = torch.Generator().manual_seed(196)
    w = torch.randn(batch, n, d, generator=g)
    ch = torch.randperm(d, generator=g)[:8]
    w[:, :, ch] += 100.0 * torch.where(torch.rand(8, generator=g) < 0.5, -1.0, 1.0)
    heavy = n // 20
    a = torch.empty(batch, n)
    for b in range(batch):
        perm = torch.randperm(n, generator=g)
        hi, lo = torch.rand(heavy, generator=g) + 0.5, torch.rand(n - heavy, generator=g) + 0.5
        a[b, perm[:heavy]] = 0.9 * hi / hi.sum()
        a[b, perm[heavy:]] = 0.1 * lo / lo.sum()
    gl = torch.randn(batch, generator=g)
    fac = torch.zeros(batch, n, n)
    for b in range(batch):
        perm = torch.randperm(n, generator=g)
        q = torch.linalg.qr(torch.randn(n - exact_rows, rank - exact_rows, generator=g, dtype=torch.float64))[0]
        proj = torch.zeros(n, n, dtype=torch.float64)
        proj[:exact_rows, :exact_rows] = torch.eye(exact_rows, dtype=torch.float64)
        proj[exact_rows:, exact_rows:] = q @ q.t()
        fac[b] = proj[perm][:, perm].float()
    fac += 1e-3 * torch.randn(batch, n, n, generator=g)
    return fac.contiguous(), w, a.contiguous(), gl


def reference_f64(fac, w, a, gl):
    """-> (out, rowdot) in fp64"""
    f, x, a64, gl64 = fac.double(), w.double(), a.double(), gl.double()
    r = x - f @ x
    c2 = (2.0 * gl64).view(-1, 1)
    return (c2 * a64.sqrt()).unsqueeze(-1) * r, c2 * (r * x).sum(-1)


def errors(out, rowdot, want):
    """rel-L2 and max-abs over max |want| of both outputs"""
    want_out, want_dot = want
    o, r = out.detach().cpu().double(), rowdot.detach().cpu().double()
    return {"out": float((o - want_out).norm() / want_out.norm()),
            "out max": float((o - want_out).abs().max() / want_out.abs().max()),
            "rowdot": float((r - want_dot).norm() / want_dot.norm()),
            "rowdot max": float((r - want_dot).abs().max() / want_dot.abs().max())}


@functools.lru_cache(maxsize=None)
def case(kind, batch, n, d, bf16):
    """inputs, the fp64 reference and the restatement's errors of one case: computed once, shared, never modified"""
    inputs = trained(batch, n, d) if kind == "trained" else white(batch, n, d)
    want = reference_f64(*inputs)
    dtype = torch.bfloat16 if bf16 else torch.float32
    emul = errors(*_pbwd_emul.procrustes_bwd_side(*inputs, dtype), want)
    return inputs, want, emul

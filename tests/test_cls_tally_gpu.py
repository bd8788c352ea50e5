"""The evaluation tally kernels (csrc/eval_tally.hip, basd_cls_tally) against the fp64 restatement of
tests/_cls_tally_cases.py: row_rank must be equal, row_loss within rtol 1e-12 and atol 1e-12 max|z| of the row (both
sides are fp64 with at most a few ten thousand terms per reduction: the bound follows from the arithmetic, it is not a
measurement), the tally equal, bit for bit and from run to run, to its previous value plus the kernel-ordered fp64 sums.
The restatement gets the smoothing the entry computes with (the float it is passed as)."""
import ctypes
import math
import types

import pytest
import torch
import torch.nn as nn

from tests._cls_tally_cases import CASES, f32, loss_close, make_case, ordered_sum, row_zmax, tally_rows

pytestmark = pytest.mark.gpu

TALLY0 = [3.0, 7.0, 1.5, 11.0]


@pytest.fixture(autouse=True)
def _native():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    native.lib()
    _ops.set_ops(None)
    yield native


def _same(a: float, b: float) -> bool:
    return a == b or (a != a and b != b)


def _run(native, name, smoothing):
    storage, logits, labels, keep, k = make_case(name)
    dev_logits = storage.cuda()[:, :logits.shape[1]]                  # the padding travels along, as +inf
    assert dev_logits.stride(0) == logits.stride(0)
    dev_keep = None if keep is None else torch.tensor(keep, device="cuda")
    top_k = min(5, k)
    tally = torch.tensor(TALLY0, dtype=torch.float64, device="cuda")
    rank, loss = native.cls_tally(dev_logits, labels.cuda(), tally, keep=dev_keep, top_k=top_k, smoothing=smoothing)
    torch.cuda.synchronize()
    return logits, labels, keep, k, top_k, rank.cpu(), loss.cpu(), tally.cpu(), (dev_logits, dev_keep)


@pytest.mark.parametrize("smoothing", ["0", "1/C"])
@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_tally_match_the_fp64_restatement(_native, name, smoothing):
    s = 0.0 if smoothing == "0" else 1.0 / CASES[name]["C"]
    logits, labels, keep, k, top_k, rank, loss, tally, dev = _run(_native, name, s)
    want_rank, want_loss = tally_rows(logits, labels, keep, f32(s))
    assert rank.dtype == torch.int32 and loss.dtype == torch.float64
    assert torch.equal(rank.long(), want_rank), (rank.tolist()[:8], want_rank.tolist()[:8])
    err = loss_close(loss, want_loss, row_zmax(logits, keep))
    want_tally = [TALLY0[0] + int((want_rank == 0).sum()), TALLY0[1] + int((want_rank < top_k).sum()),
                  TALLY0[2] + ordered_sum(loss), TALLY0[3] + labels.numel()]
    print(f"{name} s={smoothing}: K {k} top_k {top_k} hits {int((want_rank == 0).sum())} / "
          f"{int((want_rank < top_k).sum())} of {labels.numel()}, max loss error {err:.3e}, tally {tally.tolist()}")
    assert all(_same(a, b) for a, b in zip(tally.tolist(), want_tally)), (tally.tolist(), want_tally)
    # run to run: the same bits
    again = torch.tensor(TALLY0, dtype=torch.float64, device="cuda")
    rank2, loss2 = _native.cls_tally(dev[0], labels.cuda(), again, keep=dev[1], top_k=top_k, smoothing=s)
    assert torch.equal(rank2.cpu(), rank)
    assert torch.equal(loss2.cpu().view(torch.int64), loss.view(torch.int64))
    assert torch.equal(again.cpu().view(torch.int64), tally.view(torch.int64))


def test_bf16_reads_the_stored_values(_native):
    """the same bf16 values widened to fp32 give the same rows, bit for bit"""
    storage, logits, labels, _, k = make_case("bf16")
    t16, t32 = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    r16, l16 = _native.cls_tally(logits.cuda(), labels.cuda(), t16, top_k=5, smoothing=0.001)
    r32, l32 = _native.cls_tally(logits.float().cuda(), labels.cuda(), t32, top_k=5, smoothing=0.001)
    assert torch.equal(r16, r32) and torch.equal(l16, l32) and torch.equal(t16, t32)
    assert float(t16[0]) >= 1 and float(t16[1]) > float(t16[0]) and float(t16[3]) == 37


def test_two_calls_accumulate_and_an_empty_batch_leaves_the_tally(_native):
    _, la, ya, _, _ = make_case("classes_1000")
    _, lb, yb, _, _ = make_case("bf16")
    tally = torch.zeros(4, dtype=torch.float64, device="cuda")
    ra, xa = _native.cls_tally(la.cuda(), ya.cuda(), tally, top_k=5)
    first = tally.clone()
    rb, xb = _native.cls_tally(lb.cuda(), yb.cuda(), tally, top_k=5)
    one = torch.zeros(4, dtype=torch.float64, device="cuda")
    _native.cls_tally(lb.cuda(), yb.cuda(), one, top_k=5)
    want = [float(first[0]) + float(one[0]), float(first[1]) + float(one[1]),
            float(first[2]) + ordered_sum(xb), float(first[3]) + 37]
    assert tally.tolist() == want and float(tally[3]) == 74
    assert float(first[2]) == ordered_sum(xa)
    before = tally.clone()
    r0, x0 = _native.cls_tally(torch.empty(0, 1000, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                               tally, top_k=5)
    assert r0.shape == (0,) and x0.shape == (0,) and torch.equal(tally.view(torch.int64), before.view(torch.int64))


def test_shape_errors_return_their_status_and_launch_nothing(_native):
    b, c = 4, 10
    z = torch.randn(b, c, device="cuda")
    y = torch.zeros(b, dtype=torch.int64, device="cuda")
    keep = torch.tensor([3, 1, 2], device="cuda")
    rank = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((b,), -7.0, dtype=torch.float64, device="cuda")
    tally = torch.tensor(TALLY0, dtype=torch.float64, device="cuda")
    P, L = _native._ptr, ctypes.c_int64

    def call(*, logits=z, stride=c, labels=y, keep_=None, k=c, top_k=5, rank_=rank, loss_=loss, tally_=tally, rows=b,
             cols=c):
        return _native.lib().basd_cls_tally(P(logits), 0, L(stride), P(labels), P(keep_), rows, cols, k, top_k,
                                            ctypes.c_float(0.0), P(rank_), P(loss_), P(tally_),
                                            _native._stream())

    bad = {"top_k = 0": dict(top_k=0), "top_k > K": dict(top_k=11), "top_k > K of a subset": dict(keep_=keep, k=3, top_k=4),
           "keep NULL with K != C": dict(k=3, top_k=3), "row_stride < C": dict(stride=c - 1),
           "no row_rank": dict(rank_=None), "no row_loss": dict(loss_=None), "no tally": dict(tally_=None),
           "no logits": dict(logits=None), "no labels": dict(labels=None), "C = 0": dict(cols=0, k=0, top_k=1)}
    for what, kw in bad.items():
        assert call(**kw) == 1, what                                   # BASD_ERR_SHAPE
        assert b"cls_tally" in _native.lib().basd_last_error(), what
    torch.cuda.synchronize()
    assert bool((rank == -7).all()) and bool((loss == -7.0).all()) and tally.tolist() == TALLY0
    assert call(rows=0) == 0                                           # an empty batch is legal and enqueues nothing
    assert call() == 0 and call(keep_=keep, k=3, top_k=3) == 0         # the same buffers are fine with legal arguments
    torch.cuda.synchronize()
    assert float(tally[3]) == TALLY0[3] + 2 * b and bool((rank >= 0).all())
    # the wrapper raises with the entry's message
    with pytest.raises(_native.BasdNativeError, match="top_k"):
        _native.cls_tally(z, y, tally, top_k=11)


def test_entry_is_legal_inside_a_stream_capture(_native):
    _, logits, labels, _, _ = make_case("classes_1000")
    z, y = logits.cuda(), labels.cuda()
    tally = torch.zeros(4, dtype=torch.float64, device="cuda")
    one = torch.zeros(4, dtype=torch.float64, device="cuda")
    _native.cls_tally(z, y, one, top_k=5)                              # also loads the code object before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.cls_tally(z, y, tally, top_k=5)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert tally.tolist() == [2 * float(one[0]), 2 * float(one[1]), float(one[2]) + float(one[2]), 74.0]


class _Table(nn.Module):
    """logits looked up from the first pixel, as in tests/test_evaluation_cpu.py"""

    def __init__(self, logits):
        super().__init__()
        self.table = nn.Parameter(logits, requires_grad=False)

    def forward(self, x):
        return self.table[x[:, 0, 0, 0].long()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("subset", [False, True])
def test_evaluate_model_runs_on_the_kernel(_native, subset, dtype, monkeypatch):
    from basd_amd.evaluation import evaluate_model
    from basd_amd.losses import _ops
    g = torch.Generator().manual_seed(7)
    n, c = 70, 50
    # every row a permutation of 50 distinct eighths: exact in bf16, no ties
    table = torch.stack([(torch.randperm(c, generator=g) - c // 2) * 0.125 for _ in range(n)]).to(dtype)
    keep = torch.randperm(c, generator=g)[:12].tolist() if subset else None
    k = len(keep) if subset else c
    labels = torch.randint(0, k, (n,), generator=g)
    sub = table.double() if keep is None else table.double()[:, keep]
    assert all(row.unique().numel() == k for row in sub)                # tie free: topk and the kernel must agree
    labels[::4] = sub.argmax(1)[::4]
    batches = [{"pixel_values": torch.arange(i, min(i + 32, n)).float().view(-1, 1, 1, 1).expand(-1, 3, 2, 2).clone(),
                "label": labels[i:i + 32]} for i in range(0, n, 32)]
    crit = nn.CrossEntropyLoss(label_smoothing=0.1)
    model = _Table(table).cuda()
    calls = []
    real = _native.cls_tally
    monkeypatch.setattr(_native, "cls_tally", lambda *a, **kw: calls.append(kw["top_k"]) or real(*a, **kw))
    _ops.FALLBACKS.clear()
    _ops.set_strict(True)
    try:
        got = evaluate_model(model, batches, crit, num_classes=k, valid_indices=keep)
        kernel_ledger = dict(_ops.FALLBACKS)
        # the torch accounting on the same device model: a provider without the fused tally
        _ops.set_ops(types.SimpleNamespace(handles=lambda t: True))
        torch_path = evaluate_model(model, batches, crit, num_classes=k, valid_indices=keep)
        torch_ledger = dict(_ops.FALLBACKS)
    finally:
        _ops.set_strict(False)
        _ops.set_ops(None)
    assert calls == [5, 5, 5]
    assert sum(kernel_ledger.values()) <= sum(torch_ledger.values()) and not kernel_ledger
    order = sub.argsort(dim=1, descending=True)
    top1 = 100.0 * float((order[:, 0] == labels).double().mean())
    top5 = 100.0 * float((order[:, :5] == labels[:, None]).any(1).double().mean())
    want_loss = float(nn.CrossEntropyLoss(label_smoothing=f32(0.1))(sub, labels))
    assert abs(got["val_acc"] - top1) < 1e-9 and abs(got["val_acc_top5"] - top5) < 1e-9 and 0 < top1 < top5 < 100
    assert abs(got["loss"] - want_loss) <= 1e-12 * want_loss + 1e-12 * float(sub.abs().max())
    assert got["val_acc"] == torch_path["val_acc"] and got["val_acc_top5"] == torch_path["val_acc_top5"]
    assert abs(got["loss"] - torch_path["loss"]) <= 1e-6 * want_loss   # the torch path takes fp32 batch means
    assert set(got) == {"val_acc", "val_acc_top5", "loss"} and math.isfinite(got["loss"])

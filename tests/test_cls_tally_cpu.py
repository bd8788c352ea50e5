"""Host side of the evaluation tally (basd_cls_tally): the fp64 restatement the GPU tests compare the kernel with is
pinned to the reference's arithmetic (topk hits, nn.CrossEntropyLoss) and to hand-written expectations for what topk
leaves open; the export table; evaluate_model keeps its torch accounting under the kernel emulation and on the CPU."""
import math
import types

import pytest
import torch
import torch.nn as nn

from tests._cls_tally_cases import CASES, f32, make_case, ordered_sum, tally_rows


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("keep", [None, [11, 3, 40, 7, 25, 0, 19]])
def test_restatement_is_topk_and_cross_entropy_on_tie_free_inputs(keep, smoothing):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(64, 41, generator=g)
    assert all(row.unique().numel() == 41 for row in logits)
    k = 41 if keep is None else len(keep)
    labels = torch.randint(0, k, (64,), generator=g)
    rank, loss = tally_rows(logits, labels, keep, smoothing)
    sub = logits.double() if keep is None else logits.double()[:, keep]       # the reference's outputs[:, valid_indices]
    top = sub.topk(5, dim=1).indices
    assert torch.equal(rank == 0, top[:, 0] == labels)
    assert torch.equal(rank < 5, (top == labels[:, None]).any(1))
    assert 0 < int((rank == 0).sum()) + int((rank < 5).sum()) and int((rank >= 5).sum()) > 0
    want = nn.CrossEntropyLoss(label_smoothing=smoothing, reduction="none")(sub, labels)
    torch.testing.assert_close(loss, want, rtol=1e-13, atol=1e-13)


def test_tie_rule_by_hand():
    z = torch.tensor([[2.0, 5.0, 5.0, 1.0, 5.0],
                      [2.0, 5.0, 5.0, 1.0, 5.0],
                      [2.0, 5.0, 5.0, 1.0, 5.0],
                      [7.0, 7.0, 7.0, 7.0, 7.0],
                      [2.0, 5.0, 5.0, 1.0, 5.0]])
    rank, loss = tally_rows(z, torch.tensor([1, 2, 4, 3, 0]))
    assert rank.tolist() == [0, 1, 2, 3, 3]
    assert int(z[0].argmax()) == 1                                             # the winner of a tie is argmax's
    lse = math.log(math.exp(2 - 5) + 3 + math.exp(1 - 5)) + 5
    assert abs(float(loss[0]) - (lse - 5.0)) < 1e-14 and abs(float(loss[3]) - math.log(5)) < 1e-14
    # through a subset the positions are the subset's: columns [4, 0, 1] -> z = [5, 2, 5]
    rank, _ = tally_rows(z[:1], torch.tensor([2]), keep=[4, 0, 1])
    assert rank.tolist() == [1]


def test_nan_orders_as_in_topk():
    nan = math.nan
    z = torch.tensor([[1.0, nan, 3.0, 0.0],
                      [1.0, nan, 3.0, 0.0],
                      [nan, 2.0, nan, 0.0],
                      [nan, 2.0, nan, 0.0]])
    rank, loss = tally_rows(z, torch.tensor([2, 1, 2, 1]))
    assert rank.tolist() == [1, 0, 1, 2]            # NaN above 3; NaN first; the earlier of two NaNs; both NaNs above 2
    assert bool(loss.isnan().all())
    assert z.topk(2, dim=1).indices[:2, 0].tolist() == [1, 1]                  # torch.topk puts the NaN first as well


def test_out_of_range_label_and_infinities():
    z = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [-math.inf, 2.0, -math.inf]])
    rank, loss = tally_rows(z, torch.tensor([3, -1, 2, 1]))
    assert rank.tolist() == [3, 3, 0, 0]
    assert loss[:2].isnan().all() and float(loss[3]) == 0.0
    assert abs(float(loss[2]) - (math.log(math.exp(-2) + math.exp(-1) + 1))) < 1e-15
    # with smoothing a -inf logit costs an infinite loss, as in torch
    _, loss = tally_rows(z[3:], torch.tensor([1]), smoothing=0.1)
    want = nn.CrossEntropyLoss(label_smoothing=0.1, reduction="none")(z[3:].double(), torch.tensor([1]))
    assert float(loss[0]) == math.inf == float(want[0])


def test_case_table_covers_what_it_claims():
    for name in CASES:
        storage, logits, labels, keep, k = make_case(name)
        spec = CASES[name]
        assert logits.shape == (spec["B"], spec["C"]) and logits.stride(0) == spec["C"] + spec.get("pad", 0)
        assert logits.data_ptr() == storage.data_ptr() and k == (spec["C"] if keep is None else len(keep))
        if spec.get("pad"):
            assert bool(storage[:, spec["C"]:].isinf().all())
        if keep is not None:
            assert len(set(keep)) == len(keep) and (len(keep) < 2 or keep != sorted(keep))
    rank, loss = tally_rows(*[make_case("tie_whole_row")[i] for i in (1, 2)])
    assert rank.tolist() == [0, 1, 4, 5]
    rank, loss = tally_rows(*[make_case("tie_target")[i] for i in (1, 2)])
    assert rank.tolist() == [1, 0, 2, 1]
    _, logits, labels, _, _ = make_case("neg_inf")
    rank, loss = tally_rows(logits, labels)
    assert bool(loss.isfinite().all()) and float(loss[2]) == 0.0
    _, logits, labels, _, _ = make_case("nan_row")
    rank, loss = tally_rows(logits, labels)
    assert loss.isnan().tolist() == [False, False, True, True, True] and rank[3:].tolist() == [0, 1]
    _, logits, labels, keep, k = make_case("bad_label_keep")
    rank, loss = tally_rows(logits, labels, keep)
    assert rank[[1, 3]].tolist() == [3, 3] and loss.isnan().tolist() == [False, True, False, True]
    _, logits, labels, _, _ = make_case("classes_1000")
    assert labels[:2].tolist() == [0, 999]


def test_ordered_sum_is_a_sum():
    g = torch.Generator().manual_seed(1)
    for n in (1, 5, 256, 257, 300, 1000):
        v = torch.randn(n, generator=g, dtype=torch.float64)
        assert abs(ordered_sum(v) - math.fsum(v.tolist())) <= 1e-15 * n * float(v.abs().max())
    assert ordered_sum(torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)) == 7.0
    assert f32(0.001) != 0.001 and f32(0.5) == 0.5


def test_entry_is_in_the_export_table():
    import basd_amd._native as native
    assert "basd_cls_tally" in native.EXPORTS
    sig = native._SIGNATURES["basd_cls_tally"]
    assert len(sig) == 14 and sig[2] is native._I64 and sig[9] is native._F
    assert hasattr(native.lib(), "basd_cls_tally")
    assert callable(native.cls_tally) and callable(native.cls_tally_supported)


def test_wrapper_refuses_cpu_tensors():
    import basd_amd._native as native
    z = torch.zeros(2, 3)
    assert not native.cls_tally_supported(z)
    with pytest.raises(native.BasdNativeError):
        native.cls_tally(z, torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.float64), top_k=1)


class _Table(nn.Module):
    """logits looked up from the first pixel, as in tests/test_evaluation_cpu.py"""

    def __init__(self, logits):
        super().__init__()
        self.table = nn.Parameter(logits, requires_grad=False)

    def forward(self, x):
        return self.table[x[:, 0, 0, 0].long()]


def _batches(labels, bs=4):
    n = labels.numel()
    return [{"pixel_values": torch.arange(i, min(i + bs, n)).float().view(-1, 1, 1, 1).expand(-1, 3, 2, 2).clone(),
             "label": labels[i:i + bs]} for i in range(0, n, bs)]


def _torch_accounting(logits, labels, crit, num_classes, keep, bs=4):
    """evaluate_model's accounting before the fused tally existed, batch by batch"""
    tally = torch.zeros(4, dtype=torch.float64)
    for i in range(0, labels.numel(), bs):
        lg, y = logits[i:i + bs].float(), labels[i:i + bs]
        if keep is not None:
            lg = lg.index_select(1, torch.as_tensor(keep))
        hit = lg.topk(min(5, num_classes, lg.shape[1]), dim=1).indices.eq(y.unsqueeze(1))
        tally[0] += hit[:, 0].sum()
        tally[1] += hit.any(dim=1).sum()
        tally[2] += crit(lg, y).double() * y.numel()
        tally[3] += y.numel()
    h1, h5, loss, n = tally.tolist()
    return {"val_acc": 100.0 * h1 / n, "val_acc_top5": 100.0 * h5 / n, "loss": loss / n}


@pytest.mark.parametrize("provider", ["emulation", "native", "no_kernels"])
@pytest.mark.parametrize("keep", [None, [6, 1, 4, 3, 9, 0]])
def test_evaluate_model_keeps_the_torch_path_without_the_kernel(provider, keep):
    """the kernel emulation has no cls_tally (and handles every tensor): evaluate_model must not ask it for one; CPU
    logits are not the native provider's either"""
    from basd_amd.evaluation import evaluate_model
    from basd_amd.losses import _ops
    from tests import _emul
    assert not hasattr(_emul, "cls_tally")
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(10, 12, generator=g)
    k = 12 if keep is None else len(keep)
    labels = torch.randint(0, k, (10,), generator=g)
    crit = nn.CrossEntropyLoss(label_smoothing=0.05)
    want = _torch_accounting(logits, labels, crit, k, keep)
    _ops.set_ops({"emulation": _emul, "native": None,
                  "no_kernels": types.SimpleNamespace(handles=lambda t: False)}[provider])
    try:
        got = evaluate_model(_Table(logits), _batches(labels), crit, num_classes=k, valid_indices=keep)
    finally:
        _ops.set_ops(None)
    assert got == want

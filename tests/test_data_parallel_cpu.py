"""world_size-2 gloo test of the bucketed gradient reducer: after backward +
finish() every rank holds mean_r(g_r), parameters were broadcast from rank 0,
and several buckets are exercised (the all-reduce is checked as
mean_r(g_r))."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _model(seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(20, 64), nn.GELU(), nn.Linear(64, 64), nn.GELU(), nn.Linear(64, 5))


def _data(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(8, 20, generator=g), torch.randint(0, 5, (8,), generator=g)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from basd_amd.training.data_parallel import GradientReducer
    from basd_amd.training.optim import FlatParams
    model = _model(seed=rank)                       # different init per rank: broadcast must fix it
    flat = FlatParams(list(model.parameters()))
    reducer = GradientReducer(flat, bucket_bytes=1024)   # several buckets
    assert len(reducer.buckets) >= 3
    reducer.broadcast_parameters(0)
    for _ in range(2):                              # two steps: pending counters must reset
        flat.zero_grad()
        x, y = _data(rank)
        nn.functional.cross_entropy(model(x), y).backward()
        reducer.finish()
    torch.save({"grad": flat.grad.clone(), "data": flat.data.clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_rank_gradient_mean(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "r0.pt")
    r1 = torch.load(tmp_path / "r1.pt")
    torch.testing.assert_close(r0["grad"], r1["grad"], atol=0, rtol=0)
    torch.testing.assert_close(r0["data"], r1["data"], atol=0, rtol=0)
    # single-process reference: same weights (rank 0's), mean of the two shard gradients
    from basd_amd.training.optim import FlatParams
    model = _model(seed=0)
    flat = FlatParams(list(model.parameters()))
    torch.testing.assert_close(flat.data, r0["data"])
    want = torch.zeros_like(flat.grad)
    for rank in range(2):
        flat.zero_grad()
        x, y = _data(rank)
        nn.functional.cross_entropy(model(x), y).backward()
        want += flat.grad / 2
    torch.testing.assert_close(r0["grad"], want, atol=1e-7, rtol=1e-6)


def test_reducer_is_a_noop_without_process_group():
    from basd_amd.training.data_parallel import GradientReducer
    from basd_amd.training.optim import FlatParams
    model = _model(0)
    flat = FlatParams(list(model.parameters()))
    red = GradientReducer(flat)
    assert not red.enabled
    x, y = _data(0)
    nn.functional.cross_entropy(model(x), y).backward()
    g = flat.grad.clone()
    red.finish()
    torch.testing.assert_close(flat.grad, g, atol=0, rtol=0)


# ---------------------------------------------------------------------------------------------------------
# The REAL trainer on two ranks (BASELINE c1 shapes, kernels emulated on CPU): per-rank loss parity on the rank's shard,
# gradient mean through both reduction paths (bucket hooks + finish(), and the single reduce_all() used after a hipGraph
# replay), temperatures averaged with the student parameters.
CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")


def _c1_trainer():
    from basd_amd.config import load_config
    from basd_amd.losses import _ops
    from basd_amd.train import build
    from tests import _emul
    _ops.set_ops(_emul)
    torch.manual_seed(0)
    cfg = load_config(CFG, "basd_cifar100", ["data.batch_size=8", "model.drop_path_rate=0.0", "basd.bucket_mb=4"])
    trainer, _ = build(cfg, device="cpu")
    trainer.use_mixup = False
    trainer.optimizer.train()
    trainer.model.train()
    with torch.no_grad():      # distinct temperatures so that their gradients are not symmetric
        trainer.basd_loss.layer_selector.log_temperatures.add_(torch.linspace(-0.3, 0.3, 4))
    return trainer


def _shard(rank):
    from basd_amd.train import SyntheticLoader
    return next(iter(SyntheticLoader(8, 32, 100, 1, "cpu", seed=50 + rank)))


# CPU threads of a trainer rank, and of the single-process reference it is compared with: the gradients of the c1 step
# on CPU depend on the thread count at bf16 resolution (2 vs 16 threads: 86 % of the entries differ, the losses agree)
_WORKER_THREADS = 2


def _trainer_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(_WORKER_THREADS)
    trainer = _c1_trainer()
    assert trainer.reducer.enabled and trainer.reducer.world == 2 and len(trainer.reducer.buckets) >= 5
    assert not trainer.segmented          # the two-stage captured backward is opt-in (basd.segmented_backward)
    batch = _shard(rank)
    out = {}
    # path 1: bucket hooks fire during backward, finish() waits and averages
    loss, _ = trainer._forward_backward(batch["clean"], batch["augmented"], batch["label"])
    trainer.reducer.finish()
    out["loss"], out["grad_hooks"] = loss.clone(), trainer.flat.grad.clone()
    trainer.flat.zero_grad()
    # path 2: hooks paused (what a captured graph replay does), one all-reduce over the flat buffer
    trainer.reducer.paused = True
    trainer._forward_backward(batch["clean"], batch["augmented"], batch["label"])
    trainer.reducer.reduce_all()
    out["grad_all"] = trainer.flat.grad.clone()
    trainer.flat.zero_grad()
    # path 3: the two-stage backward of a captured multi-rank step -- stage 1 (loss ... block cut), the late slice of the
    # flat buffer all-reduced asynchronously, stage 2 (blocks below the cut) under it, then the early slice
    seg = trainer._segment_spec()
    assert seg is not None and 0 < seg["offset"] < trainer.flat.numel and seg["cut"] == 4
    trainer._forward_backward(batch["clean"], batch["augmented"], batch["label"], split=True)
    early_before = trainer.flat.grad[:seg["offset"]].clone()
    trainer.reducer.reduce_range_async(seg["offset"], trainer.flat.numel)
    trainer._backward_stage2()
    trainer.reducer.reduce_range_async(0, seg["offset"])
    trainer.reducer.wait_ranges()
    out["grad_split"] = trainer.flat.grad.clone()
    # stage 1 leaves the early slice untouched except for block cut's first norm (unfused CPU path: applied in stage 1)
    out["early_touched_in_stage1"] = int((early_before != 0).sum())
    trainer.reducer.paused = False
    n_t = trainer.basd_loss.layer_selector.log_temperatures.numel()
    out["temp_grad"] = trainer.basd_loss.layer_selector.log_temperatures.grad.clone()
    assert n_t == 4
    torch.save(out, os.path.join(out_dir, f"t{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_trainer_shards_losses_and_gradient_mean(tmp_path):
    port = _free_port()
    mp.spawn(_trainer_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(tmp_path / f"t{r}.pt") for r in range(2)]
    # single-process reference on each shard with the same (seeded) weights and the ranks' thread count
    from basd_amd.losses import _ops
    threads = torch.get_num_threads()
    torch.set_num_threads(_WORKER_THREADS)
    try:
        trainer = _c1_trainer()
        want_loss, want_grad = [], torch.zeros_like(trainer.flat.grad)
        for r in range(2):
            trainer.flat.zero_grad()
            b = _shard(r)
            loss, _ = trainer._forward_backward(b["clean"], b["augmented"], b["label"])
            want_loss.append(loss.clone())
            want_grad += trainer.flat.grad / 2
    finally:
        _ops.set_ops(None)
        torch.set_num_threads(threads)
    for r in range(2):
        torch.testing.assert_close(got[r]["loss"], want_loss[r], rtol=1e-6, atol=0)       # (i) per-rank loss on its shard
        torch.testing.assert_close(got[r]["grad_hooks"], want_grad, rtol=1e-5, atol=1e-7)  # (ii) finish()
        torch.testing.assert_close(got[r]["grad_all"], want_grad, rtol=1e-5, atol=1e-7)    # (ii) reduce_all()
        torch.testing.assert_close(got[r]["grad_split"], want_grad, rtol=1e-5, atol=1e-7)  # (ii) two-stage backward
        assert got[r]["early_touched_in_stage1"] <= 2 * 192
    torch.testing.assert_close(got[0]["grad_hooks"], got[1]["grad_hooks"], rtol=0, atol=0)
    # (iii) the four temperatures sit in the same flat buffer: averaged, identical on both ranks, and not zero
    torch.testing.assert_close(got[0]["temp_grad"], got[1]["temp_grad"], rtol=0, atol=0)
    torch.testing.assert_close(got[0]["temp_grad"], want_grad[-64:][:4], rtol=1e-5, atol=1e-9)
    assert float(got[0]["temp_grad"].abs().max()) > 0

"""Entry points in child processes: ``python -m basd_amd.eval`` on a ``Trainer.save_weights`` checkpoint and a local
``.npz`` dataset, and a ``BASD_STRICT=1`` training run whose start-up probes and evaluations take the fp32 "high" route."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")


def _env(**extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.update(extra)
    return env


def _run(args, timeout, **env):
    res = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, *args], cwd=ROOT, env=_env(**env),
                         capture_output=True, text=True)
    assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    return res.stdout


def _dataset(root, n_classes=10):
    g = np.random.default_rng(0)
    names = np.array([f"c{i}" for i in range(n_classes)])
    for split, n in (("train", 64), ("validation", 40)):
        imgs = g.integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8)
        labels = g.integers(0, n_classes, size=n).astype(np.int64)
        np.savez(root / f"{split}.npz", images=imgs, labels=labels, class_names=names)


def test_eval_entry_point_writes_metrics(tmp_path):
    from basd_amd.config import load_config
    from basd_amd.data import create_eval_loader, get_channel_stats
    from basd_amd.evaluation import evaluate_model, matmul_precision
    from basd_amd.losses import _ops
    from basd_amd.models.vit import create_vit
    from basd_amd.train import build
    _ops.set_ops(None)
    data = tmp_path / "data"
    data.mkdir()
    _dataset(data)
    overrides = [f"data.dataset={data}", "data.batch_size=16", f"run.output_dir={tmp_path / 'out'}", "run.name=ev",
                 "model.drop_path_rate=0.0"]
    cfg = load_config(CFG, "basd_cifar100", overrides)
    torch.manual_seed(0)
    trainer, _ = build(cfg, device="cuda")
    trainer.save_weights("w.pt", 3)
    ckpt = tmp_path / "out" / "ev" / "checkpoints" / "w.pt"
    assert ckpt.exists()
    out = _run(["-m", "basd_amd.eval", "--experiment", "basd_cifar100", *overrides, f"checkpoint.path={ckpt}"], 600)
    assert f"checkpoint_loaded path={ckpt} epoch=3" in out
    metrics = json.loads((tmp_path / "out" / "ev" / "metrics.json").read_text())
    assert set(metrics) == {"run", "primary", "robustness", "efficiency"}
    assert set(metrics["primary"]) == {"dataset", "val_acc", "val_acc_top5", "loss"}
    assert set(metrics["efficiency"]) == {"param_count", "param_count_m", "gflops", "throughput_img_per_sec"}
    assert (tmp_path / "out" / "ev" / "config.yaml").exists()
    # the same evaluation in this process
    model = create_vit(cfg.model.student_preset, num_classes=cfg.model.num_classes, img_size=cfg.model.vit.img_size,
                       patch_size=cfg.model.vit.patch_size).cuda()
    model.load_state_dict(torch.load(ckpt, map_location="cuda", weights_only=True)["model_state_dict"])
    mean, std = get_channel_stats(str(data))
    val = create_eval_loader(str(data), image_size=32, batch_size=16, mean=mean, std=std,
                             crop_ratio=float(cfg.data.eval_crop_ratio), num_workers=0)
    with matmul_precision("high"):
        want = evaluate_model(model, val, torch.nn.CrossEntropyLoss(), num_classes=cfg.model.num_classes)
    assert metrics["primary"]["val_acc"] == want["val_acc"]


def test_eval_entry_point_rejects_a_hub_dataset(tmp_path):
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "basd_amd.eval", "data.dataset=cifar100",
                          "model.num_classes=100", f"checkpoint.path={tmp_path / 'x.pt'}"], cwd=ROOT, env=_env(),
                         capture_output=True, text=True)
    assert res.returncode != 0 and "not a local directory" in res.stderr


def test_strict_training_run_starts_and_evaluates(tmp_path):
    out = _run(["-m", "basd_amd.train", "--experiment", "basd_cifar100", "--steps-per-epoch", "2", "data.dataset=synthetic",
                "training.num_epochs=1", "model.num_classes=100", "data.batch_size=16",
                "basd.teacher_model_name=vit_small_patch16_224", "basd.teacher_patch_size=4",
                f"run.output_dir={tmp_path}"], 900, BASD_STRICT="1")
    assert "metrics_json=" in out

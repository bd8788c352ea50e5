"""Evaluation entry point (reference ``src/eval.py``): ``python -m basd_amd.eval [--config ...] [--experiment ...]
a.b=c ...``.  Builds the student from ``model.student_preset`` + ``model.arch_overrides`` + ``model.vit.patch_size``,
loads ``checkpoint.path`` (the ``{"epoch", "model_state_dict"}`` file ``Trainer.save_weights`` writes), saves the
resolved ``config.yaml`` and runs the evaluation suite on the local evaluation split into ``metrics.json``.  Everything
runs under ``torch.set_float32_matmul_precision("high")`` as in the reference: the fp32 forward on the split-bf16 kernels."""
from __future__ import annotations

import argparse
import json
import os
from pathlib import Path

import torch

from .config import load_config
from .evaluation import matmul_precision, run_eval_suite, save_metrics
from .models.vit import create_vit


def _plain(x):
    return {k: _plain(v) for k, v in x.items()} if isinstance(x, dict) else [_plain(v) for v in x] \
        if isinstance(x, list) else x


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(os.path.dirname(__file__), "configs", "config.yaml"))
    ap.add_argument("--experiment", default=None)
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    config = load_config(args.config, args.experiment, args.overrides)
    from .data import create_eval_loader, get_channel_stats, is_local_dataset
    if not is_local_dataset(config.data.dataset):
        # as train.py: the reference configurations name hub datasets, which need the network
        raise SystemExit(f"data.dataset={config.data.dataset!r} is not a local directory (hub datasets need the network)")
    if not config.checkpoint.get("path"):
        raise SystemExit("checkpoint.path is required")
    with matmul_precision("high"):
        torch.manual_seed(config.run.seed)
        model = create_vit(config.model.student_preset, num_classes=config.model.num_classes,
                           img_size=config.model.vit.img_size, patch_size=config.model.vit.patch_size,
                           **dict(config.model.get("arch_overrides") or {})).cuda()
        ckpt = torch.load(config.checkpoint.path, map_location="cuda", weights_only=True)
        model.load_state_dict(ckpt["model_state_dict"])
        print(f"checkpoint_loaded path={config.checkpoint.path} epoch={ckpt['epoch']}")
        output_dir = Path(config.run.output_dir) / config.run.name
        output_dir.mkdir(parents=True, exist_ok=True)
        cfg_path = output_dir / "config.yaml"
        cfg_path.write_text(json.dumps(_plain(config), indent=2))      # JSON is YAML
        name = config.data.dataset
        mean, std = get_channel_stats(name)
        val = create_eval_loader(name, image_size=config.model.vit.img_size, batch_size=config.data.batch_size,
                                 mean=mean, std=std, crop_ratio=float(config.data.eval_crop_ratio))
        loaders = {name: val}
        for extra in config.data.get("eval_datasets") or []:
            if not is_local_dataset(extra):
                raise SystemExit(f"data.eval_datasets: {extra!r} is not a local directory")
            loaders[extra] = create_eval_loader(extra, image_size=config.model.vit.img_size,
                                                batch_size=config.data.batch_size, mean=mean, std=std,
                                                crop_ratio=float(config.data.eval_crop_ratio))
        results = run_eval_suite(model, config, config_path=str(cfg_path), loaders=loaders)
    print(f"metrics_json={save_metrics(results, output_dir)}")


if __name__ == "__main__":
    main()

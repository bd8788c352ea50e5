"""The ConvNeXt-V2 teacher on the device: the fused trunk against the fp64 restatement (tests/_convnext_ref.py) with
the module's own plain-torch bf16 channels-last forward (library convolutions) as the yardstick, a strict-mode training
step built from the cross-arch overlay, and the start-up path (intrinsic dimension, derived student)."""
import os

import pytest
import torch

from tests import _convnext_ref as R
from tests._teacher_cases import bf16_frozen, fused_and_library, images as _images

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")


def _check_trunk(model, depths, x, label):
    fused, lib = fused_and_library(model, x)
    assert fused.shape == lib.shape and fused.shape[1] > fused.shape[3]
    want = R.tokens(R.forward_features(model.state_dict(), x.to(torch.bfloat16), depths))
    e_f = R.rel_l2_per_sample(R.tokens(fused.float().cpu()), want)
    e_l = R.rel_l2_per_sample(R.tokens(lib.float().cpu()), want)
    print(f"{label}: per-sample rel-L2 vs fp64: fused {[f'{v:.3e}' for v in e_f.tolist()]}, "
          f"library bf16 {[f'{v:.3e}' for v in e_l.tolist()]}")
    assert bool((e_f <= 2.0 * e_l).all()), (e_f.tolist(), e_l.tolist())


@pytest.mark.parametrize("depths,dims", [((1, 1, 2, 1), (96, 192, 384, 768)), ((1, 1, 1, 1), (128, 256, 512, 1024))],
                         ids=["tiny-widths", "base-widths"])
def test_small_trunk_at_128px_against_fp64(depths, dims):
    """random biases and LayerNorm parameters (tests/_convnext_ref.py::randomise_affine): the bias images and the
    gamma / beta wiring of the fused path carry weight in the result"""
    from basd_amd.models.convnext import ConvNeXtV2
    torch.manual_seed(0)
    model = bf16_frozen(R.randomise_affine(ConvNeXtV2(depths, dims), seed=7).cuda(), memory_format=torch.channels_last)
    assert model.prepare_fused()
    _check_trunk(model, depths, _images(2, 128, seed=1), f"small trunk {dims[0]}..{dims[-1]} 128 px")


def test_convnextv2_tiny_at_224px_against_fp64():
    from basd_amd.models import extract_intermediates, load_teacher
    teacher = load_teacher("convnextv2_tiny.fcmae", 224, device="cuda")
    assert teacher.model._fused is not None
    R.randomise_affine(teacher.model, seed=9)                  # in place on the bf16 / fp32 device parameters ...
    assert teacher.model.prepare_fused()                       # ... so the weight images are rebuilt from them
    x = _images(2, 224, seed=2)
    _check_trunk(teacher.model, (3, 3, 9, 3), x, "convnextv2_tiny 224 px")
    tok, imp = extract_intermediates(teacher, x.cuda())
    assert list(tok) == [0] and tok[0].shape == (2, 49, 768) and tok[0].is_contiguous()
    assert torch.equal(imp[0], torch.full((2, 49), 1.0 / 49, device="cuda"))


def test_cross_arch_overlay_trains_a_strict_step_on_the_own_kernels():
    """DeiT-Tiny/16 against convnextv2_tiny.fcmae, built through train.build from the overlay: no fallback, no library
    GEMM call site in the teacher branch, the two-stream gate finds nothing to refuse"""
    import basd_amd.losses._ops as O
    from basd_amd.config import load_config
    from basd_amd.train import SyntheticLoader, build
    torch.manual_seed(0)
    cfg = load_config(CFG, "basd_imagenet_cross_arch", ["data.batch_size=8", "data.dataset=synthetic",
                                                       "model.student_preset=deit_tiny_patch16_224",
                                                       "model.vit.img_size=224", "model.vit.patch_size=16",
                                                       "model.drop_path_rate=0.0"])
    assert cfg.basd.teacher_model_name == "convnextv2_tiny.fcmae"
    trainer, _ = build(cfg, device="cuda")
    trainer.use_mixup = False
    trainer.optimizer.train()
    trainer.model.train()
    b = next(iter(SyntheticLoader(8, 224, cfg.model.num_classes, 1, "cuda", seed=5)))
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with torch.no_grad(), O.record_library_gemms() as seen:
            trainer._teacher_branch(b["clean"])
        trainer.basd_loss.layer_selector._frames = None
        torch.cuda.synchronize()
        assert not seen, seen
        loss, _ = trainer.train_step(b)
        trainer.check_health()
    finally:
        O.set_strict(False)
    assert torch.isfinite(loss.detach()).all()
    assert not O.FALLBACKS, dict(O.FALLBACKS)
    assert trainer.two_stream_refused is None


def test_startup_path_on_the_convnext_teacher():
    from basd_amd.models import estimate_intrinsic_dim, load_teacher
    from basd_amd.train import _derive_from_teacher
    teacher = load_teacher("convnextv2_tiny.fcmae", 224, device="cuda")
    calib = _images(16, 224, seed=3).cuda()
    k = estimate_intrinsic_dim(teacher, calib)
    assert 1 <= k <= 768, k
    arch = _derive_from_teacher(teacher, k)
    assert arch["embed_dim"] == 768 and arch["num_heads"] == 1 and arch["depth"] == 4   # one head of 768: whole heads

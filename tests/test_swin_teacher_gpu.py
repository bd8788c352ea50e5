"""The Swin teacher on the device: the fused trunk against the fp64 restatement (tests/_swin_ref.py) with the module's
own plain-torch bf16 forward (library GEMMs) as the yardstick, a strict-mode training step of a DeiT-Tiny student
against it, and the start-up path (intrinsic dimension, derived student)."""
import os

import pytest
import torch

from tests import _swin_ref as R
from tests._teacher_cases import bf16_frozen, fused_and_library, images as _images

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
SWIN_T = "swin_tiny_patch4_window7_224"


def _check_trunk(model, depths, heads, ws, x, label):
    fused, lib = fused_and_library(model, x)
    assert fused.shape == lib.shape and fused.shape[3] == model.embed_dim and fused.shape[1] == x.shape[2] // 32
    want = R.tokens(R.forward_features(model.state_dict(), x.to(torch.bfloat16), depths, heads, ws))
    e_f = R.rel_l2_per_sample(R.tokens(fused.float().cpu()), want)
    e_l = R.rel_l2_per_sample(R.tokens(lib.float().cpu()), want)
    print(f"{label}: per-sample rel-L2 vs fp64: fused {[f'{v:.3e}' for v in e_f.tolist()]}, "
          f"library bf16 {[f'{v:.3e}' for v in e_l.tolist()]}")
    assert bool((e_f <= 2.0 * e_l).all()), (e_f.tolist(), e_l.tolist())


@pytest.mark.parametrize("dims,heads", [((96, 192, 384, 768), (3, 6, 12, 24)), ((128, 256, 512, 1024), (4, 8, 16, 32))],
                         ids=["tiny-widths", "base-widths"])
def test_small_trunk_at_128px_against_fp64(dims, heads):
    """window 4 at 128 px: grids 32, 16, 8, 4 -- a shifted block in every stage but the last; random biases, LayerNorm
    parameters, bias tables and unit-scale attention weights (tests/_swin_ref.py::randomise_affine), so the bias
    images, the gamma / beta wiring, the window index and the mask of the fused path carry weight in the result"""
    from basd_amd.models.swin import SwinTransformer
    depths = (2, 2, 2, 2)
    torch.manual_seed(0)
    model = bf16_frozen(R.randomise_affine(SwinTransformer(depths, dims, heads, window_size=4), seed=7).cuda())
    assert model.fused_refusal() is None and model.prepare_fused()
    _check_trunk(model, depths, heads, 4, _images(2, 128, seed=1), f"small trunk {dims[0]}..{dims[-1]} 128 px")


def test_swin_tiny_at_224px_against_fp64():
    from basd_amd.models import extract_intermediates, load_teacher
    teacher = load_teacher(SWIN_T + ".ms_in1k", 224, device="cuda")
    assert teacher.model._fused is not None and teacher.feature_format == "nhwc" and teacher.embed_dim == 768
    R.randomise_affine(teacher.model, seed=9)                  # in place on the bf16 / fp32 device parameters ...
    assert teacher.model.prepare_fused()                       # ... so the weight images are rebuilt from them
    x = _images(2, 224, seed=2)
    _check_trunk(teacher.model, (2, 2, 6, 2), (3, 6, 12, 24), 7, x, "swin_tiny 224 px")
    tok, imp = extract_intermediates(teacher, x.cuda())
    assert list(tok) == [0] and tok[0].shape == (2, 49, 768) and tok[0].is_contiguous()
    assert torch.equal(imp[0], torch.full((2, 49), 1.0 / 49, device="cuda"))


def test_deit_tiny_trains_a_strict_step_against_the_swin_teacher():
    """DeiT-Tiny/16 against swin_tiny, built through train.build: no fallback, no library GEMM call site in the teacher
    branch, the two-stream gate finds nothing to refuse"""
    import basd_amd.losses._ops as O
    from basd_amd.config import load_config
    from basd_amd.train import SyntheticLoader, build
    torch.manual_seed(0)
    cfg = load_config(CFG, None, ["data.batch_size=8", "data.dataset=synthetic", f"basd.teacher_model_name={SWIN_T}",
                                  "model.student_preset=deit_tiny_patch16_224", "model.vit.img_size=224",
                                  "model.vit.patch_size=16", "model.drop_path_rate=0.0"])
    trainer, _ = build(cfg, device="cuda")
    assert trainer._teacher.model._fused is not None
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


def test_startup_path_on_the_swin_teacher():
    from basd_amd.models import estimate_intrinsic_dim, load_teacher
    from basd_amd.train import _derive_from_teacher
    teacher = load_teacher(SWIN_T, 224, device="cuda")
    calib = _images(16, 224, seed=3).cuda()
    k = estimate_intrinsic_dim(teacher, calib)
    assert 1 <= k <= 768, k
    arch = _derive_from_teacher(teacher, k)
    assert arch["embed_dim"] == 768 and arch["num_heads"] == 1 and arch["depth"] == 4   # one head of 768: whole heads

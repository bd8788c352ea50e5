"""The window-12 Swin teacher on the device (as tests/test_swin_teacher_gpu.py for window 7): the fused trunk, whose every
block takes basd_window_attention_fwd_wide_bf16, against the fp64 restatement (tests/_swin_ref.py) with the module's own
plain-torch bf16 forward as the yardstick; the 384 px preset through ``load_teacher`` and the tap; a strict-mode training
step of a DeiT-Tiny student at 384 px against it."""
import os

import pytest
import torch

from tests import _swin_ref as R
from tests._teacher_cases import bf16_frozen, fused_and_library, images as _images

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
SWIN_B_384 = "swin_base_patch4_window12_384"


def test_window_12_trunk_at_384px_against_fp64():
    """384 px is the smallest image at which window 12 fits the last stage: grids 96, 48, 24, 12 -- a shifted block in
    every stage but the last; random biases, LayerNorm parameters, bias tables and unit-scale attention weights
    (tests/_swin_ref.py::randomise_affine), so the tables, the index arithmetic and the mask of the wide kernel carry
    weight in the result.  Per-sample rel-L2 against fp64: fused <= 2 x the library bf16 path."""
    from basd_amd.models.swin import SwinTransformer
    depths, dims, heads = (2, 2, 2, 2), (96, 192, 384, 768), (3, 6, 12, 24)
    torch.manual_seed(0)
    model = bf16_frozen(R.randomise_affine(SwinTransformer(depths, dims, heads, window_size=12), seed=7).cuda())
    assert model.fused_refusal() is None and model.prepare_fused()
    assert model._fused["stages"][0]["blocks"][1]["bias"].shape == (529, 3)
    x = _images(2, 384, seed=1)
    fused, lib = fused_and_library(model, x)
    assert fused.shape == lib.shape == (2, 12, 12, 768)
    want = R.tokens(R.forward_features(model.state_dict(), x.to(torch.bfloat16), depths, heads, 12))
    e_f = R.rel_l2_per_sample(R.tokens(fused.float().cpu()), want)
    e_l = R.rel_l2_per_sample(R.tokens(lib.float().cpu()), want)
    print(f"window-12 trunk 384 px: per-sample rel-L2 vs fp64: fused {[f'{v:.3e}' for v in e_f.tolist()]}, "
          f"library bf16 {[f'{v:.3e}' for v in e_l.tolist()]}")
    assert bool((e_f <= 2.0 * e_l).all()), (e_f.tolist(), e_l.tolist())


def test_swin_base_384_loads_and_taps():
    from basd_amd.models import extract_intermediates, load_teacher
    teacher = load_teacher(SWIN_B_384 + ".ms_in22k_ft_in1k", 384, device="cuda")
    assert teacher.model._fused is not None and teacher.feature_format == "nhwc" and teacher.embed_dim == 1024
    tok, imp = extract_intermediates(teacher, _images(2, 384, seed=2).cuda())
    assert list(tok) == [0] and tok[0].shape == (2, 144, 1024) and tok[0].is_contiguous()
    assert bool(torch.isfinite(tok[0].float()).all())
    assert torch.equal(imp[0], torch.full((2, 144), 1.0 / 144, device="cuda"))


def test_deit_tiny_at_384px_trains_a_strict_step_against_the_window_12_teacher():
    """DeiT-Tiny/16 at 384 px (576 tokens) against swin_base_patch4_window12_384, built through train.build: no
    fallback, no library GEMM call site in the teacher branch, the two-stream gate finds nothing to refuse"""
    import basd_amd.losses._ops as O
    from basd_amd.config import load_config
    from basd_amd.train import SyntheticLoader, build
    torch.manual_seed(0)
    cfg = load_config(CFG, None, ["data.batch_size=8", "data.dataset=synthetic", f"basd.teacher_model_name={SWIN_B_384}",
                                  "model.student_preset=deit_tiny_patch16_224", "model.vit.img_size=384",
                                  "model.vit.patch_size=16", "model.drop_path_rate=0.0"])
    trainer, _ = build(cfg, device="cuda")
    assert trainer._teacher.model._fused is not None and trainer._teacher.model.window_size == 12
    trainer.use_mixup = False
    trainer.optimizer.train()
    trainer.model.train()
    b = next(iter(SyntheticLoader(8, 384, cfg.model.num_classes, 1, "cuda", seed=5)))
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

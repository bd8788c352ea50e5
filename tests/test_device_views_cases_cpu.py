"""The cases of tests/test_device_views_gpu.py leave its "one level" tolerance room: checked here, on the CPU, before any
kernel runs.

* Colour ops: an fp64 restatement of each op against the fp32 CPU function (the oracle) on the chosen inputs.  A case is
  one (op, magnitude) on the four input images.  Observed worst shares of pixels one level off (none is off by more),
  cap 1 %: S = 32: Brightness 0.55 % (magnitude -0.99: 0.01 x has exact .5 ties at x = 50, 150, 250), Sharpness 0.04 %,
  AutoContrast 0.06 %, Color 0, Contrast 0; S = 224: Sharpness 0.04 %, AutoContrast 0.08 %, Contrast 0.
* Affine ops: the share of pixels left out of the exact comparison (fp64 source coordinate within 1e-3 of a rounding
  boundary, exact ties excepted) at the chosen magnitudes, cap 1 %.  Observed: 0 for ShearX / ShearY, 0.39 % for Rotate by
  +-67.5 degrees at S = 32 and 0.40 % at S = 224, 0 for +-135 degrees (there 6.25 % / 0.89 % of the pixels are exact
  ties, which stay in the comparison).
"""
import pytest
import torch

from tests import _dual_view_cases as C


@pytest.mark.parametrize("s", [32, 224])
def test_fp64_restatement_of_the_colour_ops_stays_under_the_cap(s):
    from basd_amd.data import transforms as T
    imgs = C.ta_inputs(s)
    big = ("Contrast", "Sharpness", "AutoContrast")
    for op_id, mag in C.ta_cases():
        op = T.TA_WIDE_OPS[op_id]
        if op not in C.COLOUR_OPS or (s == 224 and op not in big):
            continue
        got = torch.stack([C.colour_op_fp64(img, op, mag) for img in imgs])
        want = torch.stack([C.ta_oracle(img, op_id, mag) for img in imgs])
        worst, share = C.one_level_report(got, want)
        print(f"S={s} {op} {mag:+.3f}: max {worst}, share {100 * share:.4f} %")
        assert worst <= 1 and share <= C.ONE_LEVEL_CAP, (op, mag, worst, share)


@pytest.mark.parametrize("s", [32, 224])
def test_affine_cases_leave_out_less_than_one_percent(s):
    from basd_amd.data import transforms as T
    for op_id, mag in C.ta_cases():
        op = T.TA_WIDE_OPS[op_id]
        if op not in C.AFFINE_OPS or (s == 224 and op != "Rotate"):
            continue
        share = float(C.affine_boundary_mask(s, op, mag).double().mean())
        print(f"S={s} {op} {mag:+.3f}: {100 * share:.4f} % near a rounding boundary")
        assert share < 0.01, (op, mag, share)


def test_inputs_hold_the_degenerate_channels():
    imgs = C.ta_inputs(32)
    assert int(imgs[2, 1].min()) == int(imgs[2, 1].max())                  # constant channel
    assert imgs[3].unique().numel() == 2                                   # two-valued image
    from basd_amd.data import transforms as T
    assert torch.equal(T.autocontrast(imgs[2])[1], imgs[2, 1]) and torch.equal(T.equalize(imgs[2])[1], imgs[2, 1])
    ops = {op for op, _ in C.ta_cases()}
    assert ops == set(range(len(T.TA_WIDE_OPS)))

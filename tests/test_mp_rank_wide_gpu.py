"""``marchenko_pastur_rank_wide`` (fp64 Gram -> Householder tridiagonal form -> Sturm counts, csrc/tridiag.hip) past
the 1024-value limit of ``marchenko_pastur_rank``, and the start-up path on the teacher that needs it (ViT-H/14, 1280
channels: reference src/train.py:88-106, src/models/teacher.py:161-177).

The reference of every rank is the definition (reference layer_selector.py:8-20) in fp64 numpy on the same fp32
tokens; every case first asserts, on that reference spectrum alone, that no eigenvalue lies within 1e-6 (relative) of
the edge -- closer than that, the count is a matter of rounding and no implementation is wrong."""
import numpy as np
import pytest
import torch

from tests import _tridiag_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native_provider():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    native.lib()
    _ops.set_ops(None)
    native.status_word("cuda").zero_()
    yield


@pytest.mark.parametrize("m,d,r", C.WIDE_CASES)
def test_wide_rank_is_the_fp64_count(m, d, r):
    from basd_amd.losses import _ops, marchenko_pastur_rank_wide
    x, _g, lam = C.case(m, d, r)
    want, gap = C.direct_mp_rank(lam, m, d)
    print(f"mp-rank-wide ({m}, {d}, {r}): reference rank {want}, nearest eigenvalue {gap:.2e} (relative) from the edge")
    assert gap >= C.GAP
    xd = x.cuda()
    with _ops.record_library_gemms() as seen:
        got = marchenko_pastur_rank_wide(xd)
    assert isinstance(got, int) and got == want, (got, want)
    assert not seen, seen                                   # own kernels only: no library GEMM is enqueued
    import basd_amd._native as native
    assert int(native.status_word("cuda").item()) == 0


def test_wide_rank_refuses_more_than_2048_on_both_sides():
    from basd_amd.losses import marchenko_pastur_rank_wide
    from basd_amd.losses.functional import BasdShapeError
    with pytest.raises(BasdShapeError, match="2048"):
        marchenko_pastur_rank_wide(torch.zeros(2049, 2049, device="cuda"))
    with pytest.raises(BasdShapeError, match="2048"):
        marchenko_pastur_rank_wide(torch.zeros(2100, 2049, device="cuda"))


def test_pure_noise_and_nonfinite_tokens_raise_the_status_word():
    import basd_amd._native as native
    from basd_amd.losses import marchenko_pastur_rank_wide
    x = torch.zeros(128, 64, device="cuda")
    x[:64] = torch.eye(64, device="cuda")                   # Gram = identity: nothing above the edge
    assert marchenko_pastur_rank_wide(x) == 0
    assert int(native.status_word("cuda").item()) == native.STATUS_RANK0
    native.status_word("cuda").zero_()
    x[5, 7] = float("nan")
    assert marchenko_pastur_rank_wide(x) == 0
    assert int(native.status_word("cuda").item()) == native.STATUS_NONFINITE
    native.status_word("cuda").zero_()


def test_startup_on_vit_huge():
    """100 calibration images of 56 px at patch 14 = 16 tokens each: a [1600, 1280] token matrix, which
    ``marchenko_pastur_rank`` refuses (both sides > 1024)"""
    from basd_amd.models import estimate_intrinsic_dim, extract_intermediates, load_teacher
    from basd_amd.train import _derive_from_teacher
    teacher = load_teacher("vit_huge_patch14_224", 56, device="cuda", patch_size=14)
    assert teacher.embed_dim == 1280
    calib = torch.randn(100, 3, 56, 56, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    k = estimate_intrinsic_dim(teacher, calib)
    tokens, _ = extract_intermediates(teacher, calib)
    x = tokens[max(tokens)].reshape(-1, teacher.embed_dim).float().cpu()
    assert tuple(x.shape) == (1600, 1280)
    want, gap = C.direct_mp_rank(np.linalg.eigvalsh(C.gram64(x)), 1600, 1280)
    print(f"vit-huge start-up: reference rank {want}, nearest eigenvalue {gap:.2e} (relative) from the edge, got {k}")
    assert gap >= C.GAP
    assert isinstance(k, int) and k == want, (k, want)
    arch = _derive_from_teacher(teacher, k)
    assert arch["embed_dim"] % 80 == 0 and arch["embed_dim"] <= 1280
    assert arch["num_heads"] == arch["embed_dim"] // 80 and arch["depth"] == teacher.depth

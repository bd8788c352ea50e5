"""The tiled fp32 split-bf16 evaluation attention entry (basd_attention_fwd_f32x3_long) on a CPU-only machine: exported
with the argument types of include/basd_hip.h, argument checks that return their status before anything touches a
device, the predicates of the binding, and the block predicate of the model at 577 tokens."""
import ctypes
import os
import re

import pytest

NAME = "basd_attention_fwd_f32x3_long"
BASD_ERR_SHAPE = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "basd_hip.h")
_CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p,
          "const float*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


@pytest.fixture(scope="module")
def lib():
    import basd_amd._native as native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_exported_with_the_header_signature(lib):
    import basd_amd._native as native
    assert NAME in native.EXPORTS and hasattr(lib, NAME)
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\);", open(HEADER).read())
    assert m
    args = [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]
    assert args == ["const float*", "int", "int", "int", "int", "float", "void*", "void*"]
    assert tuple(_CTYPE[a] for a in args) == native._SIGNATURES[NAME]
    assert native._SIGNATURES[NAME] == native._SIGNATURES["basd_attention_fwd_f32x3"]
    assert getattr(lib, NAME).restype == ctypes.c_int


def _fwd(lib, T, hd, B=2, H=3):
    p = ctypes.c_void_p(4096)                               # never dereferenced on the host
    return getattr(lib, NAME)(p, B, T, H, hd, ctypes.c_float(0.125), p, ctypes.c_void_p(0))


def test_refuses_bad_shapes(lib):
    for T, hd in [(0, 64), (1025, 64), (577, 96), (577, 32)]:
        assert _fwd(lib, T, hd) == BASD_ERR_SHAPE, (T, hd)
        assert b"attention_fwd_f32x3_long" in lib.basd_last_error()
    assert _fwd(lib, 577, 64, H=0) == BASD_ERR_SHAPE
    assert b"attention_fwd_f32x3_long" in lib.basd_last_error()


def test_empty_batch_is_a_no_op(lib):
    assert _fwd(lib, 577, 64, B=0) == 0
    assert _fwd(lib, 577, 80, B=0) == 0


def test_predicates():
    import basd_amd._native as native
    for t in (1, 272, 273, 577, 730, 1024):
        for hd in (64, 80):
            assert native.attention_fwd_f32x3_long_supported(t, hd), (t, hd)
    for t, hd in [(0, 64), (1025, 64), (577, 96)]:
        assert not native.attention_fwd_f32x3_long_supported(t, hd), (t, hd)
    # the short predicate keeps its meaning: the single-pass kernel
    assert native.attention_fwd_f32x3_supported(272, 64) and not native.attention_fwd_f32x3_supported(273, 64)


def test_block_accepts_577_tokens(lib):
    from basd_amd.losses import _ops
    from basd_amd.models.vit import create_vit
    _ops.set_ops(None)
    model = create_vit("deit_tiny_patch16_224", num_classes=100, img_size=384)
    assert model.pos_embed.shape[1] == 577
    blk = model.blocks[0]
    assert blk._f32x3_supported(197) and blk._f32x3_supported(577) and blk._f32x3_supported(1024)
    assert not blk._f32x3_supported(1025)

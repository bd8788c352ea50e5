"""The long-sequence attention entries (csrc/attention_long.hip) on a CPU-only machine: exported with the argument types
of include/basd_hip.h, a workspace query that grows with the shape, and argument checks that return their status
before anything touches a device."""
import ctypes
import os
import re

import pytest

NAMES = ("basd_attention_fwd_long_bf16", "basd_attention_bwd_long_workspace_bytes", "basd_attention_bwd_long_bf16")
BASD_ERR_SHAPE, BASD_ERR_WORKSPACE = 1, 3
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
    text = open(HEADER).read()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name)
        m = re.search(r"\b(int|int64_t) " + name + r"\(([^)]*)\);", text)
        assert m, name
        args = [" ".join(a.split()[:-1]) for a in m.group(2).split(",")]
        assert tuple(_CTYPE[a] for a in args) == native._SIGNATURES[name], name
        assert getattr(lib, name).restype == (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int)


def test_workspace_query_grows(lib):
    ws = lib.basd_attention_bwd_long_workspace_bytes
    assert ws(2, 257, 3, 64) > 0
    assert ws(4, 257, 3, 64) > ws(2, 257, 3, 64)
    assert ws(2, 577, 3, 64) > ws(2, 257, 3, 64)
    assert ws(2, 257, 3, 80) > ws(2, 257, 3, 64)
    assert ws(2, 257, 6, 64) > ws(2, 257, 3, 64)
    # delta [B, H, T] plus one fp32 dQ partial per 128-key block
    assert ws(1, 1024, 1, 64) >= 1024 * 4 + 8 * 1024 * 64 * 4


def _fwd(lib, T, hd, cls=False, qmean=False, out=True, lse=False, B=2, H=3):
    p = lambda on: ctypes.c_void_p(4096 if on else 0)       # never dereferenced on the host
    return lib.basd_attention_fwd_long_bf16(p(True), B, T, H, hd, ctypes.c_float(0.125), p(out), p(cls), p(qmean),
                                            p(lse), p(False))


def _bwd(lib, T, hd, ws_bytes, B=2, H=3):
    p = ctypes.c_void_p(4096)
    ws = p if ws_bytes else ctypes.c_void_p(0)
    return lib.basd_attention_bwd_long_bf16(p, p, p, p, B, T, H, hd, ctypes.c_float(0.125), p, ws,
                                            ctypes.c_int64(ws_bytes), ctypes.c_void_p(0))


def test_forward_refuses_bad_shapes(lib):
    for T, hd in [(0, 64), (1025, 64), (257, 96), (257, 32), (2048, 80)]:
        assert _fwd(lib, T, hd) == BASD_ERR_SHAPE, (T, hd)
        assert b"attention_fwd_long" in lib.basd_last_error()
    assert _fwd(lib, 257, 64, H=0) == BASD_ERR_SHAPE
    assert _fwd(lib, 1, 64, cls=True) == BASD_ERR_SHAPE              # the CLS tap needs a second token
    assert _fwd(lib, 300, 64, qmean=True, lse=False) == BASD_ERR_SHAPE   # the query-mean tap reads the LSE back
    assert _fwd(lib, 300, 64, qmean=True, lse=True, out=False) == BASD_ERR_SHAPE


def test_backward_refuses_bad_shapes_and_short_workspace(lib):
    big = 1 << 40
    for T, hd in [(0, 64), (1025, 64), (257, 96)]:
        assert _bwd(lib, T, hd, big) == BASD_ERR_SHAPE, (T, hd)
        assert b"attention_bwd_long" in lib.basd_last_error()
    need = lib.basd_attention_bwd_long_workspace_bytes(2, 577, 3, 80)
    assert _bwd(lib, 577, 80, need - 1) == BASD_ERR_WORKSPACE
    assert _bwd(lib, 577, 80, 0) == BASD_ERR_WORKSPACE
    assert b"workspace" in lib.basd_last_error()


def test_empty_batches_are_no_ops(lib):
    assert _fwd(lib, 257, 64, B=0) == 0
    assert _bwd(lib, 257, 64, 0, B=0) == 0


def test_predicates_widen_and_keep_the_short_ranges():
    import basd_amd._native as native
    for t in (1, 197, 257, 577, 1024):
        for hd in (64, 80):
            assert native.attention_fwd_supported(t, hd) and native.attention_bwd_supported(t, hd)
            assert native.cls_importance_supported(t, hd) == (t >= 2)
    for t, hd in [(0, 64), (1025, 64), (257, 96)]:
        assert not native.attention_fwd_supported(t, hd) and not native.attention_bwd_supported(t, hd)
    assert native.cls_importance_supported(300, 32) and not native.cls_importance_supported(321, 32)
    # the fp32 evaluation attention keeps its range: no long kernel there
    assert native.attention_fwd_f32x3_supported(272, 64) and not native.attention_fwd_f32x3_supported(273, 64)
    assert native._short_attention_fwd_ok(272, 80) and not native._short_attention_fwd_ok(273, 80)
    assert native._short_attention_bwd_ok(224, 64) and not native._short_attention_bwd_ok(197, 80)

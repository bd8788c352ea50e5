"""The selector forward entries (basd_selector_frames / basd_selector_weights) on a CPU-only machine: exported, workspace
queries that grow with the shape, and argument checks that return before anything touches a device."""
import ctypes

import pytest

NAMES = ("basd_selector_frames_workspace_bytes", "basd_selector_frames", "basd_selector_weights_workspace_bytes",
         "basd_selector_weights")
BASD_ERR_SHAPE, BASD_ERR_WORKSPACE = 1, 3


@pytest.fixture(scope="module")
def lib():
    import os
    import basd_amd._native as native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_exported(lib):
    import basd_amd._native as native
    for name in NAMES:
        assert name in native.EXPORTS and name in native._SIGNATURES
        assert hasattr(lib, name)


def test_workspace_queries_grow(lib):
    fw, ww = lib.basd_selector_frames_workspace_bytes, lib.basd_selector_weights_workspace_bytes
    assert fw(12, 192) > 0 and ww(4, 12, 192) > 0
    assert fw(12, 192) > fw(6, 192) and fw(12, 192) > fw(12, 96)
    assert ww(4, 12, 192) > ww(2, 12, 192) > 0
    assert ww(4, 12, 192) > ww(4, 6, 192)
    assert ww(4, 12, 192) > ww(4, 12, 32)


def _weights(lib, E, L, D, ws_bytes):
    null = ctypes.c_void_p(0)
    # the workspace pointer is never dereferenced on the host: any non-NULL address reaches the size check
    ws = ctypes.c_void_p(4096) if ws_bytes else null
    return lib.basd_selector_weights(null, null, null, null, null, E, L, D, null, null, null, null, null, ws,
                                     ctypes.c_int64(ws_bytes), null)


def _frames(lib, n, D, ws_bytes, with_ranks=1):
    null = ctypes.c_void_p(0)
    ws = ctypes.c_void_p(4096) if ws_bytes else null
    return lib.basd_selector_frames(null, null, n, ctypes.c_int64(1568), D, with_ranks, null, null, null, null, null,
                                    ws, ctypes.c_int64(ws_bytes), null)


def test_weights_refuses_wide_and_many_layers(lib):
    big = 1 << 40
    assert _weights(lib, 4, 12, 384, big) == BASD_ERR_SHAPE
    assert _weights(lib, 4, 12, 768, big) == BASD_ERR_SHAPE
    assert _weights(lib, 4, 65, 192, big) == BASD_ERR_SHAPE
    assert b"selector_weights" in lib.basd_last_error()


def test_weights_short_workspace(lib):
    need = lib.basd_selector_weights_workspace_bytes(4, 12, 192)
    assert _weights(lib, 4, 12, 192, need - 1) == BASD_ERR_WORKSPACE
    assert _weights(lib, 4, 12, 192, 0) == BASD_ERR_WORKSPACE
    assert b"workspace" in lib.basd_last_error()


def test_frames_argument_checks(lib):
    big = 1 << 40
    assert _frames(lib, 12, 384, big) == BASD_ERR_SHAPE
    need = lib.basd_selector_frames_workspace_bytes(12, 192)
    assert _frames(lib, 12, 192, need - 1) == BASD_ERR_WORKSPACE
    assert _frames(lib, 12, 192, 0, with_ranks=0) == BASD_ERR_WORKSPACE
    # enough workspace, but the teacher half without a ranks output
    assert _frames(lib, 12, 192, need) == BASD_ERR_SHAPE


def test_empty_batches_are_no_ops(lib):
    assert _weights(lib, 0, 12, 192, 0) == 0
    assert _frames(lib, 0, 192, 0) == 0

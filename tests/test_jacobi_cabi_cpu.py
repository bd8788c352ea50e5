"""basd_jacobi_svd on a CPU-only machine: shapes outside every kernel's domain are refused with BASD_ERR_SHAPE whatever
the batch size, by checks that return before anything touches a device."""
import ctypes

import pytest

BASD_ERR_SHAPE = 1


@pytest.fixture(scope="module")
def lib():
    import os
    import basd_amd._native as native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def _svd(lib, batch, m_rows, n_cols, ld=None):
    null = ctypes.c_void_p(0)
    ld = (m_rows + 3) // 4 * 4 if ld is None else ld
    # w, batch, m_rows, n_cols, ld, norm_rows, tol, max_sweeps, sort, sigma, sweeps, active, active_rows, status, stream
    return lib.basd_jacobi_svd(null, batch, m_rows, n_cols, ld, m_rows, ctypes.c_float(1e-6), 40, 1, null, null, null,
                               0, null, null)


@pytest.mark.parametrize("batch", [1, 64])
@pytest.mark.parametrize("m,n", [(300, 194), (400, 64)])
def test_too_tall_shapes_are_refused_at_every_batch(lib, m, n, batch):
    """193 .. 196 columns of more than 256 rows, and 8 or more columns of more than 384 rows, fit no kernel."""
    assert _svd(lib, batch, m, n) == BASD_ERR_SHAPE
    assert b"jacobi_svd" in lib.basd_last_error()


@pytest.mark.parametrize("batch", [1, 64])
def test_entry_bounds(lib, batch):
    assert _svd(lib, batch, 64, 257) == BASD_ERR_SHAPE          # n_cols > BASD_JACOBI_MAX_COLS
    assert _svd(lib, batch, 64, 32, ld=66) == BASD_ERR_SHAPE    # ld % 4 != 0
    assert _svd(lib, batch, 64, 32, ld=60) == BASD_ERR_SHAPE    # m_rows > ld
    assert b"jacobi_svd" in lib.basd_last_error()

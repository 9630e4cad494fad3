"""CPU: psg_rows_shape, the host arithmetic the row kernels take their tile
and lane split from (csrc/psg_rows.h), over every width and both types."""
import ctypes as C

import pytest

from parameter_server_amd import _lib, rows_shape

ACC_BYTES, LDS_BUDGET, LDS_FIXED = 64 * 1024, 80 * 1024, 2048  # psg_rows.h


@pytest.mark.parametrize("dtype,size", ((_lib.PSG_F32, 4), (_lib.PSG_F64, 8)), ids=("f32", "f64"))
def test_shape_every_width(dtype, size):
    kmax = _lib.lib().psg_rows_max_width()
    assert kmax >= 128
    for k in range(1, kmax + 1):
        T, L, E, R = rows_shape(dtype, k)
        assert 32 <= T <= 1024 and T & (T - 1) == 0, k
        # the largest tile whose accumulators fit
        assert T * k * size <= ACC_BYTES and (T == 1024 or 2 * T * k * size > ACC_BYTES), k
        assert E * size == 16 and 1 <= L <= 64 and L & (L - 1) == 0 and L * R == 64, k
        loops = -(-k // (L * E))
        assert loops <= 2 and (loops == 1 or L == 64), k
        assert L == 1 or (L // 2) * E < k, k  # no idle half of a lane group
        assert T * (k * size + 12) + LDS_FIXED <= LDS_BUDGET, k


@pytest.mark.parametrize("dtype,k", ((_lib.PSG_F32, 0), (_lib.PSG_F64, 0), (_lib.PSG_F32, None),
                                     (_lib.PSG_F64, None), (7, 4)))
def test_shape_bad_arguments(dtype, k):
    L = _lib.lib()
    k = L.psg_rows_max_width() + 1 if k is None else k
    assert L.psg_rows_shape(dtype, k, (C.c_int * 4)()) == _lib.PSG_ERR_ARG

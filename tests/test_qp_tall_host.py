"""The reduced-KKT route's entry points without a GPU: exported symbols, argument validation, the size limits,
SFB_ERR_NO_DEVICE, and the Python wrappers' shape checks."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("sfb_qp_dense_tall_solve_batch", "sfb_qp_dense_tall_solve_batch_host", "sfb_qp_dense_tall_solve_batch_host_multi")


def _call(sfb, name, prm, B, n, m, ptrs=None, wx=None, wy=None):
    p = np.zeros(64).ctypes.data
    a = [p] * 5 if ptrs is None else ptrs
    args = [prm, B, n, m, *a, wx, wy, p, p, p, p, p]
    if name == NAMES[0]:
        args.append(None)
    return getattr(sfb._capi.lib, name)(*args)


def test_symbols_exported_and_declared(sfb):
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfb.h")).read()
    for name in NAMES:
        assert hasattr(sfb._capi.lib, name)
        assert "sfb_status %s(" % name in hdr
    assert "#define SFB_QP_DENSE_TALL_MAX_N 16" in hdr
    assert sfb.qp.TALL_MAX_N == 16 and sfb.qp.TALL_MAX_M >= 65536


@pytest.mark.parametrize("name", NAMES)
def test_argument_validation(sfb, name):
    E = sfb._capi
    cp = C.byref(sfb.QPSolverParams().to_c())
    p = np.zeros(64).ctypes.data
    assert _call(sfb, name, None, 1, 3, 5) == E.SFB_ERR_INVALID_ARG                      # prm NULL
    assert _call(sfb, name, cp, -1, 3, 5) == E.SFB_ERR_INVALID_ARG                       # batch < 0
    assert _call(sfb, name, cp, 1, 0, 5) == E.SFB_ERR_INVALID_ARG                        # n < 1
    assert _call(sfb, name, cp, 1, 3, 0) == E.SFB_ERR_INVALID_ARG                        # m < 1
    assert _call(sfb, name, cp, 1, 3, 5, ptrs=[None, p, p, p, p]) == E.SFB_ERR_INVALID_ARG  # NULL problem pointer
    assert _call(sfb, name, cp, 1, 3, 5, wx=p) == E.SFB_ERR_INVALID_ARG                  # warm_x without warm_y
    assert b"warm" in E.lib.sfb_last_error()
    # the size limits come before the device: 1 <= n <= 16, m <= 2^20
    assert _call(sfb, name, cp, 1, 17, 5) == E.SFB_ERR_UNSUPPORTED
    assert _call(sfb, name, cp, 1, 3, (1 << 20) + 1) == E.SFB_ERR_UNSUPPORTED
    assert b"SFB_QP_DENSE_TALL_MAX_N" in E.lib.sfb_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_no_device_is_an_error_not_a_fallback(sfb, name):
    if sfb._capi.device_count() > 0:
        return  # (with a device the GPU suite covers the entry points)
    cp = C.byref(sfb.QPSolverParams().to_c())
    for B in (0, 1):
        assert _call(sfb, name, cp, B, 3, 203) == sfb._capi.SFB_ERR_NO_DEVICE


def test_python_wrappers_check_shapes(sfb):
    B, n, m = 2, 3, 7
    P, q, A, l, u = np.zeros((B, n * n)), np.zeros((B, n)), np.zeros((B, m * n)), np.zeros((B, m)), np.ones((B, m))
    f = sfb.solve_qp_tall_batch_host
    with pytest.raises(ValueError):
        f(P[:, :-1], q, A, l, u)
    with pytest.raises(ValueError):
        f(P, q, A[:, :-1], l, u)
    with pytest.raises(ValueError):
        f(P, q, A, l, u[:, :-1])
    with pytest.raises(ValueError):
        f(P, q[0], A, l, u)
    with pytest.raises(ValueError):
        f(P, q, A, l[:1], u[:1])
    with pytest.raises(ValueError):
        f(P, q, A, l, u, warm_x=np.zeros((B, n)))
    with pytest.raises(ValueError):
        f(P, q, A, l, u, warm_x=np.zeros((B, n)), warm_y=np.zeros((B, m + 1)))
    if sfb._capi.device_count() == 0:
        with pytest.raises(sfb._capi.SfbError) as e:
            f(P, q, A, l, u)
        assert e.value.status == sfb._capi.SFB_ERR_NO_DEVICE
    with pytest.raises(sfb._capi.SfbError) as e:
        f(np.zeros((B, 17 * 17)), np.zeros((B, 17)), np.zeros((B, m * 17)), l, u)
    assert e.value.status == sfb._capi.SFB_ERR_UNSUPPORTED
    assert callable(sfb.solve_qp_tall_batch_device)

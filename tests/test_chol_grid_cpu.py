"""Host side of the grid Cholesky (csrc/chol_grid.hip), no GPU: what is refused before any device call -- an
unknown ``chol=`` / ``method=`` through every entry point that takes one, and the RATO_EINVAL set of the two launchers -- the
scratch query, and the three symbols in the public header and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _drone_gaussian_ipm as T
import _hopper_ipm as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SYMBOLS = ("rato_chol_grid_work_doubles", "rato_chol_factor_grid_batch_f64", "rato_chol_solve_grid_batch_f64")


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _lib
    return _lib.load()


def test_an_unknown_cholesky_is_a_value_error_before_any_device_call(tmp_path):
    import torch
    from riskaversetrajopt_amd import drone_gaussian as dg, drone_gaussian_ipm, hopper_ipm, ipm, scp
    model = H.host_model('saa', 0.2)                                  # host_only: any device call would raise something else
    for bad in ('panel', None, 'Grid'):
        with pytest.raises(ValueError, match="chol must be one of"):
            hopper_ipm.solve_batch([model], chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            model.solve(chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            scp.run_hopper(model, chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            scp.hopper_experiment(alphas=(0.1,), M=H.M_SMALL, S=H.S_SMALL, chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            scp.hopper_saa_experiment(alphas=(0.1,), num_repeats=1, M=H.M_SMALL, S=H.S_SMALL, chol=bad)
        gauss = dg.Model(3, alpha=0.1)
        with pytest.raises(ValueError, match="chol must be one of"):
            drone_gaussian_ipm.solve_batch([gauss], T.starts(3, [0.1]), chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            gauss.solve(T.starts(3, [0.1])[0], chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            scp.run_drone_gaussian(gauss, Z0=T.starts(3, [0.1])[0], solver='ipm', chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            scp.drone_gaussian_experiment(alphas=(0.1,), S=3, results_dir=str(tmp_path), solver='ipm', chol=bad)
        with pytest.raises(ValueError, match="chol must be one of"):
            ipm.DeviceBase(torch.device("cpu"), 1, chol=bad)
        A = torch.eye(4, dtype=torch.float64)[None]
        with pytest.raises(ValueError, match="method must be one of"):
            ipm.chol_factor(A, method=bad)
        with pytest.raises(ValueError, match="method must be one of"):
            ipm.chol_solve(A, A.clone(), method=bad)
    assert not os.listdir(tmp_path)                                  # refused before anything was computed or written
    assert ipm.CHOL_METHODS == ("workgroup", "grid")
    # backend='numpy' takes either method and ignores it: its Cholesky is NumPy's
    cb = H.RestatementCallbacks(model, H.fields(H.M_SMALL))
    a = hopper_ipm.solve_batch([model], backend='numpy', callbacks=[cb], max_iter=2, chol='grid')
    b = hopper_ipm.solve_batch([model], backend='numpy', callbacks=[cb], max_iter=2)
    assert a[0][0].tobytes() == b[0][0].tobytes()


def test_invalid_arguments_are_refused_without_a_launch(lib):
    """every case returns RATO_EINVAL before the first device call: the pointers below are never dereferenced"""
    P = C.c_void_p(4096)
    n = 40
    assert lib.rato_chol_grid_work_doubles(n) > 0

    def fac(A=P, n_=n, lda=n, K=2, info=P, work=P):
        return lib.rato_chol_factor_grid_batch_f64(A, n_, lda, K, info, work, None)

    def sol(L=P, n_=n, lda=n, K=2, B=P, nrhs=1, ldb=n):
        return lib.rato_chol_solve_grid_batch_f64(L, n_, lda, K, B, nrhs, ldb, None)
    assert fac(A=None) == EINVAL and fac(info=None) == EINVAL and fac(work=None) == EINVAL
    assert fac(n_=0) == EINVAL and fac(n_=-1) == EINVAL and fac(lda=n - 1) == EINVAL
    assert fac(K=0) == EINVAL and fac(K=65536) == EINVAL
    assert sol(L=None) == EINVAL and sol(B=None) == EINVAL and sol(n_=0) == EINVAL and sol(lda=n - 1) == EINVAL
    assert sol(ldb=n - 1) == EINVAL and sol(K=0) == EINVAL and sol(K=65536) == EINVAL
    assert sol(nrhs=0) == EINVAL and sol(nrhs=65536) == EINVAL and sol(n_=8001, lda=8001, ldb=8001) == EINVAL


def test_scratch_query_is_monotone(lib):
    nb = lib.rato_chol_panel_width()
    q = np.array([lib.rato_chol_grid_work_doubles(n) for n in range(-2, 8200)])
    assert np.all(q >= 0) and np.all(np.diff(q) >= 0)
    assert lib.rato_chol_grid_work_doubles(nb) == 0 and lib.rato_chol_grid_work_doubles(nb + 1) > 0
    assert lib.rato_chol_grid_work_doubles(0) == 0


def test_symbols_are_declared_bound_and_listed():
    from riskaversetrajopt_amd import _lib
    with open(os.path.join(ROOT, "include", "rato_saa.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    for name in SYMBOLS:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and name in integration, name
    assert _lib.SIGNATURES["rato_chol_grid_work_doubles"][0] is C.c_int64
    assert len(_lib.SIGNATURES["rato_chol_factor_grid_batch_f64"][1]) == len(_lib.SIGNATURES["rato_chol_factor_batch_f64"][1]) + 1
    assert _lib.SIGNATURES["rato_chol_solve_grid_batch_f64"] == _lib.SIGNATURES["rato_chol_solve_batch_f64"]
    assert _lib.ABI_VERSION == 12                                    # additive

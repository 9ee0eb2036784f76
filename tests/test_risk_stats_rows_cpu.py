"""CPU: the host side of rato_risk_stats_rows (csrc/stats_rows.hip) -- the launch plan, the workspace size and every
argument error, none of which touches a device."""
import ctypes as C

import pytest

RS_SMALL_MAX = 12288          # csrc/rato_select.h
RATO_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def _single_row_blocks(M):
    """risk_stats_impl's grid (csrc/rato_select.h: rs_pass_blocks): 4 elements per thread of 256 up to 256 workgroups, then
    16 per thread with a floor of 256, capped at 1024"""
    nb = (M + 1023) // 1024
    if nb > 256:
        nb = max((M + 4095) // 4096, 256)
    return max(min(nb, 1024), 1)


def _plan(lib, M, K):
    launches, blocks = C.c_int32(-7), C.c_int32(-7)
    rc = lib.rato_risk_stats_rows_plan(M, K, C.byref(launches), C.byref(blocks))
    return rc, launches.value, blocks.value


PLANS = {1: (1, 1), 12288: (1, 1), 12289: (5, 13), 262144: (5, 256), 262145: (5, 256), 4194304: (5, 1024),
         4194305: (5, 1024), 10 ** 7: (5, 1024)}


@pytest.mark.parametrize("M", sorted(PLANS))
@pytest.mark.parametrize("K", [1, 120, 65535])
def test_plan_is_one_launch_up_to_12288_and_five_beyond_with_the_single_row_grid(lib, M, K):
    rc, launches, blocks = _plan(lib, M, K)
    assert rc == 0
    assert (launches, blocks) == PLANS[M]
    if M > RS_SMALL_MAX:
        assert blocks == _single_row_blocks(M)          # the formula itself, not only the table
    else:
        assert launches == 1 and blocks == 1            # one workgroup per row


def test_plan_accepts_null_outputs_and_refuses_bad_shapes(lib):
    assert lib.rato_risk_stats_rows_plan(20000, 3, None, None) == 0
    for M, K in ((0, 1), (-1, 1), (2 ** 32 - 1, 1), (2 ** 32, 1), (100, 0), (100, -1), (100, 65536)):
        assert _plan(lib, M, K)[0] == RATO_EINVAL, (M, K)
    assert _plan(lib, 2 ** 32 - 2, 1) == (0, 5, 1024)


@pytest.mark.parametrize("M", [12289, 262144, 262145, 4194305, 10 ** 7])
@pytest.mark.parametrize("K", [1, 7, 120])
def test_workspace_is_K_single_row_workspaces_beyond_the_one_workgroup_form(lib, M, K):
    assert lib.rato_risk_stats_rows_workspace_bytes(M, K) == K * lib.rato_risk_stats_workspace_bytes(M)


@pytest.mark.parametrize("M", [1, 63, 12288])
def test_no_workspace_in_the_one_workgroup_form(lib, M):
    assert lib.rato_risk_stats_rows_workspace_bytes(M, 120) == 0


def test_every_argument_error_is_einval_before_any_launch(lib):
    """no device in this process: a call that reached a launch would not come back with RATO_EINVAL"""
    one = lib.rato_risk_stats_workspace_bytes(20000)
    p = C.c_void_p(4096)                                # never dereferenced: every call below is refused on the host
    st = C.c_void_p(0)

    def call(Z=p, M=20000, ldz=20000, K=2, alphas=p, ws=p, nbytes=2 * one, out=p):
        return lib.rato_risk_stats_rows(Z, M, ldz, K, alphas, 1e-6, ws, nbytes, out, st)

    assert call(Z=None) == RATO_EINVAL
    assert call(alphas=None) == RATO_EINVAL
    assert call(out=None) == RATO_EINVAL
    assert call(K=0) == RATO_EINVAL
    assert call(K=-3) == RATO_EINVAL
    assert call(K=65536, nbytes=65536 * one) == RATO_EINVAL
    assert call(M=0, ldz=5) == RATO_EINVAL
    assert call(M=-5, ldz=5) == RATO_EINVAL
    assert call(M=2 ** 32 - 1, ldz=2 ** 32) == RATO_EINVAL
    assert call(M=2 ** 32, ldz=2 ** 32) == RATO_EINVAL
    assert call(ldz=19999) == RATO_EINVAL
    assert call(ws=None) == RATO_EINVAL                 # beyond 12,288 a workspace is needed
    assert call(nbytes=2 * one - 1) == RATO_EINVAL      # ... of K single-row workspaces
    assert call(nbytes=0) == RATO_EINVAL
    # the one-workgroup form: the same shape errors, with or without a workspace
    assert call(M=100, ldz=99, ws=None, nbytes=0) == RATO_EINVAL
    assert call(M=100, ldz=100, K=0, ws=None, nbytes=0) == RATO_EINVAL
    assert call(M=100, ldz=100, alphas=None, ws=None, nbytes=0) == RATO_EINVAL
    # the workspace initialiser
    assert lib.rato_risk_stats_rows_init(None, 2 * one, st) == RATO_EINVAL
    assert lib.rato_risk_stats_rows_init(p, one - 1, st) == RATO_EINVAL
    assert lib.rato_risk_stats_rows_init(p, 0, st) == RATO_EINVAL


def test_python_surface_exists():
    from riskaversetrajopt_amd import drone_risk, driving, hopper, scp, stats
    import inspect
    for f in (stats.new_rows_workspace, stats.risk_stats_rows_device, stats.risk_stats_rows, scp.monte_carlo_report_grid):
        assert callable(f)
    assert "alphas" in inspect.signature(drone_risk.Model.eval_batch_device).parameters
    assert "alphas" in inspect.signature(driving.Model.eval_batch_device).parameters
    for f in (hopper.Model.eval_batch_inputs_device, hopper.Model.eval_batch_device, scp.hopper_monte_carlo_report):
        assert inspect.signature(f).parameters["selection"].default == 'entry'
    for f in (scp.drone_saa_experiment, scp.driving_saa_experiment):
        assert inspect.signature(f).parameters["mc"].default == 'per_alpha'

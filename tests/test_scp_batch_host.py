"""CPU: the sample draws of the drone SAA experiment helper (scp.draw_saa_batches / drone_saa_experiment) follow the
reference's draw order (drone_risk.py:57, :480-490), and the batch entry points are declared in the binding."""
import numpy as np
import pytest


def test_draws_follow_the_reference_order():
    from riskaversetrajopt_amd import scp
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    got = scp.draw_saa_batches(num_repeats=4, M=50, S=20, seed=0)
    np.random.seed(0)
    want = [sample_uncertain_parameters('saa', M=50) for _ in range(4)]   # (the reference's defaults: S = 20, dt = T / S)
    assert len(got) == 4
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and np.array_equal(a, b)
    # repeats differ from each other (one stream, consumed in order), and a different seed gives different batches
    assert not np.array_equal(got[0][0], got[1][0])
    assert not np.array_equal(scp.draw_saa_batches(num_repeats=1, M=50, S=20, seed=1)[0][0], got[0][0])


def test_draws_at_another_horizon_use_its_dt():
    from riskaversetrajopt_amd import scp
    from riskaversetrajopt_amd import drone_params as P
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    got = scp.draw_saa_batches(num_repeats=2, M=7, S=30, seed=3)
    np.random.seed(3)
    want = [sample_uncertain_parameters('saa', M=7, S=30, dt=P.T / 30) for _ in range(2)]
    assert got[0][0].shape == (7, 30, 6)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert np.array_equal(a, b)


def test_grid_is_indexed_alpha_then_repeat(monkeypatch):
    """drone_saa_experiment builds the alpha x repeat grid alpha-major, every alpha on the same batches, and hands the
    whole grid to ONE batched solve (stubbed here: no GPU)"""
    from riskaversetrajopt_amd import drone_risk, scp
    built, calls = [], []

    class FakeModel:
        def __init__(self, S, DWs, masses, obs_Qs, method, alpha, device=None):
            self.S, self.DWs, self.alpha, self.method = S, DWs, alpha, method
            built.append(self)

    def fake_batch(models, num_scp_iters_max=60, n_threads=None):
        calls.append(len(models))
        return [{"us": np.full((m.S, 3), m.alpha + 1000 * k), "rounds": 7} for k, m in enumerate(models)]

    monkeypatch.setattr(drone_risk, "Model", FakeModel)
    monkeypatch.setattr(scp, "run_drone_reduced_batch", fake_batch)
    alphas, R = (0.05, 0.1, 0.2), 3
    out = scp.drone_saa_experiment(alphas=alphas, num_repeats=R, M=9, S=20, iters=2, seed=5)
    assert calls == [len(alphas) * R]
    draws = scp.draw_saa_batches(num_repeats=R, M=9, S=20, seed=5)
    for i, a in enumerate(alphas):
        for r in range(R):
            m = built[i * R + r]
            assert m.alpha == a and m.method == 'saa' and np.array_equal(m.DWs, draws[r][0])
            assert out["results"][i][r]["us"][0, 0] == a + 1000 * (i * R + r)
    assert out["us"].shape == (len(alphas), R, 20, 3) and out["rounds"] == 7 and out["alphas"] == list(alphas)


def test_batch_entry_points_are_bound():
    from riskaversetrajopt_amd import _lib
    for name in ("rato_scp_batch_bytes", "rato_scp_batch_create", "rato_scp_batch_run_drone", "rato_scp_batch_destroy",
                 "rato_scp_batch_iter_bytes"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    import ctypes as C
    assert lib.rato_scp_batch_iter_bytes() == C.sizeof(_lib.ScpBatchIter)
    # no solvers: an invalid argument, answered without touching a device
    d, h = C.c_size_t(0), C.c_size_t(0)
    assert lib.rato_scp_batch_bytes(None, 0, C.byref(d), C.byref(h)) == -1


def test_batch_rejects_a_driving_model_before_device_work():
    from riskaversetrajopt_amd import scp
    with pytest.raises(ValueError):
        scp.run_drone_reduced_batch([object()], num_scp_iters_max=1)
    with pytest.raises(ValueError):
        scp.run_drone_reduced_batch([], num_scp_iters_max=1)


@pytest.mark.parametrize("system", ["drone_risk", "driving"])
def test_check_batch_and_l2_error_are_shared_by_both_systems(system):
    """both Model modules keep ``_check_batch`` (one body, cvar_cuts.check_scp_batch) and the reference's module-level
    ``L2_error_us`` (one definition, scp.py); no device is touched"""
    import importlib
    from riskaversetrajopt_amd import scp
    mod = importlib.import_module("riskaversetrajopt_amd." + system)
    with pytest.raises(ValueError, match="at least one"):
        mod._check_batch([])
    with pytest.raises(ValueError, match=system.split("_")[0]):
        mod._check_batch([object()])
    assert mod.L2_error_us is scp.L2_error_us

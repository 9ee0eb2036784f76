"""CPU: the host-only parts of the hopper's batched Monte-Carlo evaluation -- the launch-shape rule of rato_hopper_eval_batch
(rato_hopper_eval_batch_plan makes no HIP call), ``Model.contact_inputs_batch`` on a host-only model, the ``validate=`` check
of ``scp.hopper_saa_experiment`` and the report file's round trip."""
import ctypes as C
import itertools

import numpy as np
import pytest

EINVAL, OK = -1, 0
MS, CS, KS = (1, 64, 65, 10_000, 1_000_000), (1, 7, 20, 129), (1, 2, 7, 120, 121)


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def plan(lib, M, Cn, K):
    v = [C.c_int32(-7) for _ in range(4)]
    rc = lib.rato_hopper_eval_batch_plan(M, Cn, K, *(C.byref(x) for x in v))
    return rc, tuple(x.value for x in v)


def test_plan_covers_the_batch_at_every_size(lib):
    seen = set()
    for M, Cn, K in itertools.product(MS, CS, KS):
        rc, (nw, kc, gx, gy) = plan(lib, M, Cn, K)
        assert rc == OK, (M, Cn, K)
        assert nw in (0, 1, 2) and 1 <= kc <= K, (M, Cn, K, nw, kc)
        assert gy * kc >= K > (gy - 1) * kc, (M, Cn, K, kc, gy)
        samples_per_block = 256 >> nw
        assert gx * samples_per_block >= M > (gx - 1) * samples_per_block, (M, Cn, K, nw, gx)
        assert (1 << nw) <= max(Cn, 1), "no more contact-waves than contacts"
        assert 1 <= gy <= 65535
        seen.add((nw, kc > 1))
    assert {nw for nw, _ in seen} == {0, 2}, "the sizes above reach the unsplit and the four-way form"
    assert (0, True) in seen, "and a chunk of several solutions without a split"
    # the two-way split: where it is what leaves two solutions per wave, and where there are only two or three contacts
    assert plan(lib, 10_000, 20, 30)[1][:2] == (1, 3)
    assert plan(lib, 64, 2, 1)[1][:2] == (1, 1) and plan(lib, 64, 3, 5)[1][0] == 1 and plan(lib, 64, 1, 5)[1][0] == 0
    # the report's own sizes: enough waves for three per SIMD on 1024 SIMDs where the work allows it
    for K in (7, 120):
        rc, (nw, kc, gx, gy) = plan(lib, 10_000, 20, K)
        waves = gx * 4 * gy
        print("M 10000 C 20 K", K, "-> nw_log2", nw, "k_chunk", kc, "grid", gx, gy, "waves", waves)
        assert waves >= min(3072, 157 * 4 * K)
    assert plan(lib, 10_000, 20, 7)[1][0] > 0, "K x sample-waves alone do not fill the chip: the contacts are split"
    assert plan(lib, 10_000, 20, 120)[1][:2] == (0, 6), "they do: chunks of several solutions, no split"


def test_plan_refuses_empty_batches(lib):
    for M, Cn, K in ((0, 7, 7), (7, 0, 7), (7, 7, 0), (-1, 7, 7), (7, -5, 7), (7, 7, -1)):
        rc, out = plan(lib, M, Cn, K)
        assert rc == EINVAL and out == (-7, -7, -7, -7), (M, Cn, K)
    assert lib.rato_hopper_eval_batch_plan(64, 7, 7, None, None, None, None) == EINVAL


def synthetic_Z(S, M, seed):
    rng = np.random.RandomState(seed)
    Z = rng.randn(8 * (S + 1) + 4 * S + M + 2)
    Z[3:8 * (S + 1):8] += 1.0
    return Z


def test_contact_inputs_batch_is_contact_inputs_row_by_row():
    from riskaversetrajopt_amd import hopper
    S, M = 30, 5
    m = hopper.Model.host_only(M, S=S)
    Zs = [synthetic_Z(S, M, k) for k in range(4)]
    Zs.append(synthetic_Z(S, 30, 9))                     # another problem's M: only the states and controls are read
    px, forces = m.contact_inputs_batch(Zs)
    Cn = m.time_jump + S - m.time_land
    assert px.shape == (5, Cn) and forces.shape == (5, Cn, 2) and px.dtype == forces.dtype == np.float64
    for k, Z in enumerate(Zs):
        p, f = m.contact_inputs(Z)
        assert px[k].tobytes() == p.tobytes() and forces[k].tobytes() == f.tobytes(), k
    assert not np.array_equal(px[0], px[1])
    other = hopper.Model.host_only(M, S=S, phases=(4, 25))
    assert other.contact_inputs_batch(Zs[:2])[0].shape == (2, 4 + 5)
    with pytest.raises(ValueError, match="at least one"):
        m.contact_inputs_batch([])


def test_validate_is_checked_before_any_work(monkeypatch):
    from riskaversetrajopt_amd import hopper, scp

    def touched(*a, **k):
        raise AssertionError("a model was built before the argument was checked")
    monkeypatch.setattr(hopper, "Model", touched)
    monkeypatch.setattr(scp, "draw_hopper_saa_fields", touched)
    for bad in ("nonsense", "Batch", None, 1):
        with pytest.raises(ValueError, match="validate must be 'solo' or 'batch'"):
            scp.hopper_saa_experiment(validate=bad, device="cuda:99")


def test_report_file_round_trips(tmp_path):
    from riskaversetrajopt_amd import scp
    K = 7
    rng = np.random.RandomState(3)
    report = {"alphas": np.array([0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 0.0]), "jump": rng.rand(K), "frac_satisfied": rng.rand(K),
              "var": rng.randn(K), "avar": rng.randn(K), "arg_counts": np.zeros((K, 20), dtype=np.int64), "wall_s": 1.0}
    report["var"][-1] = report["avar"][-1] = np.nan      # the baseline's row
    path = scp.save_hopper_monte_carlo_report(str(tmp_path / "results"), report)
    assert path == str(tmp_path / "results" / "hopper_monte_carlo_report.npy") == str(tmp_path / "results" / scp.HOPPER_MC_REPORT)
    back = scp.load_results(path, 5)
    assert scp.HOPPER_MC_REPORT_ARRAYS == ("alphas", "jump", "frac_satisfied", "var", "avar")
    for name, arr in zip(scp.HOPPER_MC_REPORT_ARRAYS, back):
        assert arr.dtype == np.float64 and arr.tobytes() == report[name].tobytes(), name
    assert np.isnan(back[3][-1]) and np.isnan(back[4][-1])
    # the alphas of a report: a scalar, a sequence with None or the script's 0 for the baseline
    assert scp._hopper_mc_alphas(0.1, 3) == [0.1, 0.1, 0.1]
    assert scp._hopper_mc_alphas([0.05, None, 0.0], 3) == [0.05, None, None]
    with pytest.raises(ValueError, match="alphas"):
        scp._hopper_mc_alphas([0.1, 0.2], 3)

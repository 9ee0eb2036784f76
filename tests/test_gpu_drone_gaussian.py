"""GPU: rato_drone_gaussian_linearize / rato_drone_gaussian_hessian (csrc/drone_gaussian.hip) and what is built on them,
against the fp64 NumPy restatement (tests/_drone_gaussian.py, itself pinned to the reference's text and to torch's
jacfwd o jacfwd by test_drone_gaussian_pin.py) and against the fixture recorded from the reference's text.

Tolerance.  Both sides are fp64; they differ by contraction, the device's sqrt / log / exp and the ppf routine (Wichura's
PPND16 against scipy's ndtri).  The largest max-abs-scaled difference over every shape below, measured on the MI355X, is
MEASURED = 1.667e-14 (S = 64, problem 1, the (u,u) block of the Hessian; <= 4.6e-15 at S <= 22); the bound is
100x that, 1.7e-12, and in any case no looser than 1e-9.  A wrong derivative term shows at 1e-3
or above.  The Hessian is compared per block ((u,u), (u,a), diag (a,a)), each scaled by its own max-abs.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _drone_gaussian as R

pytestmark = pytest.mark.gpu

MEASURED = 1.667e-14   # largest scaled difference seen on the MI355X over SHAPES x K (S = 64, k = 1, hess (u,u))
TOL = min(100 * MEASURED, 1e-9)
ALPHA = 0.1
MAX_S = 64
SHAPES = (1, 2, 3, 5, 20, 22, MAX_S)
HERE = os.path.dirname(os.path.abspath(__file__))

_REF = {}


def _reference(S, k):
    """the restatement of problem k of R.problems(S, 4), computed once and shared"""
    if (S, k) not in _REF:
        Z, lam = R.problems(S, 4)[k]
        _REF[(S, k)] = R.evaluate(Z, S, [lam])
    return _REF[(S, k)]


def _model(S, alpha=ALPHA):
    from riskaversetrajopt_amd import drone_gaussian as DG
    return DG.Model(S, alpha=alpha)


def _launch(S, K, want_trajectory=True):
    pr = R.problems(S, K)
    Z, lam = np.stack([p[0] for p in pr]), np.stack([p[1] for p in pr])
    m = _model(S)
    out = {k: v.cpu().numpy() for k, v in m.linearize_device(Z, want_trajectory=want_trajectory).items()}
    out["hess"] = m.hessian_device(Z, lam).cpu().numpy()
    return out


def _scaled(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def _full(tril, nvar):
    H = np.zeros((nvar, nvar))
    H[np.tril_indices(nvar)] = tril
    return H + np.tril(H, -1).T


def _check_hessian(tril, H_ref, S, what):
    """per block against the reference, and the literal zeros -> the worst scaled difference"""
    nvar = R.sizes(S)[0]
    D = 3 * S
    H = _full(tril, nvar)
    worst = 0.0
    for got, ref, name in zip(R.hess_blocks(H, S), R.hess_blocks(H_ref, S), ("(u,u)", "(u,a)", "diag (a,a)")):
        if np.max(np.abs(ref)) == 0.0:
            assert not np.any(got), (what, name)
            continue
        err = _scaled(got, ref)
        print(f"{what} hess {name}: {err:.3e}")
        assert err <= TOL, (what, name, err)
        worst = max(worst, err)
    aa = H[D:, D:]
    assert np.all((aa - np.diag(np.diag(aa))) == 0.0), "(a,a) off the diagonal is exactly 0.0"
    assert np.all(H[D + 3 * S:, :] == 0.0), "everything involving a_obs is exactly 0.0"
    ua = H[D:D + 3 * S, :D].reshape(S, 3, S, 3)
    for t in range(S):
        assert np.all(ua[t, :, t + 1:] == 0.0), "(u,a): a later control is exactly 0.0"
    return worst


def _check_jacobian_zeros(J, S):
    D = 3 * S
    for i in range(3):
        for t in range(S):
            row = J[6 + i * S + t]
            assert np.all(row[3 * (t + 1):D] == 0.0)
            alloc = row[D:].copy()
            alloc[t * 3 + i] = alloc[3 * S + i] = 0.0
            assert np.all(alloc == 0.0)
    for base in (6 + 3 * S, 6 + 3 * S + 2 * (S + 1)):
        for t in range(S + 1):
            for j in range(2):
                row = J[base + t * 2 + j]
                assert np.all(row[D:] == 0.0) and np.all(row[3 * t:D] == 0.0)
                assert np.all(np.delete(row[:D].reshape(S, 3), j, axis=1) == 0.0)
    for j in range(6):
        assert np.all(J[j, D:] == 0.0) and np.all(np.delete(J[j, :D].reshape(S, 3), j % 3, axis=1) == 0.0)


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("S", SHAPES)
def test_kernel_equals_restatement(S, K):
    """S = 1: only Sigma_0 = 0 and v = 0; S = 2: the first non-zero derivative of A; S = 22: 3S = 66 directions cross a wave;
    S = 20 / 22 / 64: the pairs span many workgroups with a ragged last one; S = 64: the guard's edge."""
    got = _launch(S, K)
    worst = 0.0
    for k in range(K):
        ref = _reference(S, k)
        assert ref["dist_norm"].min() >= 0.1 and ref["nSn"].min() >= 1e-6     # the floors the tolerance relies on
        for key in ("mus", "Sigmas", "g_nl", "jac_nl"):
            assert got[key][k].shape == ref[key].shape, key
            err = _scaled(got[key][k], ref[key])
            worst = max(worst, err)
            print(f"S={S} K={K} k={k} {key}: {err:.3e}")
            assert err <= TOL, (key, k, err)
        _check_jacobian_zeros(got["jac_nl"][k], S)
        worst = max(worst, _check_hessian(got["hess"][k], ref["hess"][0], S, f"S={S} K={K} k={k}"))
    print(f"S={S} K={K} worst scaled difference {worst:.3e}")


@pytest.mark.parametrize("rows", ["final", "obstacle", "high", "low"])
def test_lambda_on_one_row_class(rows):
    """lam supported on one row class at a time: a missing class cannot hide in a sum"""
    S = 5
    nvar, n_nl = R.sizes(S)
    Z, lam = R.problems(S, 1)[0]
    lo, hi = {"final": (0, 6), "obstacle": (6, 6 + 3 * S), "high": (6 + 3 * S, 6 + 3 * S + 2 * (S + 1)),
              "low": (6 + 3 * S + 2 * (S + 1), n_nl)}[rows]
    one = np.zeros(n_nl)
    one[lo:hi] = lam[lo:hi]
    H_ref = R.evaluate(Z, S, [one])["hess"][0]
    assert np.max(np.abs(H_ref[:3 * S, :3 * S])) > 1e-3, "the class has curvature in u at this input"
    tril = _model(S).hessian_device(Z[None], one[None]).cpu().numpy()[0]
    _check_hessian(tril, H_ref, S, rows)


@pytest.mark.parametrize("kind", ["wave", "swerve"])
def test_kernel_equals_reference_fixture(kind):
    """the S = 20 Jacobian and Hessian against the arrays recorded from the reference's own text"""
    S = 20
    fx = np.load(os.path.join(HERE, "golden", "ref_drone_gaussian_S20.npz"))
    nvar, n_nl = R.sizes(S)
    Z, lam = fx[kind + "_Z"], fx[kind + "_lam"][:n_nl]
    m = _model(S)
    lin = {k: v.cpu().numpy()[0] for k, v in m.linearize_device(Z[None], want_trajectory=True).items()}
    for key, ref in (("mus", fx[kind + "_xs"]), ("Sigmas", fx[kind + "_Sigmas"]), ("g_nl", fx[kind + "_g"][:n_nl]),
                     ("jac_nl", fx[kind + "_jac"][:n_nl])):
        err = _scaled(lin[key], ref)
        print(f"{kind} {key}: {err:.3e}")
        assert err <= TOL, (key, err)
    _check_hessian(m.hessian_device(Z[None], lam[None]).cpu().numpy()[0], fx[kind + "_hess"], S, kind)


@pytest.mark.parametrize("S", [5, 22])
def test_batch_is_bit_identical_to_single_launches(S):
    pr = R.problems(S, 4)
    Z, lam = np.stack([p[0] for p in pr]), np.stack([p[1] for p in pr])
    m = _model(S)
    batch = {k: v.cpu().numpy() for k, v in m.linearize_device(Z, want_trajectory=True).items()}
    hess = m.hessian_device(Z, lam).cpu().numpy()
    for k in range(4):
        one = m.linearize_device(Z[k:k + 1], want_trajectory=True)
        for key in batch:
            assert np.array_equal(batch[key][k], one[key].cpu().numpy()[0]), (key, k)
        assert np.array_equal(hess[k], m.hessian_device(Z[k:k + 1], lam[k:k + 1]).cpu().numpy()[0]), k


@pytest.mark.parametrize("K", [64, 65, 130])
def test_trajectory_of_more_problems_than_one_block_holds(K):
    """``drone_gaussian_trajectory_kernel`` takes the problem number from the lane, 64 problems a block: a full block, one problem
    into the second, and a ragged third.  K distinct blends of the two control sequences of ``_drone_gaussian.problems``;
    every row of mus / Sigmas bitwise its K = 1 launch, rows 0, 63, 64 and K - 1 against the restatement"""
    S = 3
    a = np.arange(K) / (K - 1.0)
    Z = np.stack([R.make_z(a[k] * R.us_wave(S) + (1.0 - a[k]) * R.us_swerve(S),
                           R.alphas_spread(S, ALPHA) if k % 2 == 0 else R.alphas_uniform(S, ALPHA)) for k in range(K)])
    m = _model(S)
    batch = {k: v.cpu().numpy() for k, v in m.linearize_device(Z, want_trajectory=True).items()}
    assert batch["mus"].shape == (K, S + 1, 6) and batch["Sigmas"].shape == (K, S + 1, 6, 6)
    for k in range(K):
        one = m.linearize_device(Z[k:k + 1], want_trajectory=True)
        for key in ("mus", "Sigmas"):
            assert batch[key][k].tobytes() == one[key].cpu().numpy()[0].tobytes(), (key, k)
    for k in sorted({0, 63, 64, K - 1} & set(range(K))):
        ref = R.evaluate(Z[k], S)
        for key in ("mus", "Sigmas"):
            err = _scaled(batch[key][k], ref[key])
            print(f"S={S} K={K} k={k} {key}: {err:.3e}")
            assert err <= TOL, (key, k, err)


@pytest.mark.parametrize("S", [5, 22])
def test_null_trajectory_leaves_the_rest_bit_identical(S):
    with_traj, without = _launch(S, 3, want_trajectory=True), _launch(S, 3, want_trajectory=False)
    assert "mus" not in without and "Sigmas" not in without
    for key in ("g_nl", "jac_nl", "hess"):
        assert np.array_equal(with_traj[key], without[key]), key


def _buffers(S):
    import torch
    nvar, n_nl = R.sizes(S)
    buf = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    Z = buf(1, nvar)
    Z += torch.as_tensor(R.problems(S, 1)[0][0], device="cuda")
    return Z, buf(1, n_nl) + 1.0, buf(1, n_nl), buf(1, n_nl, nvar), buf(1, nvar * (nvar + 1) // 2)


@pytest.mark.parametrize("S,K", [(MAX_S + 1, 1), (0, 1), (20, 0)])
def test_invalid_arguments_do_not_launch(S, K):
    """valid buffers (sized for S = 65), the status only: RATO_EINVAL (-1) without a launch, the outputs untouched"""
    import torch
    from riskaversetrajopt_amd import _lib
    from riskaversetrajopt_amd import drone_gaussian as DG
    lib = _lib.load()
    p = DG.gauss_params(20)
    p.S = S
    Z, lam, g, jac, hess = _buffers(MAX_S + 1)
    st = _lib.current_stream()
    assert lib.rato_drone_gaussian_linearize(C.byref(p), K, _lib.ptr(Z), None, None, _lib.ptr(g), _lib.ptr(jac), st) == -1
    assert lib.rato_drone_gaussian_hessian(C.byref(p), K, _lib.ptr(Z), _lib.ptr(lam), _lib.ptr(hess), None, 0, st) == -1
    torch.cuda.synchronize()
    assert not torch.any(g) and not torch.any(jac) and not torch.any(hess)


def test_null_required_pointer_and_short_workspace_are_invalid():
    """each required pointer NULL; a workspace one byte short of the query (the query is 0 bytes at every (S, K) -- the
    kernels keep their state in registers -- so no shorter workspace exists: asserted, with NULL accepted)"""
    import torch
    from riskaversetrajopt_amd import _lib
    from riskaversetrajopt_amd import drone_gaussian as DG
    lib = _lib.load()
    S = 5
    p = DG.gauss_params(S)
    Z, lam, g, jac, hess = _buffers(S)
    st = _lib.current_stream()
    lin = [Z, g, jac]
    for missing in range(3):
        a = [None if i == missing else _lib.ptr(t) for i, t in enumerate(lin)]
        assert lib.rato_drone_gaussian_linearize(C.byref(p), 1, a[0], None, None, a[1], a[2], st) == -1
    assert lib.rato_drone_gaussian_linearize(None, 1, _lib.ptr(Z), None, None, _lib.ptr(g), _lib.ptr(jac), st) == -1
    hs = [Z, lam, hess]
    for missing in range(3):
        a = [None if i == missing else _lib.ptr(t) for i, t in enumerate(hs)]
        assert lib.rato_drone_gaussian_hessian(C.byref(p), 1, a[0], a[1], a[2], None, 0, st) == -1
    assert lib.rato_drone_gaussian_hessian(None, 1, _lib.ptr(Z), _lib.ptr(lam), _lib.ptr(hess), None, 0, st) == -1
    for S_q, K_q in ((1, 1), (5, 1), (20, 4), (MAX_S, 4)):
        need = lib.rato_drone_gaussian_hessian_workspace_bytes(S_q, K_q)
        assert need == 0
    torch.cuda.synchronize()
    assert not torch.any(g) and not torch.any(jac) and not torch.any(hess)
    assert lib.rato_drone_gaussian_hessian(C.byref(p), 1, _lib.ptr(Z), _lib.ptr(lam), _lib.ptr(hess), None, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.any(hess)


@pytest.mark.parametrize("S", [5, 20])
def test_mean_rows_equal_the_saa_models(S):
    """`final` and its Jacobian against drone_risk.Model at nominal mass and zero noise for the same us.  The form of
    tests/test_car_final_rows.py, 64 S eps scale; the SAA model's rollout and tangents are fp32 per sample, so eps is
    float32's: the Jacobian within 64 S eps max|final_du|, the values within 64 S eps (max|x_S - x_final| + max_i sum
    |final_du . u|)."""
    from riskaversetrajopt_amd import drone_params as P
    from riskaversetrajopt_amd import drone_risk
    eps = np.finfo(np.float32).eps
    M = 64
    Q = np.tile(np.eye(3)[None, None], (M, 3, 1, 1))
    saa = drone_risk.Model(S, np.zeros((M, S, 6)), np.full(M, P.mass_nom), Q, 'saa', ALPHA)
    got = _launch(S, 2, want_trajectory=False)
    for k in range(2):
        us = R.problems(S, 2)[k][0][:3 * S].reshape(S, 3)
        E, rhs, _ = saa.sample_means(us)
        v_ref = -(rhs - E @ us.reshape(-1))                          # final_rhs = -(x_S - x_final) + final_du . u
        assert np.max(np.abs(got["jac_nl"][k][:6, :3 * S] - E)) <= 64 * S * eps * np.max(np.abs(E))
        bound = 64 * S * eps * (np.max(np.abs(v_ref)) + np.sum(np.abs(E * us.reshape(-1)[None]), axis=1).max())
        assert np.max(np.abs(got["g_nl"][k][:6] - v_ref)) <= bound


def test_solver_in_lockstep_with_the_restatement():
    """30 iterations of run_drone_gaussian on the device at S = 5: at every visited point the device's g and Jacobian equal
    the restatement at the DEVICE's own iterate, at the first three Hessian calls the Hessian does too; the final constraint
    violation is below a tenth of the initial 1.93.  (Iterates are not compared across legs.)"""
    from riskaversetrajopt_amd import scp
    S = 5
    m = _model(S)
    cb = m.device_callbacks()
    seen_lin, seen_hess = [], []

    def linearize(Z):
        out = cb["linearize"](Z)
        seen_lin.append((Z.copy(), out))
        return out

    def hessian(Z, lam):
        out = cb["hessian"](Z, lam)
        if len(seen_hess) < 3:
            seen_hess.append((Z.copy(), lam.copy(), out))
        return out
    Z0 = R.start_point(S, ALPHA)
    res = scp.run_drone_gaussian(m, Z0=Z0, maxiter=30, callbacks=dict(linearize=linearize, hessian=hessian,
                                                                      trajectory=cb["trajectory"]))
    assert len(seen_lin) >= 10 and len(seen_hess) == 3
    for Z, (g, J) in seen_lin:
        ref = R.evaluate(Z, S)
        assert _scaled(g, ref["g_nl"]) <= TOL and _scaled(J, ref["jac_nl"]) <= TOL
    for Z, lam, tril in seen_hess:
        if np.any(lam):
            _check_hessian(tril, R.evaluate(Z, S, [lam])["hess"][0], S, "solver")

    def violation(Z):
        g = R.evaluate(Z, S)["g_nl"]
        return max(np.max(np.abs(g[:6])), np.max(g[6:]), 0.0)
    v0, v1 = violation(Z0), violation(res["Z"])
    print(f"violation {v0:.3f} -> {v1:.3e}; status {res['status']} nit {res['nit']} nfev {res['nfev']} "
          f"callbacks {res['callback_s']:.3f}s of {res['total_s']:.3f}s")
    assert v0 == pytest.approx(1.93, abs=5e-3)
    assert v1 < 0.1 * 1.93
    assert _scaled(res["xs"], R.dense_trajectory(res["us"], S)[0]) <= TOL


def test_experiment_report(tmp_path):
    from riskaversetrajopt_amd import drone_params as P
    from riskaversetrajopt_amd import scp
    S, alphas = 5, (0.1, 0.3)
    out = scp.drone_gaussian_experiment(alphas=alphas, S=S, maxiter=40, M_mc=2000, results_dir=str(tmp_path))
    assert out["alphas"] == [0.1, 0.3] and out["us"].shape == (2, S, 3) and out["Z"].shape == (2, 2000)
    assert out["status"].shape == (2,) and len(out["results"]) == 2
    np.testing.assert_array_equal(out["percentage_safe"], np.mean(out["Z"] <= 1e-6, axis=1))
    assert np.all((out["percentage_safe"] >= 0.0) & (out["percentage_safe"] <= 1.0))
    for k, a in enumerate(alphas):
        assert os.path.isfile(os.path.join(str(tmp_path), f"drone_alpha={a}_repeat=0.npy"))
        us, xs = scp.load_results(os.path.join(str(tmp_path), f"drone_gaussian_alpha={a}.npy"), 2)
        assert us.shape == (S, 3) and xs.shape == (S + 1, 6)
        np.testing.assert_array_equal(us, out["us"][k])
        assert out["cost"][k] == pytest.approx(P.dt * np.sum(np.diag(P.R)[None] * us * us), rel=1e-12)

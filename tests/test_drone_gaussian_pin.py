"""CPU: the drone Gaussian baseline's callbacks (drone/drone_gaussian.py) without a device.

  * the fp64 NumPy restatement (tests/_drone_gaussian.py: values, Jacobian and Hessian of lam . g) equals what the
    reference's own text gives on the stand-in (tests/golden/ref_drone_gaussian_S20.npz,
    make_reference_golden_drone_gaussian.py) to 1e-11 of each array's max-abs -- the project's pin level -- at S = 20 and
    S = 5; the Hessian PER BLOCK ((u,u), (u,a), diag (a,a), each scaled by its own max-abs: (a,a) reaches 5.8e4 against 20
    for (u,u), and one global scale would hide a wrong second-order term);
  * its derivatives equal torch.func.jacfwd and jacfwd o jacfwd of an independent torch-fp64 forward (written from the
    reference's statements, no closed-form derivative in it) at S in {1, 2, 3, 5}, at the same level;
  * the structure the kernels' literal zeros rely on, in the reference's own numbers;
  * the documented inputs stay away from |d| -> 0 and sqrt(0);
  * ``Model.ipopt_callbacks`` fed the fixture's arrays lands them in the script's layout, with the script's bounds;
  * ``scp.run_drone_gaussian`` on the restatement's callbacks converges at S = 5 to the prototype's objective.
"""
import os

import numpy as np
import pytest

import _drone_gaussian as R

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = 1e-11
ALPHA = 0.1
CASES = [("", 20, "wave"), ("", 20, "swerve"), ("s5_", 5, "wave"), ("s5_", 5, "swerve")]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_drone_gaussian_S20.npz"))


_EVAL = {}


def _restatement(fx, pre, S, kind):
    """the restatement at one fixture case, computed once and shared"""
    key = (pre, kind)
    if key not in _EVAL:
        _EVAL[key] = R.evaluate(fx[pre + kind + "_Z"], S, [fx[pre + kind + "_lam"][:R.sizes(S)[1]]])
    return _EVAL[key]


def _close(a, b, what, tol=PIN):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny)
    assert err <= tol, (what, err)


def test_fixture_is_the_documented_case(fx):
    assert float(fx["alpha"]) == ALPHA and "stand-in" in str(fx["notes"]) and "ndtri" in str(fx["notes"])
    for pre, S, kind in CASES:
        us = R.us_wave(S) if kind == "wave" else R.us_swerve(S)
        np.testing.assert_array_equal(fx[pre + kind + "_Z"], R.make_z(us, R.alphas_spread(S, ALPHA)))
        np.testing.assert_array_equal(fx[pre + kind + "_us_mat"], us)          # us_mat[t, i] = z[3t + i]
        nvar, n_nl = R.sizes(S)
        assert fx[pre + kind + "_g"].shape == (n_nl + nvar + 1,)
        np.testing.assert_array_equal(fx[pre + kind + "_lam"], R.lam_mixed(n_nl + nvar + 1))
        assert fx[pre + kind + "_jac"].shape == (n_nl + nvar + 1, nvar) and fx[pre + kind + "_hess"].shape == (nvar, nvar)


def test_fixture_was_generated_from_this_reference(fx):
    import hashlib
    ref = os.environ.get("RATO_REFERENCE", "/root/reference")
    for key, rel in (("gauss_sha256__drone__drone_gaussian_py", "drone/drone_gaussian.py"),
                     ("gauss_sha256__drone__drone_utils_py", "drone/drone_utils.py"),
                     ("ref_sha256__drone__drone_params_py", "drone/drone_params.py")):
        assert fx[key].dtype == np.uint8 and fx[key].shape == (32,)
        path = os.path.join(ref, rel)
        if os.path.exists(path):
            assert hashlib.sha256(open(path, "rb").read()).digest() == fx[key].tobytes(), path


@pytest.mark.parametrize("pre,S,kind", CASES)
def test_restatement_equals_reference(fx, pre, S, kind):
    r = _restatement(fx, pre, S, kind)
    nvar, n_nl = R.sizes(S)
    k = pre + kind
    _close(r["mus"], fx[k + "_xs"], "us_to_state_trajectory")
    _close(r["Sigmas"], fx[k + "_Sigmas"], "us_to_covariance_trajectory")
    _close(r["g_nl"], fx[k + "_g"][:n_nl], "g")
    _close(r["jac_nl"], fx[k + "_jac"][:n_nl], "jacfwd(g)")
    # the linear rows carry no second derivative, so lam[:n_nl] gives the whole Hessian
    got, ref = R.hess_blocks(r["hess"][0], S), R.hess_blocks(fx[k + "_hess"], S)
    for g, h, name in zip(got, ref, ("(u,u)", "(u,a)", "diag (a,a)")):
        assert np.max(np.abs(h)) > 1.0, name
        _close(g, h, "hess " + name)
    # and the host part of g: z itself and the allocation sum
    _close(R.g_full(fx[k + "_Z"], S, r["g_nl"]), fx[k + "_g"], "g with its linear rows")
    assert R.objective(fx[k + "_Z"], S) == pytest.approx(float(fx[k + "_f"]), rel=1e-14)


@pytest.mark.parametrize("pre,S,kind", CASES)
def test_structure_in_the_references_numbers(fx, pre, S, kind):
    k = pre + kind
    D = 3 * S
    nvar, n_nl = R.sizes(S)
    H, J = fx[k + "_hess"], fx[k + "_jac"]
    assert np.array_equal(H, H.T) or np.max(np.abs(H - H.T)) <= PIN * np.max(np.abs(H))
    aa = H[D:, D:]
    assert not np.any(aa - np.diag(np.diag(aa))), "(a,a) is exactly diagonal"
    assert not np.any(H[D + 3 * S:, :]) and not np.any(H[:, D + 3 * S:]), "a_obs rows and columns are exactly 0"
    assert np.all(np.diag(aa)[:3 * S] != 0.0)
    for i in range(3):
        for t in range(S):
            row = J[6 + i * S + t]
            assert not np.any(row[3 * (t + 1):D]), "obstacle row t does not see u[t'] for t' > t"
            alloc = row[D:].copy()
            assert alloc[t * 3 + i] < 0.0 and alloc[3 * S + i] == pytest.approx(-2 * 0.025 / 3, rel=1e-15)
            alloc[t * 3 + i] = alloc[3 * S + i] = 0.0
            assert not np.any(alloc), "an obstacle row sees its own two allocations only"
            assert not np.any(H[D + np.arange(3 * S), :D].reshape(S, 3, S, 3)[t, i, t + 1:]), "(u,a): no later control"
    r_high, r_low = 6 + 3 * S, 6 + 3 * S + 2 * (S + 1)
    for base in (r_high, r_low):
        for t in range(S + 1):
            for j in range(2):
                row = J[base + t * 2 + j]
                assert not np.any(row[D:]) and not np.any(row[3 * t:D]), "a mean row of state t: columns t' >= t are 0"
                assert not np.any(np.delete(row[:D].reshape(S, 3), j, axis=1)), "cross-axis columns are 0"
    for j in range(6):
        assert not np.any(J[j, D:]) and not np.any(np.delete(J[j, :D].reshape(S, 3), j % 3, axis=1))
    np.testing.assert_array_equal(J[n_nl:n_nl + nvar], np.eye(nvar))
    np.testing.assert_array_equal(J[-1], np.concatenate([np.zeros(D), np.ones(nvar - D)]))


def _torch_g(Z, S, c):
    """An independent torch-fp64 forward of the n_nl non-linear rows, statement by statement from the reference (:135-382),
    derivative free except for b_dx and b_dmass, which the reference defines as Jacobians and are taken by jacfwd here as
    there."""
    import torch
    f64 = torch.float64
    FG = torch.as_tensor(np.hstack([c["kp"] * np.eye(3), c["kd"] * np.eye(3)]))

    def b(x, u, mass):
        v = x[3:6]
        return torch.cat([v, (u + FG @ x) / mass - c["cd"] * torch.abs(v) * v / mass])
    D = 3 * S
    us, a_state, a_obs = Z[:D].reshape(S, 3), Z[D:D + 3 * S].reshape(S, 3), Z[D + 3 * S:]
    m = torch.tensor(c["m"], dtype=f64)
    x = torch.as_tensor(c["x0"])
    Sig = torch.zeros(6, 6, dtype=f64)
    Sw = torch.zeros(6, 6, dtype=f64)
    Sw[3:, 3:] = c["dt"] * (c["beta"] / c["m"]) ** 2 * torch.eye(3, dtype=f64)
    xs, obs = [x], [[] for _ in range(3)]
    for t in range(S):
        A = torch.eye(6, dtype=f64) + c["dt"] * torch.func.jacfwd(b, argnums=0)(x, us[t], m)
        b_dm = c["dt"] * torch.func.jacfwd(b, argnums=2)(x, us[t], m)
        Sig = A @ Sig @ A.T + Sw + c["var_m"] * torch.dot(b_dm, b_dm)
        x = x + c["dt"] * b(x, us[t], m)
        xs.append(x)
        for i in range(3):
            d = x[:2] - torch.as_tensor(c["obs"][i])
            dist = torch.linalg.norm(d)
            n = d / dist
            rad = (c["radii"][i] + c["delta"]) - (a_obs[i] / 3.0) * (2.0 * c["delta"])
            obs[i].append(-(dist - torch.special.ndtri(1 - a_state[t, i]) * torch.sqrt(n @ Sig[:2, :2] @ n) - rad))
    xs = torch.stack(xs)
    return torch.cat([x - torch.as_tensor(c["xf"]), torch.stack([torch.stack(o) for o in obs]).reshape(-1),
                      (xs[:, :2] - torch.as_tensor(R.BOUND_HIGH)).reshape(-1),
                      (-xs[:, :2] + torch.as_tensor(R.BOUND_LOW)).reshape(-1)])


@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_closed_forms_equal_torch(S):
    import torch
    c = R.constants(S)
    Z, lam = R.problems(S, 1)[0]
    r = R.evaluate(Z, S, [lam])
    Zt, lt = torch.as_tensor(Z), torch.as_tensor(lam)
    g = lambda z: _torch_g(z, S, c)
    _close(r["g_nl"], g(Zt).numpy(), "g")
    _close(r["jac_nl"], torch.func.jacfwd(g)(Zt).numpy(), "jacfwd(g)")
    H = torch.func.jacfwd(torch.func.jacfwd(lambda z: torch.dot(lt, g(z))))(Zt).numpy()
    for a, b_, name in zip(R.hess_blocks(r["hess"][0], S), R.hess_blocks(H, S), ("(u,u)", "(u,a)", "diag (a,a)")):
        _close(a, b_, "hess " + name)
    D = 3 * S
    aa = H[D:, D:]
    assert not np.any(aa - np.diag(np.diag(aa))) and not np.any(r["hess"][0][D:, D:] - np.diag(np.diag(r["hess"][0][D:, D:])))


# (S, min |d|, min n^T Sigma n) measured with us_wave and alphas_spread at alpha = 0.1
FLOORS = {1: (0.522, 6.4e-4), 2: (0.522, 1.6e-4), 3: (0.522, 7.1e-5), 5: (0.295, 2.5e-5), 20: (0.130, 1.6e-6)}


@pytest.mark.parametrize("S", sorted(FLOORS))
def test_inputs_stay_away_from_the_singularities(S):
    r = R.evaluate(R.make_z(R.us_wave(S), R.alphas_spread(S, ALPHA)), S)
    d, w = FLOORS[S]
    assert r["dist_norm"].min() == pytest.approx(d, abs=6e-4) and r["nSn"].min() == pytest.approx(w, rel=0.05)
    assert r["dist_norm"].min() >= 0.1 and r["nSn"].min() >= 1e-6
    r = R.evaluate(R.make_z(R.us_swerve(S), R.alphas_spread(S, ALPHA)), S)
    assert r["dist_norm"].min() >= 0.1 and r["nSn"].min() >= 1e-6


@pytest.mark.parametrize("S", [1, 2, 3, 5, 20, 22, 64])
def test_blended_problems_stay_away_from_the_singularities(S):
    """every (Z, lam) the GPU tests launch (measured: the smallest are 0.12 and 1.3e-6, at S = 64 and S = 20)"""
    for Z, _ in R.problems(S, 4):
        r = R.evaluate(Z, S)
        assert r["dist_norm"].min() >= 0.1 and r["nSn"].min() >= 1e-6


@pytest.mark.parametrize("pre,S,kind", [("", 20, "wave"), ("s5_", 5, "swerve")])
def test_ipopt_callbacks_assemble_the_scripts_arrays(fx, pre, S, kind):
    """the facade's host assembly, fed the REFERENCE'S arrays through an injected host implementation"""
    from riskaversetrajopt_amd import drone_gaussian as DG
    k = pre + kind
    Z, lam = fx[k + "_Z"], fx[k + "_lam"]
    nvar, n_nl = R.sizes(S)
    calls = []

    def linearize(z):
        calls.append(z.copy())
        np.testing.assert_array_equal(z, Z)
        return fx[k + "_g"][:n_nl], fx[k + "_jac"][:n_nl]

    def hessian(z, l):
        np.testing.assert_array_equal(l, lam[:n_nl])
        return R.tril(fx[k + "_hess"])
    m = DG.Model(S, alpha=ALPHA)
    cb = m.ipopt_callbacks(host=dict(linearize=linearize, hessian=hessian))
    assert cb["nvar"] == nvar and cb["ncon"] == n_nl + nvar + 1
    np.testing.assert_array_equal(cb["g_L"], fx[k + "_gL"])
    np.testing.assert_array_equal(cb["g_U"], fx[k + "_gU"])
    assert cb["g_L"][6] == -1e15 and cb["g_L"][n_nl + 3 * S] == 1e-6 and cb["g_U"][n_nl + 3 * S] == ALPHA
    assert cb["g_L"][-1] == 0.0 and cb["g_U"][-1] == ALPHA and cb["g_L"][n_nl] == -10 and cb["g_U"][n_nl] == 10
    g = cb["eval_g"](Z, np.empty(cb["ncon"]))
    J = cb["eval_jac_g"](Z, np.empty(cb["ncon"] * nvar))
    assert len(calls) == 1, "eval_g and eval_jac_g at the same x share one evaluation"
    _close(g, fx[k + "_g"], "eval_g")
    np.testing.assert_array_equal(J.reshape(cb["ncon"], nvar), fx[k + "_jac"])       # dense, row-major, constant rows included
    assert cb["eval_f"](Z) == pytest.approx(float(fx[k + "_f"]), rel=1e-14)
    dt = 50.0 / S
    np.testing.assert_allclose(cb["eval_grad_f"](Z, np.empty(nvar)), np.concatenate([4 * dt * Z[:3 * S], np.zeros(nvar - 3 * S)]),
                               rtol=1e-15)
    h = cb["eval_h"](Z, lam, 0.7, np.empty(nvar * (nvar + 1) // 2))
    Hf = np.diag(np.concatenate([np.full(3 * S, 4 * dt), np.zeros(nvar - 3 * S)]))
    _close(h, R.tril(0.7 * Hf + fx[k + "_hess"]), "eval_h")
    i1, i2 = cb["eval_jac_g_sparsity_indices"]
    assert i1.shape == (cb["ncon"] * nvar,) and i1[nvar] == 1 and i2[nvar - 1] == nvar - 1
    r, c_ = cb["eval_h_sparsity_indices"]
    assert np.array_equal(r, np.tril_indices(nvar)[0]) and np.array_equal(c_, np.tril_indices(nvar)[1])
    # the layout helpers and the reference's error text
    assert np.array_equal(m.convert_us_vec_to_us_mat(Z[:3 * S]), fx[k + "_us_mat"])
    assert np.array_equal(m.convert_us_mat_to_us_jaxvec(fx[k + "_us_mat"]), Z[:3 * S])
    np.testing.assert_array_equal(m.initial_guess_alphas_risk(), R.alphas_uniform(S, ALPHA))
    with pytest.raises(FileNotFoundError, match="run drone_risk.py first"):
        m.initial_guess_us_mat(os.path.join(HERE, "no_such_dir"))


def test_driver_converges_on_the_restatement():
    """run_drone_gaussian(callbacks=<restatement>) at S = 5, alpha = 0.1 from the prototype's start point (all u_x = 0.05,
    uniform allocation).  Measured here: status 1 (gtol) after 219 iterations / 283 evaluations, objective 0.95671383
    (7.5e-6 relative from the prototype's 0.95670661 with torch callbacks), violation 3.4e-12, optimality 9.5e-9."""
    from riskaversetrajopt_amd import drone_gaussian as DG
    from riskaversetrajopt_amd import scp
    S = 5
    cb = R.callbacks(S, ALPHA)
    m = DG.Model(S, alpha=ALPHA)
    res = scp.run_drone_gaussian(m, Z0=R.start_point(S, ALPHA), callbacks=cb)
    print({k: v for k, v in res.items() if np.ndim(v) == 0})
    assert res["status"] in (1, 2), res["message"]
    g = R.evaluate(res["Z"], S)["g_nl"]
    al = res["alphas_risk"]
    viol = max(np.max(np.abs(g[:6])), np.max(g[6:]), np.max(1e-6 - al), np.max(al - ALPHA), np.sum(al) - ALPHA,
               np.max(np.abs(res["us"])) - 10.0, 0.0)
    assert viol <= 1e-8 and res["constr_violation"] <= 1e-8
    assert res["optimality"] <= 1e-6
    assert R.objective(res["Z"], S) == pytest.approx(0.95670661, rel=1e-4)
    assert res["us"].shape == (S, 3) and res["xs"].shape == (S + 1, 6) and res["Sigmas"].shape == (S + 1, 6, 6)
    np.testing.assert_array_equal(res["xs"], R.dense_trajectory(res["us"], S)[0])
    assert 0.0 <= res["callback_s"] <= res["total_s"] and res["nfev"] >= res["nit"] > 0

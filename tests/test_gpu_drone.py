"""GPU parity: drone HIP path (through the C ABI) vs the fp64 oracle and the
committed golden fixtures; full-size properties at BASELINE config C2."""
import os

import numpy as np
import pytest

from tests import _tol as tol

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _models(S, M, seed=0, method='saa', alpha=0.1):
    from oracle import drone as od
    from riskaversetrajopt_amd import drone_risk
    rng = np.random.RandomState(seed)
    DWs, masses, obs_Qs = od.sample_uncertain_parameters(rng, method, M=M, S=S)
    return od.Model(S, DWs, masses, obs_Qs, method, alpha), drone_risk.Model(S, DWs, masses, obs_Qs, method, alpha)


def graze(S):
    t = np.arange(S)[:, None]
    return np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)


def test_sampler_draw_order_matches_oracle():
    from oracle import drone as od
    from riskaversetrajopt_amd import drone_utils
    a = od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=7, S=20)
    np.random.seed(0)
    b = drone_utils.sample_uncertain_parameters('saa', M=7)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    a = od.sample_uncertain_parameters(np.random.RandomState(3), 'baseline', M=5, S=20)
    b = drone_utils.sample_uncertain_parameters('baseline', M=5, rng=np.random.RandomState(3))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("S,M", [(20, 300), (50, 257), (30, 64), (7, 1)])
def test_rollout_and_constraints_vs_oracle(S, M):
    o, d = _models(S, M)
    us = graze(S)
    xs_o = o.us_to_state_trajectories(us)
    np.testing.assert_allclose(d.us_to_state_trajectories(us), xs_o, rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)
    g_o = o.obstacle_avoidance_constraints(xs_o, o.obs_Qs)
    _, _, g = d.eval_device(us, want_g=True)
    np.testing.assert_allclose(g.permute(2, 0, 1).cpu().numpy(), g_o, rtol=tol.G_RTOL, atol=tol.G_ATOL)
    # obstacle_avoidance_constraints on given trajectories (single-sample and batched forms)
    np.testing.assert_allclose(d.obstacle_avoidance_constraints(xs_o, o.obs_Qs), g_o, rtol=tol.G_RTOL, atol=tol.G_ATOL)
    np.testing.assert_allclose(d.obstacle_avoidance_constraints(xs_o[0], o.obs_Qs[0]), g_o[0],
                               rtol=tol.G_RTOL, atol=tol.G_ATOL)
    # single-sample rollout API
    np.testing.assert_allclose(d.us_to_state_trajectory(us, o.masses[0], o.DWs[0]), xs_o[0],
                               rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)
    ok_o, Z_o = o.monte_carlo_no_collisions_constraint_verification(us)
    ok, Z = d.monte_carlo_no_collisions_constraint_verification(us)
    np.testing.assert_allclose(Z, Z_o, rtol=tol.G_RTOL, atol=tol.G_ATOL)
    tol.assert_satisfied_close(ok, Z_o)


# (cols_per_thread, samples_per_lane); cols_per_thread = -1 is the row-parallel adjoint kernel (the default)
VARIANTS = [(4, 1), (8, 1), (16, 1), (32, 1), (4, 2), (8, 2), (2, 4), (4, 4), (-1, 1)]


@pytest.mark.parametrize("S,M,cpt,spl", [(20, 300, 0, 0), (50, 130, 0, 0), (2, 5, 4, 1), (2, 5, -1, 1), (1, 3, 0, 0),
                                          (33, 65, 8, 2), (20, 1031, 4, 4), (50, 517, 2, 4), (50, 517, -1, 1),
                                          (120, 70, 0, 0), (125, 3, -1, 1), (130, 9, 0, 0)]
                         + [(20, 101, c, l) for c, l in VARIANTS] + [(50, 70, c, l) for c, l in VARIANTS])
def test_linearization_vs_oracle(S, M, cpt, spl):
    o, d = _models(S, M)
    us = graze(S)
    fdu_o, flo_o, _, gdu_o, gup_o = o.get_all_constraints_coeffs(us)
    r = d.linearize_device(us, cols_per_thread=cpt, samples_per_lane=spl)
    gdu = d.expand_g_obs_du(r)
    tol.assert_jac_close(gdu, gdu_o, what="g_obs_du")
    # exact structural zeros survive the packing
    assert np.all(gdu[gdu_o == 0.0] == 0.0)
    tol.assert_gup_close(r["g_up"].permute(2, 0, 1).cpu().numpy(), gup_o, rtol=tol.GUP_RTOL, atol=tol.GUP_ATOL, what="g_up")
    _, Z_o = o.monte_carlo_no_collisions_constraint_verification(us)
    np.testing.assert_allclose(r["Z"].cpu().numpy(), Z_o, rtol=tol.G_RTOL, atol=tol.G_ATOL)
    fdu = d.expand_final_du(r["du_sum"].cpu().numpy(), 1.0 / M)
    np.testing.assert_allclose(fdu, fdu_o.mean(0), rtol=tol.MEAN_RTOL, atol=tol.MEAN_ATOL)
    np.testing.assert_allclose(r["rhs_sum"].cpu().numpy() / M, flo_o.mean(0), rtol=tol.MEAN_RTOL, atol=2e-5)


@pytest.mark.parametrize("S,M", [(20, 300), (50, 130), (2, 5), (125, 3)])
def test_products_output_of_rows_kernel_vs_oracle(S, M):
    """the row-parallel kernel writing the products (un-factored) Jacobian; the default is factored"""
    o, d = _models(S, M)
    us = graze(S)
    _, _, _, gdu_o, gup_o = o.get_all_constraints_coeffs(us)
    r = d.linearize_device(us, cols_per_thread=-1, factored=False)
    assert not r["factored"] and r["W"] is None
    gdu = d.expand_g_obs_du(r)
    tol.assert_jac_close(gdu, gdu_o, what="g_obs_du")
    assert np.all(gdu[gdu_o == 0.0] == 0.0)
    tol.assert_gup_close(r["g_up"].permute(2, 0, 1).cpu().numpy(), gup_o, rtol=tol.GUP_RTOL, atol=tol.GUP_ATOL, what="g_up")
    f = d.linearize_device(us, cols_per_thread=-1, factored=True)
    assert f["factored"]
    # same factors, different association of dt/m ((w dt/m) mu  vs  w (mu dt/m)): equal to a few fp32 ulp
    a, b = d.packed_jacobian(f).cpu().numpy(), d.packed_jacobian(r).cpu().numpy()
    assert np.all(np.abs(a - b) <= 4e-7 * np.abs(b)) and np.array_equal(a == 0.0, b == 0.0)
    with pytest.raises(Exception):
        d.linearize_device(us, cols_per_thread=4, factored=True)       # column kernels only write products


def test_variants_agree_and_are_deterministic():
    """Every kernel variant computes the same linearization up to fp32 rounding, and each one is
    bitwise reproducible run to run (fixed reduction order; the LDS work queue only decides WHICH
    wave sweeps a row, not the arithmetic)."""
    from riskaversetrajopt_amd.drone_risk import untile
    M = 200
    _, d = _models(50, M)
    us = graze(50)
    ref = d.linearize_device(us, cols_per_thread=4, samples_per_lane=1)
    assert not ref["factored"]
    b = d.packed_jacobian(ref).cpu().numpy()
    for cpt, spl, fact in [(c, l, False) for c, l in VARIANTS] + [(-1, 1, True)]:
        r = d.linearize_device(us, cols_per_thread=cpt, samples_per_lane=spl, factored=fact)
        assert r["factored"] == fact and (r["W"] is not None) == fact
        a = d.packed_jacobian(r).cpu().numpy()
        assert np.all(np.abs(a - b) <= 2e-6 * np.abs(b).max(axis=(0, 1, 2), keepdims=True) + 1e-12), (cpt, spl)
        assert np.array_equal(a == 0.0, b == 0.0)
        np.testing.assert_allclose(r["g_up"].cpu().numpy(), ref["g_up"].cpu().numpy(), rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(r["du_sum"].cpu().numpy(), ref["du_sum"].cpu().numpy(), rtol=1e-5)
        np.testing.assert_allclose(r["rhs_sum"].cpu().numpy(), ref["rhs_sum"].cpu().numpy(), rtol=1e-5, atol=1e-3)
        again = d.linearize_device(us, cols_per_thread=cpt, samples_per_lane=spl, factored=fact)
        assert bool((untile(again["G"], M) == untile(r["G"], M)).all()), (cpt, spl)
        if fact:
            assert bool((again["W"] == r["W"]).all())
        assert bool((again["g_up"] == r["g_up"]).all()) and bool((again["Z"] == r["Z"]).all())
        np.testing.assert_array_equal(again["du_sum"].cpu().numpy(), r["du_sum"].cpu().numpy())
        np.testing.assert_array_equal(again["rhs_sum"].cpu().numpy(), r["rhs_sum"].cpu().numpy())


def test_single_sample_api_matches_reference_shapes():
    S = 20
    o, d = _models(S, 4)
    us = graze(S)
    fdu_o, flo_o, fup_o, gdu_o, gup_o = o.get_all_constraints_coeffs(us)
    i = 2
    v_final_du, lo, up, g_obs_du, g_up = d.get_all_constraints_coeffs(us, o.masses[i], o.DWs[i], o.obs_Qs[i])
    assert v_final_du.shape == (6, 3 * S) and g_obs_du.shape == (3, S, 3 * S) and g_up.shape == (3, S)
    tol.assert_jac_close(v_final_du, fdu_o[i], what="v_final_du")
    tol.assert_jac_close(g_obs_du, gdu_o[i], what="g_obs_du")
    np.testing.assert_allclose(lo, flo_o[i], rtol=1e-5, atol=2e-5)
    assert np.array_equal(lo, up)
    tol.assert_gup_close(g_up, gup_o[i], rtol=tol.GUP_RTOL, atol=tol.GUP_ATOL, what="g_up")


def test_baseline_method_is_nominal_rollout():
    o, d = _models(20, 9, method='baseline')
    us = graze(20)
    xs = d.us_to_state_trajectories(us)
    assert np.all(xs == xs[0:1])
    np.testing.assert_allclose(xs, o.us_to_state_trajectories(us), rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)


@pytest.mark.parametrize("name", ["drone_S20_M16", "drone_S50_M8"])
def test_golden_fixture(name):
    from riskaversetrajopt_amd import drone_risk
    f = np.load(os.path.join(G, name + ".npz"))
    S, M = int(f["S"]), int(f["M"])
    d = drone_risk.Model(S, f["DWs"], f["masses"], f["obs_Qs"], 'saa', float(f["alpha"]))
    for kind in ("init", "graze"):
        us = f[f"{kind}_us"]
        np.testing.assert_allclose(d.us_to_state_trajectories(us), f[f"{kind}_xs"],
                                   rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)
        gdu, gup = d.get_all_constraints_coeffs_batched(us)
        tol.assert_jac_close(gdu, f[f"{kind}_g_obs_du"], what="g_obs_du")
        tol.assert_gup_close(gup, f[f"{kind}_g_up"], rtol=tol.GUP_RTOL, atol=tol.GUP_ATOL, what="g_up")
        fdu, flo, fup = d.sample_means(us)
        np.testing.assert_allclose(fdu, f[f"{kind}_final_du_mean"], rtol=tol.MEAN_RTOL, atol=tol.MEAN_ATOL)
        np.testing.assert_allclose(flo, f[f"{kind}_final_low_mean"], rtol=tol.MEAN_RTOL, atol=2e-5)
        ok, Z = d.monte_carlo_no_collisions_constraint_verification(us)
        np.testing.assert_allclose(Z, f[f"{kind}_Z"], rtol=tol.G_RTOL, atol=tol.G_ATOL)
        st = d.monte_carlo_statistics(us, alpha=0.3)
        assert abs(st["var"] - f[f"{kind}_var"]) < tol.RISK_ATOL * max(1.0, abs(f[f"{kind}_var"]))
        assert abs(st["cvar"] - f[f"{kind}_avar"]) < tol.RISK_ATOL * max(1.0, abs(f[f"{kind}_avar"]))


def test_full_size_C2_properties():
    """BASELINE config 2 (M=1e4, S=50): size-independent properties + a sampled
    comparison with the oracle."""
    import torch
    from oracle import drone as od, stats as ostats
    S, M = 50, 10000
    o, d = _models(S, M, seed=0)
    us = graze(S)
    r = d.linearize_device(us)
    from riskaversetrajopt_amd.drone_risk import untile
    assert r["factored"]                                            # default representation: (W, Phi)
    G_dev = d.packed_jacobian(r)                                    # (n_pairs,2,3,M)
    # linearity of the linearization: g_up + g == G.u (row sums through the packed layout)
    _, _, g = d.eval_device(us, want_g=True)
    u = torch.as_tensor(us, dtype=torch.float32, device=G_dev.device)
    Gu = torch.zeros_like(g)
    for t in range(1, S):
        off = t * (t - 1) // 2
        blk = G_dev[off:off + t]                                    # (t,2,3,M)
        Gu[:, t, :] = (blk * u[:t, :2, None, None]).sum(dim=(0, 1))
    resid = (r["g_up"] + g - Gu).abs().max().item()
    tol.report("C2 linearity |g_up + g - G.u| (fp32 row sums of up to 49 products, |g| up to ~1e3)", resid, tol.LINEARITY_ABS_DRONE_C2)
    assert resid < tol.LINEARITY_ABS_DRONE_C2, resid
    # Z from linearize == Z from eval (same formulas, two kernels)
    Z_eval, _, _ = d.eval_device(us)
    assert (Z_eval - r["Z"]).abs().max().item() <= 1e-5 * max(1.0, Z_eval.abs().max().item())
    # statistics vs the oracle on all 1e4 samples
    ok_o, Z_o = o.monte_carlo_no_collisions_constraint_verification(us)
    st = d.monte_carlo_statistics(us, alpha=0.1)
    assert abs(st["frac_satisfied"] - ok_o.mean()) <= np.sum(np.abs(Z_o - 1e-6) < tol.NEAR_THRESHOLD) / M + 1e-12
    assert abs(st["var"] - ostats.monte_carlo_var(Z_o, 0.1)) < 2e-4 * max(1.0, abs(st["var"]))
    assert abs(st["cvar"] - ostats.monte_carlo_avar(Z_o, 0.1)) < 2e-4 * max(1.0, abs(st["cvar"]))
    # sampled Jacobian comparison
    idx = np.arange(0, M, 997)
    sub = od.Model(S, o.DWs[idx], o.masses[idx], o.obs_Qs[idx])
    _, _, _, gdu_o, _ = sub.get_all_constraints_coeffs(us)
    gdu = d.expand_g_obs_du(G_dev[..., torch.as_tensor(idx, device=G_dev.device)])
    tol.assert_jac_close(gdu, gdu_o, what="g_obs_du (sampled)")
    # means vs the oracle over the full batch (oracle evaluated in chunks of 1000 samples)
    acc = np.zeros((6, 3 * S))
    for lo in range(0, M, 1000):
        sl = slice(lo, lo + 1000)
        part = od.Model(S, o.DWs[sl], o.masses[sl], o.obs_Qs[sl])
        Phi = part.sensitivities(us, part.us_to_state_trajectories(us))
        for a in range(3):
            acc[a, a::3] += Phi[:, S, a, :, 0].sum(0)
            acc[3 + a, a::3] += Phi[:, S, a, :, 1].sum(0)
    np.testing.assert_allclose(d.expand_final_du(r["du_sum"].cpu().numpy(), 1.0 / M), acc / M,
                               rtol=tol.MEAN_RTOL, atol=tol.MEAN_ATOL)


def test_captured_step_graph_matches_eager():
    import torch
    from riskaversetrajopt_amd import stats
    from riskaversetrajopt_amd.drone_risk import untile
    S, M = 50, 3000
    _, d = _models(S, M)
    step = d.capture_step(alpha=0.1)
    for scale in (1.0, 0.6):
        us = graze(S) * scale
        out, st = step.replay(us)
        torch.cuda.synchronize()
        eager = d.linearize_device(us)
        assert bool((untile(out["G"], M) == untile(eager["G"], M)).all()) and bool((out["W"] == eager["W"]).all())
        assert bool((out["g_up"] == eager["g_up"]).all()) and bool((out["Z"] == eager["Z"]).all())
        np.testing.assert_array_equal(out["sums"].cpu().numpy(), eager["sums"].cpu().numpy())
        ref = stats.risk_stats_device(eager["Z"], 0.1).cpu().numpy()
        np.testing.assert_array_equal(st.cpu().numpy(), ref)


def test_bad_arguments_are_rejected_not_computed():
    import ctypes as C
    import torch
    from riskaversetrajopt_amd import _lib, drone_risk
    _, d = _models(20, 8)
    with pytest.raises(ValueError):
        d.eval_device(np.zeros((19, 3)))                        # wrong horizon
    with pytest.raises(_lib.RatoError):
        d.linearize_device(graze(20), cols_per_thread=5)        # no such kernel variant
    with pytest.raises(_lib.RatoError):
        drone_risk.Model.from_device(20, torch.zeros((20, 3, 8), dtype=torch.float64, device="cuda"),
                                     torch.ones(8, device="cuda"), torch.zeros((3, 3, 8), device="cuda"))
    lib = _lib.load()
    p = d._params(0, 8)                                         # M = 0: empty batch is an error, not a no-op
    z = torch.zeros(8, device="cuda")
    rc = lib.rato_drone_eval(C.byref(p), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, None,
                             _lib.current_stream())
    assert rc == -1
    p = d._params(8, 4)                                         # ld < M
    assert lib.rato_drone_eval(C.byref(p), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None,
                               None, _lib.current_stream()) == -1
    p = d._params(8, 8)
    assert lib.rato_drone_eval(C.byref(p), None, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, None,
                               _lib.current_stream()) == -1     # null input pointer


def test_padded_tile_layout_is_shared_by_producer_and_consumers():
    """Tiles of >= 1 MiB start on 2 MiB boundaries (rato_packed_tile_stride): the products output at S = 50 is such a
    layout (1.88 MB per 64-sample tile).  The buffer linearize_device hands out has that stride and alignment, and
    what the consumers read from it (untile, rato_saa_rowmax, rato_emit_csc_values) equals what they get from the
    factored output of the same samples, whose tiles are packed back to back."""
    import torch
    from riskaversetrajopt_amd import _lib
    from riskaversetrajopt_amd.drone_risk import untile, num_pairs
    S, M = 50, 200
    _, d = _models(S, M)
    lib = d._lib
    us = graze(S)
    rp = d.linearize_device(us, factored=False)
    rf = d.linearize_device(us, factored=True)
    payload = num_pairs(S) * 2 * 3 * rp["tile"]
    stride = lib.rato_packed_tile_stride(payload)
    assert payload * 4 >= (1 << 20) and stride % ((2 << 20) // 4) == 0 and stride > payload
    assert rp["G"].stride(0) == stride and rp["G"].data_ptr() % (2 << 20) == 0 and rp["G"][0].is_contiguous()
    assert rf["G"].is_contiguous() and lib.rato_packed_tile_stride(num_pairs(S) * 2 * rf["tile"]) == num_pairs(S) * 2 * rf["tile"]
    # the same Jacobian through both representations
    Gp, Gf = d.packed_jacobian(rp), d.packed_jacobian(rf)                   # (n_pairs, 2, n_obs, M)
    scale = Gp.abs().max().item()
    assert (Gp - Gf).abs().max().item() <= 2e-6 * scale
    # a buffer of an earlier call is reused only in this layout
    again = d.linearize_device(us, factored=False, out=rp)
    assert again["G"].data_ptr() == rp["G"].data_ptr()
    wrong = dict(rp, G=torch.empty(tuple(rp["G"].shape), device=rp["G"].device))     # back-to-back tiles: not the layout
    fresh = d.linearize_device(us, factored=False, out=wrong)
    assert fresh["G"].data_ptr() != wrong["G"].data_ptr() and fresh["G"].stride(0) == stride
    # consumers: rowmax and CSC emission from the padded products buffer == from the factored one
    ld = rp["_g_up"].shape[-1]
    u_dev = torch.as_tensor(us + 0.1, dtype=torch.float64, device=rp["G"].device).contiguous()
    res = []
    for r in (rp, rf):
        m = torch.empty(M, dtype=torch.float32, device=u_dev.device)
        a = torch.empty(M, dtype=torch.int32, device=u_dev.device)
        _lib.check(lib.rato_saa_rowmax(_lib.ptr(r["G"]), _lib.ptr(r["_W"]), r["tile"], 3, S, M, ld, _lib.ptr(r["_g_up"]),
                                       -1.0, _lib.ptr(u_dev), 3, _lib.ptr(m), _lib.ptr(a), _lib.current_stream()), "rowmax")
        vals = torch.empty(M * 3 * 2 * num_pairs(S), dtype=torch.float32, device=u_dev.device)
        _lib.check(lib.rato_emit_csc_values(_lib.ptr(r["G"]), _lib.ptr(r["_W"]), ld, r["tile"], 2, 3, S, M, 0.01,
                                            _lib.ptr(vals), _lib.current_stream()), "emit_csc")
        res.append((m.cpu().numpy(), vals.cpu().numpy()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=0, atol=2e-5 * max(1.0, np.abs(res[1][0]).max()))
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=0, atol=2e-6 * 0.01 * scale)


def test_ragged_last_tile_at_the_C2_size():
    """M = 10,007 (prime; BASELINE C2 is 10,000): ld = 10,008, the last 64-sample tile holds 23 samples.  Samples around
    the tile boundaries against the fp64 oracle on the same device-drawn numbers, exact statistics, run-to-run bitwise."""
    import torch
    from riskaversetrajopt_amd import drone_risk, drone_utils, stats
    from tests._drone_shapes import oracle_model
    S, M = 50, 10007
    dW, mass, Qsym = drone_utils.sample_uncertain_parameters_device(M, S, seed=5)
    d = drone_risk.Model.from_device(S, dW, mass, Qsym, 'saa', 0.1, M=M)
    t = np.arange(S)[:, None]
    us = np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)
    r = d.linearize_device(us)
    idx = np.array([0, 63, 64, 9983, 9984, 10000, 10006])
    ti = torch.as_tensor(idx, device=dW.device)
    sub = oracle_model(dW[:, :, ti].cpu().numpy(), mass[ti].cpu().numpy(), Qsym[:, :, ti].cpu().numpy())
    _, _, _, gdu_o, gup_o = sub.get_all_constraints_coeffs(us)
    gdu = d.expand_g_obs_du(d.packed_jacobian(r)[..., ti])
    tol.assert_jac_close(gdu, gdu_o, what="g_obs_du (ragged tile)")
    assert np.array_equal(gdu == 0.0, gdu_o == 0.0)
    tol.assert_gup_close(r["g_up"].permute(2, 0, 1).cpu().numpy()[idx], gup_o, rtol=tol.GUP_RTOL, atol=tol.GUP_ATOL)
    _, Z_o = sub.monte_carlo_no_collisions_constraint_verification(us)
    np.testing.assert_allclose(r["Z"][ti].cpu().numpy(), Z_o, rtol=tol.G_RTOL, atol=tol.G_ATOL)
    Zh = r["Z"][:M].cpu().numpy().astype(np.float64)
    st = stats.risk_stats(r["Z"][:M], 0.1)
    srt = np.sort(Zh)
    assert st["var"] == srt[M - int(np.floor(0.1 * M)) - 1] and st["max"] == srt[-1]
    again = d.linearize_device(us)                     # (lanes >= M of the last tile are not written: compare the samples)
    assert bool((d.packed_jacobian(again) == d.packed_jacobian(r)).all()) and bool((again["Z"][:M] == r["Z"][:M]).all())


@pytest.mark.parametrize("M,S,factored", [(300, 20, False), (10007, 50, False), (100000, 50, True), (100000, 50, False), (5000, 126, False)])
def test_tiled_noise_gives_the_same_linearization_bit_for_bit(M, S, factored):
    """rato_drone_linearize_tiled (the noise re-tiled once per batch: one contiguous block per tile of 64 samples) against
    rato_drone_linearize on the [S][3][ld] array: every output identical (static grid, split tiles, tile queue)."""
    import torch
    from riskaversetrajopt_amd import drone_risk, drone_utils
    dW, mass, Q = drone_utils.sample_uncertain_parameters_device(M, S, seed=4)
    d = drone_risk.Model.from_device(S, dW, mass, Q, 'saa', 0.1, M=M)
    t = np.arange(S)[:, None]
    us = np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)
    assert drone_risk.Model.TILED_NOISE
    a = d.linearize_device(us, factored=factored)
    try:
        drone_risk.Model.TILED_NOISE = False
        b = d.linearize_device(us, factored=factored)
    finally:
        drone_risk.Model.TILED_NOISE = True
    torch.cuda.synchronize()
    for k in ("g_up", "Z", "sums", "part"):
        assert torch.equal(a[k], b[k]), k
    if factored:
        assert torch.equal(a["W"], b["W"])
    if M <= 10007:
        assert torch.equal(drone_risk.untile(a["G"], M), drone_risk.untile(b["G"], M))
    else:
        assert torch.equal(a["G"][:3], b["G"][:3]) and torch.equal(a["G"][-2:-1], b["G"][-2:-1])


def test_per_sample_linearization_never_reuses_another_samples_noise():
    """``get_all_constraints_coeffs`` builds a fresh one-sample noise array per call; the allocator
    hands the next call the same address.  Each sample's result must be that sample's own (== the oracle, == the
    un-tiled kernel), and the model's own re-tiled copy must survive the per-sample calls."""
    import torch
    from riskaversetrajopt_amd import drone_risk
    S, M = 20, 6
    o, d = _models(S, M, seed=2)
    us = graze(S)
    own = d.linearize_device(us)                                      # (caches the model's own tiled noise)
    Z_own = own["Z"].clone()
    outs = []
    for i in range(M):
        v = d.get_all_constraints_coeffs(us, o.masses[i], o.DWs[i], o.obs_Qs[i])
        fdu_o, flo_o, _, gdu_o, gup_o = (x[i] for x in o.get_all_constraints_coeffs(us))
        scale = np.abs(gdu_o).max(axis=-1, keepdims=True)
        assert np.all(np.abs(v[3] - gdu_o) <= tol.JAC_REL_ROWMAX * scale + 1e-12), i
        np.testing.assert_allclose(v[4], gup_o, rtol=tol.GUP_RTOL, atol=tol.GUP_ATOL)
        np.testing.assert_allclose(v[1], flo_o, rtol=1e-5, atol=1e-5)
        outs.append(v)
    try:
        drone_risk.Model.TILED_NOISE = False
        for i in range(M):
            w = d.get_all_constraints_coeffs(us, o.masses[i], o.DWs[i], o.obs_Qs[i])
            for a, b in zip(outs[i], w):
                assert np.array_equal(a, b), i
    finally:
        drone_risk.Model.TILED_NOISE = True
    assert not np.array_equal(outs[0][4], outs[1][4])
    assert torch.equal(d.linearize_device(us)["Z"], Z_own)


def test_in_place_noise_refill_needs_and_honours_invalidate():
    """The library's samplers write through raw pointers (no version bump): ``invalidate_noise`` / ``set_noise`` drop
    the re-tiled copy, after which linearize == the kernel that reads dW as it lies, bit for bit."""
    import torch
    from riskaversetrajopt_amd import drone_risk, drone_utils
    M, S = 3000, 20
    dW, mass, Q = drone_utils.sample_uncertain_parameters_device(M, S, seed=4)
    d = drone_risk.Model.from_device(S, dW, mass, Q, 'saa', 0.1, M=M)
    us = graze(S)
    a = d.linearize_device(us)["Z"].clone()
    dW2, _, _ = drone_utils.sample_uncertain_parameters_device(M, S, seed=5)
    d.set_noise(dW2)
    b = d.linearize_device(us)["Z"].clone()
    try:
        drone_risk.Model.TILED_NOISE = False
        c = d.linearize_device(us)["Z"].clone()
    finally:
        drone_risk.Model.TILED_NOISE = True
    assert torch.equal(b, c) and not torch.equal(a, b)
    with pytest.raises(ValueError):
        d.set_noise(dW2[:, :2].contiguous())


@pytest.mark.parametrize("S,M", [(64, 5), (20, 1), (50, 300), (33, 257)])
def test_generators_linearization_ignores_what_its_scratch_held(S, M):
    """rato_drone_linearize_generators reads its step-Jacobian table back in the adjoint pass.  A lane past the batch must
    not: its clamped address is the last sample's entry, which another wave may not have written yet when the lane's own
    wave is entirely past the batch, and a NaN left in a fresh buffer survived the multiplication by zero that was meant
    to silence the lane (round 6, found by tools/soak.py: NaN sample sums on the second call at S = 64, M = 5).  Here the
    scratch, the outputs and the partial sums are pre-filled with NaN: the results must be finite, identical to a run on
    zero-filled buffers, and equal to the oracle's sample sums."""
    import torch
    from oracle import drone as od
    from riskaversetrajopt_amd import drone_risk
    DWs, masses, Q = od.sample_uncertain_parameters(np.random.RandomState(3), 'saa', M=M, S=S)
    o, d = od.Model(S, DWs, masses, Q, 'saa', 0.1), drone_risk.Model(S, DWs, masses, Q, 'saa', 0.1)
    t = np.arange(S)[:, None]
    us = np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)
    ref = d.linearize_generators_device(us)
    ld = ref["_A22"].shape[-1]
    for fill in (float("nan"), 0.0, float("inf")):
        bufs = {"_A22": torch.full((S, 3, ld), fill, device=d.device), "_W": torch.full((3, S, 2, ld), fill, device=d.device),
                "_g_up": torch.full((3, S, ld), fill, device=d.device), "_Z": torch.full((ld,), fill, device=d.device),
                "part": torch.full(tuple(ref["part"].shape), fill, device=d.device)}
        for _ in range(3):
            r = d.linearize_generators_device(us, out=bufs)
            assert bool(torch.isfinite(r["sums"]).all()) and bool(torch.isfinite(r["g_up"]).all()), fill
            assert torch.equal(r["sums"], ref["sums"]) and torch.equal(r["g_up"], ref["g_up"]) and torch.equal(r["Z"], ref["Z"])
    fdu, flo, _, _, _ = o.get_all_constraints_coeffs(us)
    np.testing.assert_allclose(d.expand_final_du(ref["du_sum"].cpu().numpy(), 1.0 / M), fdu.mean(0), rtol=1e-5, atol=1e-6)


def test_eval_device_keeps_the_reusable_g_buffer_across_a_call_without_g():
    """``eval_device(out=o)`` without ``want_g`` used to overwrite ``o['_g']`` with None, dropping the buffer a later
    call with ``want_g`` would have reused (drone and driving facades alike)."""
    from oracle import drone as od, driving as ocar
    from riskaversetrajopt_amd import drone_risk, driving
    S, M = 20, 300
    DWs, masses, Q = od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=M, S=S)
    d = drone_risk.Model(S, DWs, masses, Q, 'saa', 0.1)
    c = driving.Model(M, 'saa', 0.1, S=S, samples=ocar.sample_uncertain_parameters(np.random.RandomState(0), M, 'saa', S))
    for m, us in ((d, d.initial_guess_us_mat()), (c, c.initial_guess_us_mat())):
        o = {}
        m.eval_device(us, want_g=True, out=o)
        g_ptr, z_ptr = o["_g"].data_ptr(), o["_Z"].data_ptr()
        m.eval_device(us, out=o)                               # no g wanted: the buffer stays
        assert o["_g"] is not None and o["_g"].data_ptr() == g_ptr and o["_Z"].data_ptr() == z_ptr
        m.eval_device(us, want_g=True, out=o)
        assert o["_g"].data_ptr() == g_ptr

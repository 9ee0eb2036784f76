"""GPU: the hopper's fp64 slip rows (csrc/hopper_slip64.hip) and ``hopper.Model(precision='f64')`` against oracle/hopper.py,
the fp64 restatement of the whole NLP (tests/_hopper_nlp.py) and the reference's own matrices (tests/golden/ref_hopper_nlp.npz).

Errors are relative to each array's max |entry|, the Hessian's per step block.  DEV_TOL is 100 x the worst error of the sweep of
test_kernel_equals_the_restatement against oracle/hopper.py, capped at 1e-12 (mu is a 30-term sum of terms <= 6.5e-3 beside 0.1
and the trig arguments lie below 16 rad: thousands of ulps would be a finding, not a bound).  Measured on the MI355X over the
sweep: h 3.3e-15, dh_dfz 8.3e-16, dh_dx 2.6e-15, Zmax 1.3e-14, D1 3.4e-15, D2 4.9e-15, D0 3.4e-15, the Hessian share 1.5e-14
(the worst, at M = 300: the mixed-sign multipliers cancel in the sums, whose rounding is relative to sum_i |lam_i term_i|, and
h = fx - mu fz cancels beside fx ~ 0.08 fz).  100 x 1.5e-14 lies above the cap, so DEV_TOL = 1e-12, 65 x the worst.  The same
lanes executed on the host give 3.0e-15 (tests/test_hopper_slip64_host.py).  The facade against the reference's fixture
(test_f64_facade_equals_the_reference_on_every_row) measured 1.5e-15 on the risk rows of g and 9.5e-15 on the slip share of
the Hessian, where the fp32 path needs rtol 1e-4 / atol 3e-5.

The derivative test (test_derivatives_through_ipopt_callbacks) measured 2.9e-10 (g against J v) and 3.1e-10 (J' lam against
H v) on every row, dense and sparse alike.  The same check on a precision='f32' model, which is the contrast the fp64 path exists
for and is not asserted: 5.5e-3 and 6.2e-3 (measured on the MI355X).
"""
import os

import numpy as np
import pytest

import _hopper_nlp as R
import _hopper_slip64 as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV_TOL = 1e-12                # min(100 x 1.5e-14, 1e-12)
PIN = 7e-14                   # the fixture's own error against the restatement (tests/test_hopper_nlp_pin.py)
FD_TOL = 1e-8
ALPHA = T.ALPHA
EPS = np.finfo(np.float64).eps
E = {(r, c): r * (r + 1) // 2 + c for r in range(12) for c in range(r + 1)}
SLIP_ENTRIES = [E[p] for p in ((0, 0), (2, 0), (3, 0), (2, 2), (3, 2), (3, 3), (11, 0), (11, 2), (11, 3))]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_hopper_nlp.npz"))


def dev_model(S, M, fields, phases=None, method="saa", precision="f64"):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, ALPHA, S=S, fields=fields, phases=phases, precision=precision)


def upload(m, Zs, pad=0):
    """Zs (K, nvar) -> device tensor [K][nvar + pad]; the padding holds NaN, which no kernel may read"""
    import torch
    buf = torch.full((Zs.shape[0], Zs.shape[1] + pad), float("nan"), dtype=torch.float64, device=m.device)
    buf[:, :Zs.shape[1]] = torch.as_tensor(Zs, device=m.device)
    return buf


def device_outputs(m, Zd, lams, add=None):
    """every output of both kernels as host arrays; the Hessian share goes into ``add`` (zeros by default)"""
    import torch
    r = m.slip_device_f64(Zd, lams)
    got = {k: r[k].cpu().numpy() for k in ("h", "dh_dfz", "dh_dx", "Zmax")}
    if lams is not None:
        K = Zd.shape[0]
        a = torch.zeros((K, m.S + 1, 78), dtype=torch.float64, device=m.device) if add is None else torch.as_tensor(add, device=m.device)
        m.slip_hess_blocks_device_f64(Zd, r["D"], a)
        got["D"], got["add"] = r["D"].cpu().numpy(), a.cpu().numpy()
        got.update(T.split_D(got["D"]))
    return got, r


# ---- 1. kernel against the restatement ---------------------------------------------------------------------------------------
_WORST = {}


@pytest.mark.parametrize("M", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("S", [1, 6, 30])
def test_kernel_equals_the_restatement(S, M):
    import torch
    worst = {}
    for phase, phases in T.phase_cases(S).items():
        fields, Zs, lams, add = T.inputs(S, M, 3, phases)
        ref = T.reference(fields, Zs, lams, np.zeros_like(add), S, phases)
        m = dev_model(S, M, fields, phases)
        Cn = m.nlp_layout()["C"]
        for K in (1, 3):
            for pad in (0, 5):
                Zd = upload(m, Zs[:K], pad)
                got, r = device_outputs(m, Zd, lams[:K])
                errs = T.errors(got, {k: v[:K] for k, v in ref.items()})
                if Cn == 0:
                    assert got["h"].shape == (K, 0, M) and not np.any(got["add"]) and np.all(got["Zmax"] == -np.inf)
                else:
                    assert set(errs) == {"h", "dh_dfz", "dh_dx", "Zmax", "D1", "D2", "D0", "hess"}
                for name, e in errs.items():
                    worst[name] = max(worst.get(name, 0.0), e)
        # without lam and with NULL outputs (K = 3, padded): what is written is bitwise what the full call wrote
        for want in (("h",), ("dh_dfz",), ("dh_dx", "Zmax"), ("h", "dh_dfz", "dh_dx"), ()):
            some = m.slip_device_f64(Zd, None, want=want)
            assert set(some) == set(want) | {"D"} and some["D"] is None
            for name in want:
                assert torch.equal(some[name], r[name]), (phase, name)
        only_sums = m.slip_device_f64(Zd, lams, want=())
        assert torch.equal(only_sums["D"], r["D"])
    print("S", S, "M", M, {k: float("%.3g" % v) for k, v in worst.items()})
    for name, err in worst.items():
        _WORST[name] = max(_WORST.get(name, 0.0), err)
    print("worst so far", {k: float("%.3g" % v) for k, v in _WORST.items()})
    for name, err in worst.items():
        assert err <= DEV_TOL, (name, err)


# ---- 2. - 4. exact zeros, zero multipliers, add --------------------------------------------------------------------------------
def test_exact_zeros_zero_multipliers_and_add():
    S, M, K = 6, 65, 2
    phases = T.phase_cases(S)["default"]
    fields, Zs, lams, add = T.inputs(S, M, K, phases, seed=5)
    m = dev_model(S, M, fields, phases)
    steps = m.contact_steps()
    # sin x2 = 0: a literal 0.0 in the x3 column, and only there
    Z0 = Zs.copy()
    Z0[:, 2:8 * (S + 1):8] = 0.0
    got0, _ = device_outputs(m, upload(m, Z0), lams)
    assert not np.any(got0["dh_dx"][:, :, 2, :]) and np.all(got0["dh_dx"][:, :, :2, :] != 0.0)
    for e, zero in (((3, 0), True), ((3, 3), True), ((11, 3), True), ((2, 2), False), ((3, 2), False), ((0, 0), False)):
        assert np.all(got0["add"][:, steps, E[e]] == 0.0) == zero, e
    # lam = 0: every sum is exactly 0 and nothing is added
    gotz, _ = device_outputs(m, upload(m, Zs), np.zeros_like(lams), add)
    assert not np.any(gotz["D"])
    np.testing.assert_array_equal(gotz["add"], add)
    # add is forwarded where no contact sits, and added to exactly once where one does
    share, _ = device_outputs(m, upload(m, Zs), lams)
    with_add, _ = device_outputs(m, upload(m, Zs), lams, add)
    touched = np.zeros((K, S + 1, 78), dtype=bool)
    touched[:, steps[:, None], np.array(SLIP_ENTRIES)[None, :]] = True
    assert not np.any(share["add"][~touched]) and np.all(share["add"][touched] != 0.0)
    np.testing.assert_array_equal(with_add["add"][~touched], add[~touched])
    np.testing.assert_array_equal(with_add["add"][touched], (add + share["add"])[touched])
    np.testing.assert_array_equal(with_add["D"], share["D"])


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,M", [(6, 30), (6, 300)])
def test_two_calls_and_batch_against_singles_are_bitwise_equal(S, M):
    import torch
    phases = T.phase_cases(S)["default"]
    fields, Zs, lams, add = T.inputs(S, M, 3, phases, seed=9)
    m = dev_model(S, M, fields, phases)
    Zd = upload(m, Zs, 5)
    a, b = m.slip_device_f64(Zd, lams), m.slip_device_f64(Zd, lams)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    batch = m.nlp_device(Zd, lams, add=add)
    assert set(batch) == {"defect", "d_defect", "rows", "d_rows", "jac_values", "hess_blocks", "hess_tril", "slip_h", "slip_rows",
                          "slip_jac_values"}
    again = m.nlp_device(Zd, lams, add=add)
    for k in range(3):
        one = m.slip_device_f64(Zd[k:k + 1], lams[k:k + 1])
        for name in a:
            assert torch.equal(a[name][k], one[name][0]), name
        single = m.nlp_device(Zs[k:k + 1], lams[k:k + 1], add=add[k:k + 1])
        for name, t in batch.items():
            assert torch.equal(t[k], single[name][0]) and torch.equal(t, again[name]), name


# ---- 6. facade against the reference's own matrices ------------------------------------------------------------------------------
def _fixture_case(fx, pre):
    import scipy.sparse as sp
    S, M = int(fx[pre + "S"]), int(fx[pre + "M"])
    fields = (fx[pre + "intensities"], fx[pre + "thetas"], fx[pre + "taus"])
    dense = lambda key: sp.csc_matrix((fx[pre + key + "_data"], fx[pre + key + "_indices"], fx[pre + key + "_indptr"]),
                                      shape=tuple(fx[pre + key + "_shape"])).toarray()
    return S, M, fields, dense("J"), dense("H")


@pytest.mark.parametrize("pre", ["", "s6_"])
def test_f64_facade_equals_the_reference_on_every_row(fx, pre):
    S, M, fields, J_fx, H_fx = _fixture_case(fx, pre)
    Z = fx[pre + "Z"]
    bound = DEV_TOL + PIN
    errs = {}
    for method in ("saa", "baseline"):
        m = dev_model(S, M, fields, method=method)
        lay = m.nlp_layout()
        risk = slice(lay["off"]["risk"], lay["off"]["control"])
        if method == "saa":
            lam, g_ref, J_ref, H_ref = fx[pre + "lam"], fx[pre + "g_saa"], J_fx, H_fx
        else:                                                     # the fixture holds g alone for the baseline
            lam = np.random.RandomState(12).uniform(-1, 1, lay["ncon"])
            g_ref, J_ref = fx[pre + "g_baseline"], R.jac_dense(Z, S, M, method, ALPHA, fields)
            H_ref = R.dense_from_blocks(R.hess_blocks_full(Z, lam, S, M, method, ALPHA, fields), S, m.num_vars)
        g = m.g(Z)
        assert g.dtype == np.float64 and g.shape == g_ref.shape
        errs["g " + method], errs["g risk rows " + method] = R.rel_err(g, g_ref), R.rel_err(g[risk], g_ref[risk])
        A = m.jac_g(Z)
        np.testing.assert_array_equal(A.indices, lay["jac_indices"])
        np.testing.assert_array_equal(A.indptr, lay["jac_indptr"])
        J = A.toarray()
        errs["jac_g " + method], errs["jac_g risk rows " + method] = R.rel_err(J, J_ref), R.rel_err(J[risk], J_ref[risk])
        B = m.hess_lagrangian_blocks(Z, lam, 0.0)
        tril = m.hess_lagrangian(Z, lam, 0.0)
        np.testing.assert_array_equal(tril, R.dense_from_blocks(B, S, m.num_vars)[np.tril_indices(m.num_vars)])
        B_ref, rest = R.blocks_from_dense(H_ref, S)
        assert not np.any(rest)
        errs["hess " + method] = R.rel_err_blocks(R.tril78(B), R.tril78(B_ref), 1)
        # the slip members on their own, against oracle/hopper.py
        o = T.oracle(fields, S, (m.time_jump, m.time_land), method)
        r0 = m.risk_rows_offset()[1]
        lam_s = lam[r0:r0 + M * lay["C"]].reshape(M, lay["C"])
        errs["slip_risk_constraints " + method] = R.rel_err(m.slip_risk_constraints(Z), o.slip_risk_constraints(Z))
        Js, Jo = m.slip_jacobian(Z), o.slip_jacobian(Z)
        assert Js.dtype == np.float64 and np.array_equal(Js.indices, Jo.indices) and np.array_equal(Js.indptr, Jo.indptr)
        errs["slip_jacobian " + method] = R.rel_err(Js.toarray(), Jo.toarray())
        Hs, Ho = m.slip_hessian(Z, lam_s), o.slip_hessian(Z, lam_s)
        assert np.array_equal(Hs.indices, Ho.indices) and np.array_equal(Hs.indptr, Ho.indptr)
        slip_blocks = R.blocks_from_dense(Ho.toarray(), S)[0]
        errs["slip_hessian " + method] = R.rel_err_blocks(R.tril78(R.blocks_from_dense(Hs.toarray(), S)[0]), R.tril78(slip_blocks), 1)
        errs["slip_hessian_blocks " + method] = R.rel_err_blocks(m.slip_hessian_blocks(Z, lam), R.tril78(slip_blocks), 1)
    print(pre, {k: float("%.3g" % v) for k, v in errs.items()})
    for what, err in errs.items():
        assert err <= bound, (what, err)
    # obj_factor hess_f: 2 R on the diagonal of u0 and u1, beside the slip share
    m = dev_model(S, M, fields)
    lam = fx[pre + "lam"]
    d = m.hess_lagrangian_blocks(Z, lam, 0.7) - m.hess_lagrangian_blocks(Z, lam, 0.0)
    want = np.zeros_like(d)
    want[:S, 8, 8] = want[:S, 9, 9] = 1.4
    np.testing.assert_allclose(d, want, rtol=0, atol=4 * EPS * np.max(np.abs(H_fx)))


def test_no_contact_step_and_device_fields():
    """time_jump = 0, time_land = S: no slip row exists and both precisions give the same numbers; fields given on the device
    (fp32) are upcast once"""
    import torch
    from riskaversetrajopt_amd import hopper
    S, M = 6, 4
    fields, Zs, lams, _ = T.inputs(S, M, 1, (0, S))
    for method in ("saa", "baseline"):
        m64, m32 = (dev_model(S, M, fields, (0, S), method, p) for p in ("f64", "f32"))
        lam = np.random.RandomState(3).uniform(-1, 1, m64.nlp_layout()["ncon"])
        Z = Zs[0]
        np.testing.assert_array_equal(m64.g(Z), m32.g(Z))
        np.testing.assert_array_equal(m64.jac_g(Z).toarray(), m32.jac_g(Z).toarray())
        np.testing.assert_array_equal(m64.hess_lagrangian(Z, lam, 0.3), m32.hess_lagrangian(Z, lam, 0.3))
        cb = m64.ipopt_callbacks(sparse=True)
        np.testing.assert_array_equal(cb["eval_g"](Z, np.empty(cb["ncon"])), m32.g(Z))
    phases = T.phase_cases(S)["default"]
    fields, Zs, lams, _ = T.inputs(S, M, 2, phases)
    host = dev_model(S, M, fields, phases)
    dev = hopper.Model.from_device(host._a, host._th, host._tau, "saa", ALPHA, S=S, precision="f64")
    for t in dev.fields_f64():
        assert t.dtype == torch.float64 and t.shape == (30, M)
    a, b = host.slip_device_f64(Zs, lams), dev.slip_device_f64(Zs, lams)
    for name in ("h", "dh_dfz", "dh_dx", "Zmax", "D"):                     # fields rounded to fp32: equal to fp32 accuracy only
        assert R.rel_err(b[name].cpu().numpy(), a[name].cpu().numpy()) <= 1e-5, name


# ---- 7. derivative test through ipopt_callbacks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_derivatives_through_ipopt_callbacks(fx, sparse):
    """central differences at h = 1e-5 along three directions with max |v| = 1, at a perturbed iterate, on ALL rows: g against
    J v relative to max |J|, J' lam against H v relative to max |H|, both within FD_TOL = 1e-8 (the host restatement meets it at
    2.9e-10; measured here 2.9e-10 / 3.1e-10; on a precision='f32' model 5.5e-3 / 6.2e-3, see the module docstring)."""
    S, M, fields, _, _ = _fixture_case(fx, "")
    m = dev_model(S, M, fields)
    cb = m.ipopt_callbacks(sparse=sparse)
    nvar, ncon = cb["nvar"], cb["ncon"]
    Z = R.problem(S, M, 0)
    lam = np.random.RandomState(50 + S).uniform(-1, 1, ncon)
    jr, jc = cb["eval_jac_g_sparsity_indices"]
    hr, hc = cb["eval_h_sparsity_indices"]

    def g_of(x):
        return cb["eval_g"](x, np.empty(ncon)).copy()

    def J_of(x):
        J = np.zeros((ncon, nvar))
        J[jr, jc] = cb["eval_jac_g"](x, np.empty(jr.size))
        return J
    J = J_of(Z)
    H = np.zeros((nvar, nvar))
    H[hr, hc] = cb["eval_h"](Z, lam, 0.0, np.empty(hr.size))
    H = H + np.tril(H, -1).T
    lay = m.nlp_layout()
    risk = slice(lay["off"]["risk"], lay["off"]["control"])
    assert np.max(np.abs(J)) > 1.0 and np.max(np.abs(H)) > 1.0 and np.max(np.abs(J[risk])) > 1.0
    h = 1e-5
    for v in R.directions(nvar):
        e_g = np.max(np.abs((g_of(Z + h * v) - g_of(Z - h * v)) / (2 * h) - J @ v)) / np.max(np.abs(J))
        e_h = np.max(np.abs((J_of(Z + h * v) - J_of(Z - h * v)).T @ lam / (2 * h) - H @ v)) / np.max(np.abs(H))
        print("fd through ipopt_callbacks, sparse =", sparse, e_g, e_h)
        assert e_g <= FD_TOL and e_h <= FD_TOL


# ---- 8. eval_g and eval_jac_g share one slip evaluation ---------------------------------------------------------------------------
def test_eval_g_and_eval_jac_g_share_one_slip_evaluation(fx, monkeypatch):
    S, M, fields, _, _ = _fixture_case(fx, "s6_")
    m = dev_model(S, M, fields)
    Z = fx["s6_Z"]
    calls = []
    entry = m._lib.rato_hopper_slip_f64

    def counted(*args):
        calls.append(1)
        return entry(*args)
    monkeypatch.setattr(m._lib, "rato_hopper_slip_f64", counted)
    for sparse in (False, True):
        cb = m.ipopt_callbacks(sparse=sparse)
        n = cb["eval_jac_g_sparsity_indices"][0].size
        del calls[:]
        g = cb["eval_g"](Z, np.empty(cb["ncon"]))
        cb["eval_jac_g"](Z, np.empty(n))
        assert len(calls) == 1, "eval_g followed by eval_jac_g at the same x"
        cb["eval_jac_g"](Z + 1e-3, np.empty(n))
        np.testing.assert_array_equal(cb["eval_g"](Z, np.empty(cb["ncon"])), g)
        assert len(calls) == 3, "a new x is a new evaluation"


# ---- 9. the C4 size once -----------------------------------------------------------------------------------------------------------
def test_hessian_sums_at_the_c4_size():
    """M = 5e4, C = 40 (S = 60), K = 1: D1 / D2 / D0 against fp64 sums of oracle/hopper.py's terms, within DEV_TOL sum_i |lam_i
    term_i| per entry.  Measured on the MI355X: |D - ref| <= 4.1e-17 sum |terms|, i.e. 2.3e-13 of |D2| at worst (2.2e-14 of |D1|,
    1.3e-14 of |D0|); the fp32 path is bounded at atol 2.2e-2 on D2 at this size (tests/test_gpu_hopper.py)."""
    from oracle import hopper as oh
    S, M = 60, 50000
    phases = (S // 3, 2 * S // 3)
    rng = np.random.RandomState(44)
    fields = oh.sample_friction_fields(rng, M)
    Z = R.problem(S, M, 0)
    m = dev_model(S, M, fields, phases)
    ncon, r0 = m.risk_rows_offset()
    Cn = 40
    lam = np.zeros((1, ncon))
    lam[0, r0:r0 + M * Cn] = rng.uniform(-1, 1, M * Cn)
    D = m.slip_device_f64(Z[None], lam, want=())["D"][0].cpu().numpy()            # (C, 3) = D1, D2, D0
    o = T.oracle(fields, S, phases)
    px, forces = o.contact_inputs(Z)
    lam_s = lam[0, r0:r0 + M * Cn].reshape(M, Cn)
    ref, mass = np.zeros((Cn, 3)), np.zeros((Cn, 3))
    for i0 in range(0, M, 5000):                                                 # the (M, C, 30) arrays, a slice of the samples at a time
        sl = slice(i0, i0 + 5000)
        _, dmu, d2mu = oh.friction_derivatives(px, o.intensities[sl], o.thetas[sl], o.taus[sl])
        terms = np.stack([-lam_s[sl] * dmu, -lam_s[sl] * d2mu * forces[None, :, 1], -lam_s[sl] * dmu * forces[None, :, 1]], -1)
        ref += terms.sum(axis=0)
        mass += np.abs(terms).sum(axis=0)
    assert np.all(np.isfinite(D)) and np.all(mass > 10 * np.abs(ref)), "mixed-sign multipliers: the sums cancel"
    ratio = np.abs(D - ref) / mass
    print("C4 sums: worst |D - ref| / sum |terms|", ratio.max(axis=0), "worst relative to |sum|", (np.abs(D - ref) / np.abs(ref)).max(axis=0))
    assert np.all(np.abs(D - ref) <= DEV_TOL * mass)

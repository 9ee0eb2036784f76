"""CPU: the hopper's fp64 slip rows (csrc/hopper_slip64.hip, csrc/rato_hopper_slip64.h) without a device.

  * tests/host/hopper_slip64_host.hip executes every lane of both grids in host loops, with the kernels' own per-lane functions
    and order of sums, under the address and undefined-behaviour sanitizers, with NaN in the ldz padding; every output is compared
    with oracle/hopper.py.  Errors are relative to each array's max |entry|, the Hessian share's per step block.  Measured here
    over the six cases: 3.0e-15 at worst (the Hessian share at S = 6, M = 65, K = 3; h 1.4e-15, Zmax 1.8e-15, the other
    arrays below 7e-16); HOST_TOL is 100 x that;
  * the facade's plumbing on a NumPy stand-in of the device calls (the oracle's own h, dh/dfz and dh/dx in the kernel's layouts):
    the emission maps of ``nlp_layout()`` reproduce the reference's jacrev(g) and g on the risk rows for 'saa' and 'baseline'
    (tests/golden/ref_hopper_nlp.npz), the multipliers' offset is the risk rows' own, and ``precision='f32'`` stays the default;
  * the RATO_EINVAL cases of the new entry points, which return before any device call.
"""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import _hopper_nlp as R
import _hopper_slip64 as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_TOL = 3e-13
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
_WORST = {}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("slip64") / "hopper_slip64_host")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=fast", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "riskaversetrajopt_amd", "csrc"), os.path.join(HERE, "host", "hopper_slip64_host.hip"), "-o", path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return path


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def run_host(exe, tmp_path, S, M, K, pad, phases, fields, Zs, lams, add, want_zmax=True):
    L = T.layout(S, M, phases)
    Cn, ncon = L["C"], L["ncon"]
    r0 = L["risk"] + 1 + M
    ldz = Zs.shape[1] + pad
    Zp = np.full((K, ldz), np.nan)
    Zp[:, :Zs.shape[1]] = Zs
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([S, phases[0], phases[1], M, K, ldz, ncon, r0, lams is not None, want_zmax], dtype=np.int64).tofile(f)
        np.array([T.MU_NOM]).tofile(f)
        Zp.tofile(f)
        for fld in fields:
            np.ascontiguousarray(np.asarray(fld, dtype=np.float64).T).tofile(f)
        if lams is not None:
            np.ascontiguousarray(lams).tofile(f)
            np.ascontiguousarray(add).tofile(f)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "slip64 host ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])
    flat = np.fromfile(fout)
    shapes = [("h", (K, Cn, M)), ("dh_dfz", (K, Cn, M)), ("dh_dx", (K, Cn, 3, M))]
    if want_zmax:
        shapes.append(("Zmax", (K, M)))
    if lams is not None:
        shapes += [("D", (K, Cn, 3)), ("add", (K, S + 1, 78))]
    got, o = {}, 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        got[name] = flat[o:o + n].reshape(shape)
        o += n
    assert o == flat.size
    if lams is not None:
        got.update(T.split_D(got["D"]))
    return got


CASES = [(6, 4, 1, 0, "default"), (6, 65, 3, 5, "default"), (30, 30, 2, 0, "default"), (5, 3, 1, 0, "no first phase"),
         (5, 3, 1, 0, "no second phase"), (5, 3, 1, 0, "no contacts")]


@needs_hipcc
@pytest.mark.parametrize("S,M,K,pad,phase", CASES)
def test_every_lane_on_the_host_equals_the_oracle(exe, tmp_path, S, M, K, pad, phase):
    phases = T.phase_cases(S)[phase]
    fields, Zs, lams, add = T.inputs(S, M, K, phases)
    zero = np.zeros_like(add)
    ref = T.reference(fields, Zs, lams, zero, S, phases)
    got = run_host(exe, tmp_path, S, M, K, pad, phases, fields, Zs, lams, zero)
    Cn = T.layout(S, M, phases)["C"]
    errs = T.errors(got, ref)
    if Cn == 0:
        assert got["h"].size == 0 and not np.any(got["add"]) and np.all(got["Zmax"] == 0.0), "nothing is launched, nothing is written"
    else:
        assert set(errs) == {"h", "dh_dfz", "dh_dx", "Zmax", "D1", "D2", "D0", "hess"}
    for name, e in errs.items():
        _WORST[name] = max(_WORST.get(name, 0.0), e)
    print(phase, {k: float("%.3g" % v) for k, v in errs.items()}, "worst so far", {k: float("%.3g" % v) for k, v in _WORST.items()})
    for name, e in errs.items():
        assert e <= HOST_TOL, (name, e)
    # the outputs do not depend on which of the others are asked for: without lam and without Zmax the rest is bitwise the same
    bare = run_host(exe, tmp_path, S, M, K, pad, phases, fields, Zs, None, None, want_zmax=False)
    for name in ("h", "dh_dfz", "dh_dx"):
        np.testing.assert_array_equal(bare[name], got[name])
    # add is forwarded where no contact sits and added to where one does; row k is what the K = 1 run gives
    fwd = run_host(exe, tmp_path, S, M, K, pad, phases, fields, Zs, lams, add)
    np.testing.assert_array_equal(fwd["D"], got["D"])
    touched = got["add"] != 0.0
    np.testing.assert_array_equal(fwd["add"][~touched], add[~touched])
    np.testing.assert_array_equal(fwd["add"][touched], (add + got["add"])[touched])
    if K > 1:
        one = run_host(exe, tmp_path, S, M, 1, pad, phases, fields, Zs[1:2], lams[1:2], zero[1:2])
        for name in one:
            np.testing.assert_array_equal(one[name][0], got[name][1])


# ---- the facade's plumbing on a NumPy stand-in of the device calls ------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_hopper_nlp.npz"))


@pytest.mark.parametrize("pre", ["", "s6_"])
@pytest.mark.parametrize("method", ["saa", "baseline"])
def test_emission_maps_reproduce_the_references_risk_rows(fx, lib, pre, method):
    from riskaversetrajopt_amd import hopper
    S, M = int(fx[pre + "S"]), int(fx[pre + "M"])
    phases = (int(fx[pre + "time_jump"]), int(fx[pre + "time_land"]))
    fields = (fx[pre + "intensities"], fx[pre + "thetas"], fx[pre + "taus"])
    Z, lam = fx[pre + "Z"], fx[pre + "lam"]
    m = hopper.Model.host_only(M, method, T.ALPHA, S=S)
    lay = m.nlp_layout()
    L = T.layout(S, M, phases, method)
    Cn = lay["C"]
    ncon, r0 = m.risk_rows_offset()
    assert (ncon, r0) == (L["ncon"], L["risk"] + (1 + M if method == "saa" else 0)) and ncon == lay["ncon"]
    lams = np.zeros((1, ncon))
    if method == "saa":
        lams[0] = lam
    ref = T.reference(fields, Z[None], lams, np.zeros((1, S + 1, 78)), S, phases, method)
    # the stand-in: what rato_scatter_f64 does with the kernel's arrays
    vals = lay["slip_const"].copy()
    for mp, src in ((lay["map_slip_dx"], ref["dh_dx"][0].reshape(-1)), (lay["map_slip_dfz"], ref["dh_dfz"][0].reshape(-1))):
        assert np.unique(mp).size == mp.size and np.all(lay["slip_const"][mp] == 0.0)
        vals[mp] = src
    rows = np.empty(M * Cn)
    rows[lay["map_slip_h"]] = ref["h"][0].reshape(-1)
    assert np.array_equal(np.sort(lay["map_slip_h"]), np.arange(M * Cn)) and vals.size == lay["nnz_slip"]
    indices, indptr = m._jacobian_pattern(Cn)
    n_risk = lay["n_risk"]
    J_slip = sp.csc_matrix((vals, indices, indptr), shape=(n_risk, m.num_vars)).toarray()
    o = T.oracle(fields, S, phases, method)
    np.testing.assert_array_equal(J_slip, o.slip_jacobian(Z).toarray())
    g_risk = m._risk_rows(Z, rows)
    np.testing.assert_array_equal(g_risk, o.slip_risk_constraints(Z))
    # in the whole Jacobian through pos_slip, against the reference's own numbers
    risk = slice(lay["off"]["risk"], lay["off"]["control"])
    if method == "saa":
        data = np.zeros(lay["jac_indices"].size)
        data[lay["pos_slip"]] = vals
        J = sp.csc_matrix((data, lay["jac_indices"], lay["jac_indptr"]), shape=(ncon, m.num_vars)).toarray()
        Jr = sp.csc_matrix((fx[pre + "J_data"], fx[pre + "J_indices"], fx[pre + "J_indptr"]), shape=tuple(fx[pre + "J_shape"])).toarray()
        assert R.rel_err(J[risk], Jr[risk]) <= 7e-14 and not np.any(J[:risk.start]) and not np.any(J[risk.stop:])
    assert R.rel_err(g_risk, fx[pre + "g_" + method][risk]) <= 7e-14
    # the Hessian share as a matrix: the blocks the kernel adds, placed by _blocks_to_csc, are the oracle's slip_hessian
    lam_s = lams[0][r0:r0 + M * Cn].reshape(M, Cn)
    H = m._blocks_to_csc(ref["add"][0]).toarray()
    np.testing.assert_array_equal(H, o.slip_hessian(Z, lam_s).toarray())


def test_precision_defaults_to_f32(lib):
    from riskaversetrajopt_amd import hopper
    assert inspect.signature(hopper.Model.__init__).parameters["precision"].default == "f32"
    assert inspect.signature(hopper.Model.from_device).parameters["precision"].default == "f32"
    assert hopper.Model.host_only(3, S=5).precision == "f32"
    with pytest.raises(ValueError):
        hopper.Model(3, S=5, fields="device", device="cpu", precision="f16")
    for phases, Cn in (((0, 5), 0), ((1, 3), 3), ((5, 5), 5)):
        lay = hopper.Model.host_only(3, S=5, phases=phases).nlp_layout()
        assert lay["C"] == Cn and lay["nnz_slip"] == lay["pos_slip"].size == (8 * Cn * 3 + 2 * 3 + 1 if Cn else 0)


def test_invalid_arguments_are_refused_without_a_launch(lib):
    """every case returns before the first device call: the pointers below are never dereferenced"""
    from riskaversetrajopt_amd import hopper
    EINVAL, OK = -1, 0
    P = C.c_void_p(4096)
    S, M = 6, 4
    nvar = 8 * (S + 1) + 4 * S
    good = hopper.nlp_params(S)
    Cn = good.time_jump + S - good.time_land

    def slip(p=good, K=1, M=M, Z=P, ldz=nvar, a=P, lam=None, ldlam=0, r0=0, part=None, D=None):
        return lib.rato_hopper_slip_f64(C.byref(p), 0.1, K, M, Z, ldz, a, P, P, lam, ldlam, r0, P, P, P, P, part, D, None)

    def hess(p=good, K=1, Z=P, ldz=nvar, D=P, add=P):
        return lib.rato_hopper_slip_hess_blocks_f64(C.byref(p), K, Z, ldz, D, add, None)
    for call in (slip, hess):
        assert call(p=hopper.nlp_params(0, 0, 0, dt=1.0)) == EINVAL
        assert call(K=0) == EINVAL and call(K=65536) == EINVAL
        assert call(ldz=nvar - 1) == EINVAL and call(Z=None) == EINVAL
        for tj, tl in ((-1, 3), (4, 3), (2, S + 1)):
            assert call(p=hopper.nlp_params(S, tj, tl)) == EINVAL
        assert call(p=hopper.nlp_params(S, 0, S)) == OK, "no contact step: valid, nothing is launched"
    assert slip(M=0) == EINVAL and slip(a=None) == EINVAL
    assert slip(lam=P, ldlam=M * Cn + 5, r0=5, part=None, D=P) == EINVAL and slip(lam=P, ldlam=M * Cn + 5, r0=5, part=P, D=None) == EINVAL
    assert slip(lam=P, ldlam=M * Cn + 4, r0=5, part=P, D=P) == EINVAL and slip(lam=P, ldlam=M * Cn, r0=-1, part=P, D=P) == EINVAL
    assert hess(D=None) == EINVAL and hess(add=None) == EINVAL
    assert [lib.rato_hopper_slip_f64_nblocks(M) for M in (0, 1, 30, 256, 257, 50000)] == [0, 1, 1, 1, 2, 196]

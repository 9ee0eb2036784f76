"""GPU: the hopper slip kernel's launch shapes.  hopper_nw_log2 takes 4 contact-waves per sample-wave (64 samples per
workgroup) while ceil(M / 64) < 1536 and 2 (two sample-waves, 128 samples) from there on; RATO_HOPPER_NW_LOG2=0 (one
contact-wave, four sample-waves, 256 samples) is the A/B knob.  Both sides of the edge against the fp64 oracle, the
three shapes against each other bit for bit, the per-workgroup Hessian partials through tests/_hopper_check.py, and
the largest contact counts the dynamic-LDS path accepts.

The oracle is evaluated on the inputs the device actually receives (fields, px, fx, fz and lambda rounded to fp32):
the differences left are the kernel's own arithmetic."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _hopper_check as hc
from tests import _tol as tol
from tests.test_gpu_hopper import H_ATOL, MU_ATOL, hessian_partials3, synthetic_Z

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, M_MAX = 60, 200003
_CACHE = {}


def inputs():
    """The construction of test_gpu_hopper._models / synthetic_Z at S = 60 (40 contacts), fields drawn once for M_MAX
    samples and cut to M for smaller batches (the contact inputs do not depend on M); lambda [C][M_MAX] fp32 on
    [0.5, 1) so that no term of a partial is near zero."""
    if "inputs" not in _CACHE:
        from oracle import hopper as oh
        fields = oh.sample_friction_fields(np.random.RandomState(1), M_MAX)
        o = oh.Model(*(f[:30] for f in fields), method='saa', alpha=0.2, S=S)
        px, forces = o.contact_inputs(synthetic_Z(o))
        lam = np.random.RandomState(4).uniform(0.5, 1.0, (px.shape[0], M_MAX)).astype(np.float32)
        _CACHE["inputs"] = fields, px, forces, lam
    return _CACHE["inputs"]


def model(M):
    from riskaversetrajopt_amd import hopper
    fields, px, forces, lam = inputs()
    d = hopper.Model(M, 'saa', 0.2, S=S, fields=tuple(f[:M] for f in fields))
    return d, px, forces, np.ascontiguousarray(lam[:, :M])


def terms(M):
    """the checker's fp64 per-sample terms for the first M samples (one oracle pass over M_MAX, cut)"""
    if "terms" not in _CACHE:
        fields, px, forces, lam = inputs()
        f32 = lambda v: np.asarray(v, dtype=np.float32)
        _CACHE["terms"] = hc.SampleTerms(lam, f32(px), f32(forces[:, 0]), f32(forces[:, 1]),
                                         tuple(f32(f) for f in fields))
    return _CACHE["terms"].head(M)


def run_shape(d, px, forces, lam):
    """-> the per-sample outputs and both partial layouts of one batch (numpy), as the library's callers launch it"""
    import torch
    from riskaversetrajopt_amd import _lib, stats
    lamd = torch.as_tensor(lam, device="cuda")
    r = d.slip_device(px, forces, lam=lamd, want_Z=True, want_h=True, want_deriv=True, reduce=False)
    p3 = hessian_partials3(d, px, forces, lamd)
    out = {k: r[k].cpu().numpy() for k in ("Z", "h", "dh_dfz", "dh_dpx")}
    out["part2"], out["part3"] = r["part"].cpu().numpy(), p3.cpu().numpy()
    out["sums2"], out["sums3"] = stats.sum_partials(r["part"]).cpu().numpy(), stats.sum_partials(p3).cpu().numpy()
    out["nblocks"] = np.int64(_lib.load().rato_hopper_nblocks(lam.shape[1]))
    return out


def check_partials(out, T, blocks, what):
    """both partial layouts through the checker; the library's second stage (sum_partials) is the fp64 sum of them"""
    worst = {}
    for key, sums in (("part2", "sums2"), ("part3", "sums3")):
        p = out[key]
        w = hc.check_partials(p, T, blocks, what=f"{what} {key}")
        worst.update({f"{key} {k}": v for k, v in w.items()})
        exact = p.astype(np.float64).sum(axis=0)
        assert np.all(np.abs(out[sums] - exact) <= 1e-12 * np.abs(p.astype(np.float64)).sum(axis=0)), (what, key)
    return worst


@pytest.mark.parametrize("M,nblocks", [(98239, 1535), (98240, 1535), (98241, 768), (196672, 1537), (200003, 1563)])
def test_both_sides_of_the_shape_edge(M, nblocks):
    """98,239: one sample-wave per workgroup, the last one ragged; 98,240: the last M with 64 samples per workgroup;
    98,241: two sample-waves, the last workgroup's second one holds ONE valid lane; 196,672: the last workgroup's second
    sample-wave is clamped entirely; 200,003: ragged second sample-wave."""
    from oracle import stats as ostats
    from riskaversetrajopt_amd import _lib
    assert _lib.load().rato_hopper_nblocks(M) == nblocks
    blocks = hc.block_of(M, nblocks)
    d, px, forces, lam = model(M)
    out = run_shape(d, px, forces, lam)
    T = terms(M)
    h_o = T.h()
    Z_o = h_o.max(axis=0)
    # every sample and every contact, the last workgroups included (rows [C][M])
    np.testing.assert_allclose(out["Z"], Z_o, rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(out["h"], h_o, rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(out["dh_dfz"], T.dh_dfz(), rtol=0, atol=MU_ATOL)
    np.testing.assert_allclose(out["dh_dpx"], T.dh_dpx(), rtol=1e-5, atol=2e-5)
    tail = slice(min(M - 130, blocks.lo[-2]), M)
    assert np.abs(out["h"][:, tail] - h_o[:, tail]).max() <= H_ATOL and np.all(np.isfinite(out["Z"][tail]))
    st = d.monte_carlo_statistics(px, forces, alpha=0.1)
    assert abs(st["var"] - ostats.monte_carlo_var(Z_o, 0.1)) < 5e-5
    assert abs(st["cvar"] - ostats.monte_carlo_avar(Z_o, 0.1)) < 5e-5
    eps = T.trig_eps(out["dh_dfz"])
    tol.report(f"M={M} trig path: max |mu - mu_ref| / sum |a|", eps, hc.EPS_TRIG)
    assert eps < hc.EPS_TRIG
    T.set_device_dh_dpx(out["dh_dpx"])
    worst = check_partials(out, T, blocks, f"M={M}")
    for k, v in worst.items():
        tol.report(f"M={M} {k} per-workgroup |err| / checker limit", v, 1.0)


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
from tests import test_gpu_hopper_shapes as T
out = {}
for M in %(Ms)r:
    r = T.run_shape(*T.model(M))
    out.update({"%%s_%%d" %% (k, M): v for k, v in r.items()})
np.savez(%(path)r, **out)
'''


def test_launch_shapes_compute_the_same_values(tmp_path):
    """RATO_HOPPER_NW_LOG2 = 0, 1, 2 (read once per process: one child each) at M = 50,000 and 98,241: every
    (sample, contact) value is computed by one lane with the same instructions and Z's fmaxf fold is order-free, so Z,
    h, dh/dfz and dh/dpx are bit for bit the same; each shape's partials pass the checker with its own workgroups."""
    Ms = (50000, 98241)
    res = {}
    for nw in (0, 1, 2):
        path = str(tmp_path / ("nw%d.npz" % nw))
        env = dict(os.environ, RATO_HOPPER_NW_LOG2=str(nw))
        p = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, Ms=Ms, path=path)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        res[nw] = np.load(path)
    for M in Ms:
        base = res[2]
        for nw in (0, 1):
            for k in ("Z", "h", "dh_dfz", "dh_dpx"):
                a, b = base["%s_%d" % (k, M)], res[nw]["%s_%d" % (k, M)]
                assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (M, nw, k)
        T = terms(M)
        T.set_device_dh_dpx(base["dh_dpx_%d" % M])
        for nw in (0, 1, 2):
            out = {k: res[nw]["%s_%d" % (k, M)] for k in ("part2", "part3", "sums2", "sums3", "nblocks")}
            blocks = hc.block_of(M, int(out["nblocks"]), nw_log2=nw)
            assert out["part2"].shape[0] == blocks.nblocks == out["part3"].shape[0]
            check_partials(out, T, blocks, f"M={M} nw_log2={nw}")


@pytest.mark.parametrize("nslots,C_max", [(2, 20352), (3, 13568)])
def test_dynamic_lds_edge(nslots, C_max):
    """(256 + SW C HC) floats of LDS, at most 160 KiB: at M = 300 (SW = 1) the largest accepted contact count is 20,352
    with the (D1, D2) partials and 13,568 with (D1, D2, D0).  Without partials the kernel needs 1 KiB, so they are
    requested.  One more contact is refused (RATO_EINVAL) before anything is written; every buffer is sized for the
    larger count, so that a wrong acceptance would still stay in bounds."""
    import torch
    from riskaversetrajopt_amd import _lib, hopper
    from oracle import hopper as oh
    lib = _lib.load()
    M = 300
    fields = oh.sample_friction_fields(np.random.RandomState(1), M)
    d = hopper.Model(M, 'saa', 0.2, S=S, fields=fields)
    rng = np.random.RandomState(6)
    Cb = C_max + 1
    px = np.linspace(-3.0, 3.0, Cb).astype(np.float32)
    fz = (32.0 + rng.randn(Cb)).astype(np.float32)
    fx = (0.08 * fz + 0.3 * rng.randn(Cb)).astype(np.float32)
    lam = rng.uniform(0.5, 1.0, (Cb, M)).astype(np.float32)
    dev = lambda v: torch.as_tensor(v, device="cuda")
    pxd, fxd, fzd, lamd = dev(px), dev(fx), dev(fz), dev(lam)
    nb = lib.rato_hopper_nblocks(M)
    blocks = hc.block_of(M, nb)
    assert blocks.spw == 64
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    Z, h, dfz, dpx, part = nan(M), nan(Cb, M), nan(Cb, M), nan(Cb, M), nan(nb * Cb * nslots)
    P = _lib.ptr
    fa = (P(d._a), P(d._th), P(d._tau), P(lamd), P(Z), P(h), P(dfz), P(dpx), P(part))

    def call(C):
        if nslots == 2:
            return lib.rato_hopper_slip(M, C, P(pxd), P(fxd), P(fzd), *fa, _lib.current_stream())
        return lib.rato_hopper_slip_hessian(M, C, P(pxd), P(fxd), P(fzd), 0, *fa, _lib.current_stream())

    assert (256 + C_max * nslots) * 4 == 160 * 1024
    assert call(C_max + 1) == -1                                  # RATO_EINVAL
    torch.cuda.synchronize()
    for t in (Z, h, dfz, dpx, part):
        assert bool(torch.isnan(t).all())
    assert call(C_max) == 0
    torch.cuda.synchronize()
    C = C_max
    hh, dz, dp = (t[:C].cpu().numpy() for t in (h, dfz, dpx))
    assert bool(torch.isnan(h[C:]).all() and torch.isnan(part[nb * C * nslots:]).all())    # nothing past C contacts
    T = hc.SampleTerms(lam[:C], px[:C], fx[:C], fz[:C], tuple(f.astype(np.float32) for f in fields), dh_dpx=dp)
    np.testing.assert_allclose(hh, T.h(), rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(Z.cpu().numpy(), T.h().max(axis=0), rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(dz, T.dh_dfz(), rtol=0, atol=MU_ATOL)
    np.testing.assert_allclose(dp, T.dh_dpx(), rtol=1e-5, atol=2e-5)
    hc.check_partials(part[:nb * C * nslots].view(nb, C, nslots).cpu().numpy(), T, blocks, what=f"C={C}")

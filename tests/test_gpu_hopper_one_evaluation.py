"""GPU: the hopper NLP is evaluated once for everyone who reads it -- ``hopper.Model`` (what the IPOPT callbacks read),
``hopper_ipm.DeviceBackend`` and ``hopper_arrow.ArrowDeviceBackend`` give the same bits for the deterministic rows' Jacobian
values, the step blocks of the Lagrangian's Hessian and g; the multiplier fold of ``nlp_device`` does not depend on ``fold=`` or
on where the multipliers lie; and the arrow backend's evaluation stays O(M C) in memory.

Everything here is an equality of bits between two consumers of the same kernels on the same inputs (K = 3 problems with their
own alphas, the designed iterates of tests/_hopper_nlp.py, multipliers over seven decades with exact zeros among them, the
objective's blocks at sf = 0 and at a non-trivial sf), so no tolerance appears."""
import gc

import numpy as np
import pytest

import _hopper_ipm as H
import _hopper_nlp as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHAS = (0.05, 0.2, 0.6)
SFS = (0.0, 0.37, 0.0)               # the objective's scale per problem: none of it, and a non-trivial one


def up(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes()


def device_model(S, M, method, phases, alpha, flds):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, alpha, S=S, fields=flds, phases=phases, precision='f64')


@pytest.mark.parametrize("S,M,method,phases", H.map_cases())
def test_one_evaluation_for_every_consumer(S, M, method, phases):
    from riskaversetrajopt_amd import hopper_arrow, hopper_ipm
    K = len(ALPHAS)
    flds = H.fields(M)
    models = [device_model(S, M, method, phases, a, flds) for a in ALPHAS]
    m0, lay = models[0], models[0].nlp_layout()
    ncon, everyone = lay["ncon"], list(range(K))
    rng = np.random.RandomState(900 + S + 10 * M)
    lams = rng.uniform(-2, 2, (K, ncon)) * 10.0 ** rng.randint(-3, 4, (K, ncon))
    lams[:, rng.rand(ncon) < 0.2] = 0.0
    Zs = [R.problem(S, M, k) for k in range(K)]
    Z = np.stack(Zs)
    add = up(np.stack([hopper_ipm._obj_add(m0, sf) for sf in SFS]))
    kept = bits(add)
    backends = [hopper_ipm.DeviceBackend(models)]
    if lay["C"] >= 1:
        backends.append(hopper_arrow.ArrowDeviceBackend(models))

    # (a) the deterministic rows' Jacobian values and the step blocks: the Model's call against what the backends keep
    r = m0.nlp_device(Z, lams, add=add)
    assert bits(add) == kept, "the caller's add is left as it is"
    G = {}
    for be in backends:
        G[be] = be.eval_full(everyone, Zs, list(lams), list(SFS))
        name = type(be).__name__
        assert bits(be.vals0) == bits(r["jac_values"]), name
        assert bits(be.hessd) == bits(r["hess_blocks"]), name
        assert bits(be.hess_host) == bits(r["hess_blocks"]), name

    # (b) g, row for row: Model.g with each problem's own alpha, eval_g and the g eval_full returns
    g_model = [m.g(Zk) for m, Zk in zip(models, Zs)]
    for be in backends:
        g1 = be.eval_g(everyone, Zs)
        for k in everyone:
            assert g_model[k].shape == (ncon,)
            assert bits(g1[k]) == bits(g_model[k]), (type(be).__name__, "eval_g", k)
            assert bits(G[be][k]) == bits(g_model[k]), (type(be).__name__, "eval_full", k)

    # (c) the fold: 'host' and 'device' give the same blocks wherever the multipliers lie; only 'host' builds hess_tril
    assert "hess_tril" in r
    host_dev = m0.nlp_device(up(Z), up(lams), add=add, fold='host')
    dev_dev = m0.nlp_device(up(Z), up(lams), add=add, fold='device')
    assert bits(host_dev["hess_blocks"]) == bits(r["hess_blocks"]) and bits(host_dev["hess_tril"]) == bits(r["hess_tril"])
    assert bits(dev_dev["hess_blocks"]) == bits(r["hess_blocks"])
    assert "hess_tril" not in dev_dev
    assert bits(add) == kept


def test_arrow_evaluation_stays_linear_in_M():
    """S = 2, M = 20 000: one tril template of hess_tril would be n (n + 1) / 2 doubles = 1.6 GB at n = 20 034; the friction
    fields, the partials and the maps the arrow path needs are a few tens of MB.  256 MB has room on both sides."""
    import torch
    from riskaversetrajopt_amd import hopper_arrow
    S, M = 2, 20000
    model = device_model(S, M, 'saa', None, 0.2, H.fields(M))
    be = hopper_arrow.ArrowDeviceBackend([model])
    ncon = model.nlp_layout()["ncon"]
    Z = R.problem(S, M, 0)
    lam = np.random.RandomState(7).uniform(-1, 1, ncon)
    Zt, Yt = up(Z[None]), up(lam[None])
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    g = be.eval_full([0], [Z], [lam], [1.0])[0]
    g1 = be.eval_g([0], [Z])[0]
    gt = be.eval_full_t(Zt, Yt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("peak device memory of the arrow evaluation at M = %d: %.1f MB" % (M, peak / 2.0 ** 20))
    assert peak < 256 * 2 ** 20, peak
    assert g.shape == g1.shape == (ncon,) and tuple(gt.shape) == (1, ncon) and bits(g) == bits(g1)

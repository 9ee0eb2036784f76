"""CPU: what the arrowhead Newton step under ``driver='device'`` rests on and a host can check -- the inverse maps
of ``hopper_arrow.arrow_structure`` that rato_scatter_f64 gathers with, the argument checks of the ``arrow_*`` bindings, and
the entry point's refusal of models it cannot serve."""
import numpy as np
import pytest

import _hopper_ipm as H


def model_of(S, M, method, phases=None, alpha=0.2, **kw):
    from riskaversetrajopt_amd import hopper
    return hopper.Model.host_only(M, method=method, alpha=alpha, S=S, phases=phases, **kw)


def scatter(src, index_map, n_dst):
    """rato_scatter_f64 on a zeroed destination: dst[k][map[i]] = src[k][i]; an entry outside [0, n_dst) is not emitted"""
    dst = np.zeros((src.shape[0], n_dst))
    for i, t in enumerate(index_map):
        if 0 <= t < n_dst:
            dst[:, t] = src[:, i]
    return dst


CASES = H.map_cases() + [(6, 65, 'saa', None), (6, 65, 'baseline', None)]       # (2, (0, 2)) and (6, (0, 6)): no contact step


@pytest.mark.parametrize("S,M,method,phases", CASES)
def test_inverse_maps_reproduce_the_gathers(S, M, method, phases):
    from riskaversetrajopt_amd import hopper_arrow
    m = model_of(S, M, method, phases)
    if m.nlp_layout()["C"] < 1:
        with pytest.raises(ValueError, match="newton='arrow'"):
            hopper_arrow.arrow_structure(m)
        return
    st = hopper_arrow.arrow_structure(m)
    n, nc, q = st["n"], st["nc"], st["q"]
    assert st["inv_qz"].shape == st["inv_core_z"].shape == (n,) and st["inv_qcol"].shape == (nc,)
    assert all(st[k].dtype == np.int64 for k in ("inv_qz", "inv_core_z", "inv_qcol"))
    rng = np.random.RandomState(S + 10 * M)
    x = rng.uniform(-2, 2, (3, n)) * 10.0 ** rng.randint(-3, 4, (3, n))
    xc = rng.uniform(-2, 2, (3, nc)) * 10.0 ** rng.randint(-3, 4, (3, nc))
    assert scatter(x, st["inv_qz"], q).tobytes() == np.ascontiguousarray(x[:, st["qz"]]).tobytes()
    assert scatter(x, st["inv_core_z"], nc).tobytes() == np.ascontiguousarray(x[:, st["core_z"]]).tobytes()
    assert scatter(xc, st["inv_qcol"], q).tobytes() == np.ascontiguousarray(xc[:, st["qcol"]]).tobytes()
    # every target has exactly one source, so a gather needs no zeroed destination; the y block has none in either map
    for inv, size in ((st["inv_qz"], q), (st["inv_core_z"], nc), (st["inv_qcol"], q)):
        assert np.array_equal(np.sort(inv[inv >= 0]), np.arange(size)) and np.all(inv >= -1)
    assert np.all(st["inv_core_z"][st["y0"]:st["y0"] + M] == -1) and np.all(st["inv_qz"][st["y0"]:st["y0"] + M] == -1)
    # the scatter back: out[core_z] = xc leaves the y block alone
    back = scatter(xc, st["core_z"], n)
    assert back[:, st["core_z"]].tobytes() == xc.tobytes() and not np.any(back[:, st["y0"]:st["y0"] + M])


def test_binding_argument_errors():
    """the bindings refuse what is not a device fp64 tensor of the stated shape before the library is called"""
    import torch
    from riskaversetrajopt_amd import hopper_ipm as m
    K, M, Cn, n, nc = 2, 4, 2, 40, 30
    f = lambda *s: torch.zeros(s, dtype=torch.float64)
    i32, i64 = lambda k: torch.zeros(k, dtype=torch.int32), lambda k: torch.zeros(k, dtype=torch.int64)
    with pytest.raises(ValueError, match="src"):
        m.scatter_rows(f(K, n), n, i64(n), f(K, nc), nc)
    with pytest.raises(ValueError, match="a must be"):
        m.arrow_scale(f(K), f(K, n), n - 1, None, f(K, n), 3)
    with pytest.raises(ValueError, match="out must be"):
        m.arrow_tfix(M, Cn, True, n, i32(5 * Cn), f(K, 5 * Cn + 1), f(K), f(K, 50), 7, f(K, M), f(K, n))
    with pytest.raises(ValueError, match="malpha"):
        m.arrow_kkbeta(Cn, f(K, 50), 7, f(K, 200), f(K), f(K), f(K))
    with pytest.raises(ValueError, match="e must be"):
        m.arrow_einv(f(K, M), f(K, M), None, None, f(K, M))
    with pytest.raises(ValueError, match="beta"):
        m.arrow_rhsfix(Cn, nc, i32(5 * Cn + 2), f(K, 5 * Cn + 1), f(K), f(K, nc))


def test_entry_point_refuses_what_it_cannot_serve():
    from riskaversetrajopt_amd import hopper_ipm, scp
    m = model_of(2, 4, 'saa')                                        # host only, fp32
    for call in (lambda: hopper_ipm.solve_batch([m], driver='device', newton='arrow'),
                 lambda: m.solve(driver='device', newton='arrow'),
                 lambda: scp.run_hopper(m, driver='device', newton='arrow')):
        with pytest.raises(ValueError, match="newton='arrow'"):
            call()
    with pytest.raises(ValueError, match="backend='device'"):
        hopper_ipm.solve_batch([m], driver='device', backend='numpy', newton='arrow')
    with pytest.raises(ValueError, match="newton must be"):
        hopper_ipm.solve_batch([m], driver='device', newton='x')
    with pytest.raises(ValueError, match="one .num_vars,. vector per model"):
        hopper_ipm.solve_batch([m], [np.zeros(3)], newton='arrow')

"""CPU: the hopper SAA grid over resampled friction fields -- the draw order of ``scp.hopper_saa_experiment``, the grouping of
``hopper_ipm.solve_batch`` (problems with their own fields are ONE lockstep group; backend='numpy' on the restatement's
callbacks, tests/_hopper_ipm.py) and the argument checks that precede any device call (``fields=`` of the facade, ``ldf`` of
rato_hopper_slip_f64_fields)."""
import ctypes as C

import numpy as np
import pytest

import _hopper_ipm as H


# ---- draw order ---------------------------------------------------------------------------------------------------------------
def test_draw_order_of_the_experiment():
    from riskaversetrajopt_amd import hopper, scp
    M, M_mc, R = 30, 50, 3
    draws, mc = scp.draw_hopper_saa_fields(R, M, M_mc, seed=1)
    assert len(draws) == R and all(f.shape == (M, 30) and f.dtype == np.float64 for d in draws for f in d)
    assert all(f.shape == (M_mc, 30) for f in mc)
    # repeat 0 is hopper_experiment's draw (RandomState(seed), one sample_friction_fields)
    first = hopper.sample_friction_fields(M, np.random.RandomState(1))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(draws[0], first))
    # one stream: the repeats in sequence, the validation fields last
    rng = np.random.RandomState(1)
    for d in draws:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d, hopper.sample_friction_fields(M, rng)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(mc, hopper.sample_friction_fields(M_mc, rng)))
    for r in range(R):
        for q in range(r):
            assert all(not np.array_equal(a, b) for a, b in zip(draws[r], draws[q])), (r, q)
    # a longer study keeps the repeats it shares with a shorter one, and moves the validation draw behind the new repeats
    more, mc_more = scp.draw_hopper_saa_fields(R + 1, M, M_mc, seed=1)
    assert all(a.tobytes() == b.tobytes() for d, e in zip(draws, more) for a, b in zip(d, e))
    assert not np.array_equal(mc[0], mc_more[0])
    assert not np.array_equal(scp.draw_hopper_saa_fields(1, M, M_mc, seed=2)[0][0][0], draws[0][0])


# ---- grouping -----------------------------------------------------------------------------------------------------------------
def bitwise(r0, r1):
    (Z0, i0), (Z1, i1) = r0, r1
    keys = ("y", "zl", "zu", "s")
    return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(i0[k].tobytes() == i1[k].tobytes() for k in keys) and \
        all(i0[k] == i1[k] for k in i0 if k not in keys)


def test_a_grid_of_alphas_and_field_sets_is_one_group_and_bitwise_the_solo_runs(monkeypatch):
    """2 alphas x 2 field sets at (S, M) = (6, 4) from the baseline's solution: ``ipm.solve_groups`` receives ONE group of the four
    problems, and every (Z, info) is bitwise the problem's own K = 1 ``solve_batch``"""
    from riskaversetrajopt_amd import hopper_ipm, ipm
    sets = [H.fields(H.M_SMALL, seed) for seed in (1, 2)]
    assert not np.array_equal(sets[0][0], sets[1][0])
    base = H.host_model('baseline', 0.1)
    zero = sets[0]                                                 # the restatement zeroes a baseline's fields itself
    (Zb, _), = hopper_ipm.solve_batch([base], backend='numpy', callbacks=[H.RestatementCallbacks(base, zero)], tol=H.TOL)
    models = [H.host_model('saa', a) for a in (0.1, 0.3) for _ in sets]
    cbs = [H.RestatementCallbacks(m, sets[k % 2]) for k, m in enumerate(models)]
    Z0s = [H.warm_start(m, Zb) for m in models]
    seen = []
    inner = ipm.solve_groups

    def spy(groups, *args, **kw):
        seen.append([list(g) for g in groups])
        return inner(groups, *args, **kw)
    monkeypatch.setattr(ipm, "solve_groups", spy)
    batch = hopper_ipm.solve_batch(models, Z0s, backend='numpy', callbacks=cbs, tol=H.TOL)
    assert seen == [[[0, 1, 2, 3]]], seen
    solos = [hopper_ipm.solve_batch([m], [Z0], backend='numpy', callbacks=[cb], tol=H.TOL)[0] for m, Z0, cb in zip(models, Z0s, cbs)]
    assert seen[1:] == [[[0]]] * 4
    for k, (got, solo) in enumerate(zip(batch, solos)):
        print(k, got[1]["status"], got[1]["iterations"])
        assert bitwise(got, solo), k
        if got[1]["status"] == "converged":
            H.check_solution(models[k], sets[k % 2], *got)
    # the field sets matter: the two problems of one alpha end at different points
    assert not np.array_equal(batch[0][0], batch[1][0]) and not np.array_equal(batch[2][0], batch[3][0])
    # a baseline and an SAA problem still form two groups (one method per group)
    del seen[:]
    hopper_ipm.solve_batch([base, models[0]], [base.initial_guess(), Z0s[0]], backend='numpy',
                           callbacks=[H.RestatementCallbacks(base, zero), cbs[0]], tol=H.TOL, max_iter=2)
    assert seen == [[[0], [1]]]


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def test_fields_argument_is_checked_before_any_device_call():
    """through a host_only model: every device call on it fails, so a ValueError that names the fields came first"""
    import torch
    from riskaversetrajopt_amd import hopper
    S, M, K = 6, 4, 2
    m = hopper.Model.host_only(M, S=S)
    m.precision = 'f64'
    Zs = np.zeros((K, m.num_vars))
    good = tuple(torch.zeros((K, 30, M), dtype=torch.float64) for _ in range(3))
    bad = {
        "two tensors": good[:2],
        "not a triple": good[0],
        "K": tuple(t[:1] for t in good),
        "M": tuple(torch.zeros((K, 30, M + 1), dtype=torch.float64) for _ in range(3)),
        "features": tuple(torch.zeros((K, 29, M), dtype=torch.float64) for _ in range(3)),
        "2-D": tuple(torch.zeros((30, M), dtype=torch.float64) for _ in range(3)),
        "dtype": (good[0], good[1].float(), good[2]),
        "not contiguous": (good[0], good[1], torch.zeros((K, M, 30), dtype=torch.float64).transpose(1, 2)),
        "host array": (good[0], good[1], np.zeros((K, 30, M))),
        "device": tuple(t.to("meta") for t in good),
    }
    for what, f in bad.items():
        for call in (lambda: m.slip_device_f64(Zs, fields=f), lambda: m._slip_f64(Zs, fields=f), lambda: m.nlp_device(Zs, fields=f)):
            with pytest.raises(ValueError, match="fields"):
                call()
    m32 = hopper.Model.host_only(M, S=S)
    with pytest.raises(ValueError, match="precision='f64'"):
        m32.nlp_device(Zs, fields=good)
    with pytest.raises(ValueError, match="at least one model"):
        hopper.stack_fields_f64([])
    # a well-formed triple passes the check and the call goes on to the device, where a host_only model has none
    with pytest.raises(ValueError, match="Z must be a device"):
        m.slip_device_f64(Zs, fields=good)


def test_bad_ldf_is_refused_without_a_launch():
    """every case returns before the first device call: the pointers below are never dereferenced"""
    from riskaversetrajopt_amd import _build, _lib, hopper
    _build.build()
    lib = _lib.load()
    EINVAL, OK = -1, 0
    P = C.c_void_p(4096)
    S, M = 6, 4
    nvar = 8 * (S + 1) + 4 * S
    good = hopper.nlp_params(S)
    none = hopper.nlp_params(S, 0, S)                              # no contact step: a valid call launches nothing

    def slip(ldf, p=none, K=3, M=M, a=P):
        return lib.rato_hopper_slip_f64_fields(C.byref(p), 0.1, K, M, P, nvar, a, P, P, ldf, None, 0, 0, P, P, P, P, None, None, None)
    for ldf in (-1, 1, 30 * M - 1, -30 * M, -2 ** 40):
        assert slip(ldf) == EINVAL and slip(ldf, p=good) == EINVAL, ldf
    for ldf in (0, 30 * M, 30 * M + 7, 2 ** 40):
        assert slip(ldf) == OK, ldf
    assert slip(30 * 5, M=5) == OK and slip(30 * 5 - 1, M=5) == EINVAL
    # the arguments the shared entry refuses are refused here too
    assert slip(30 * M, K=0) == EINVAL and slip(30 * M, M=0) == EINVAL and slip(30 * M, a=None) == EINVAL

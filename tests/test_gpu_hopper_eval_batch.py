"""GPU: K hopper solutions on one set of validation fields in one call -- rato_hopper_eval_batch (csrc/hopper.hip),
``hopper.Model.eval_batch_device`` / ``contact_inputs_batch``, ``scp.hopper_monte_carlo_report`` and the ``M_mc=`` / ``validate=``
arguments of the two hopper experiments.

The property everywhere is bitwise: row k of Z is the Z that rato_hopper_slip writes for solution k, whatever the launch shape;
the records are those of rato_risk_stats on row k; the batched report and experiment return the arrays of the per-solution
loop.  Accuracy is held against the fp64 oracle at H_ATOL = 2e-5, the bound of tests/test_gpu_hopper.py for h = fx - mu fz
(fz ~ 32, mu ~ 0.1: fp32 rounding of mu fz ~ 4e-7 over 30-term sums); the values are that kernel's, so nothing new enters."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_ATOL = 2e-5                  # tests/test_gpu_hopper.py
EINVAL, OK = -1, 0
Z_SENTINEL, ARG_SENTINEL, IN_SENTINEL = -777.0, -99, 1e30
THR = 1e-6


def fields(M, seed=1):
    """a device model on synthetic fields drawn in HBM"""
    from riskaversetrajopt_amd import hopper
    return hopper.Model.from_device(*hopper.sample_friction_fields_device(M, seed=seed, device=DEV))


def contacts(K, Cn, seed):
    """px in [-3, 3], forces at the hopper's scale (fz ~ 32, fx ~ mu fz) -> float32 (3, K, Cn)"""
    rng = np.random.RandomState(seed)
    px = rng.uniform(-3, 3, (K, Cn))
    fz = 32.0 + rng.randn(K, Cn)
    fx = 0.1 * fz + 0.3 * rng.randn(K, Cn)
    return np.stack([px, fx, fz]).astype(np.float32)


def padded_inputs(host, ldc):
    """(3, K, ldc) on the device, the padding filled with a value that would win every maximum"""
    import torch
    _, K, Cn = host.shape
    t = torch.full((3, K, ldc), IN_SENTINEL, dtype=torch.float32, device=DEV)
    t[:, :, :Cn] = torch.from_numpy(host).to(DEV)
    return t


def raw(d, inp, Cn, ldz=None, want_arg=False, alphas=None, shape=None, M=None, K=None, ldz_arg=None, ws=None):
    """the C entry itself on sentinel-filled outputs -> (status, Z (K, ldz), arg (K, ldz) or None, records (K, N) or None)"""
    import torch
    from riskaversetrajopt_amd import _lib, stats
    lib = _lib.load()
    Mm = d._a.shape[1]
    Kk, ldc = inp.shape[1], inp.shape[2]
    ldz = Mm if ldz is None else ldz
    Z = torch.full((Kk, max(ldz, Mm)), Z_SENTINEL, dtype=torch.float32, device=DEV)
    arg = torch.full((Kk, max(ldz, Mm)), ARG_SENTINEL, dtype=torch.int32, device=DEV) if want_arg else None
    rec = al = None
    if alphas is not None:
        rec = torch.full((Kk, stats.N_STATS), -5.0, dtype=torch.float64, device=DEV)
        ws = stats.new_workspace(Mm, DEV) if ws is None else ws
        if alphas != "missing":
            al = np.asarray(alphas, dtype=np.float64)
    p = _lib.ptr
    args = (Mm if M is None else M, Cn, Kk if K is None else K, p(inp[0]), p(inp[1]), p(inp[2]), ldc, p(d._a), p(d._th), p(d._tau),
            p(Z), ldz if ldz_arg is None else ldz_arg, p(arg), None if al is None else al.ctypes.data_as(C.POINTER(C.c_double)),
            THR, p(ws), 0 if ws is None else ws.numel(), p(rec))
    if shape is None:
        rc = lib.rato_hopper_eval_batch(*args, _lib.current_stream())
    else:
        rc = lib.rato_hopper_eval_batch_shaped(*args, _lib.current_stream(), *shape)
    torch.cuda.synchronize()
    return rc, Z, arg, rec


def solo(d, inp, k, Cn, want_h=False):
    """rato_hopper_slip on the device arrays of solution k -> Z (M,) [, h (Cn, M)]"""
    import torch
    from riskaversetrajopt_amd import _lib
    M = d._a.shape[1]
    Z = torch.full((M,), Z_SENTINEL, dtype=torch.float32, device=DEV)
    h = torch.empty((Cn, M), dtype=torch.float32, device=DEV) if want_h else None
    rows = [inp[j, k, :Cn].contiguous() for j in range(3)]
    p = _lib.ptr
    _lib.check(_lib.load().rato_hopper_slip(M, Cn, *(p(r) for r in rows), p(d._a), p(d._th), p(d._tau), None, p(Z), p(h), None,
                                            None, None, _lib.current_stream()), "rato_hopper_slip")
    torch.cuda.synchronize()
    return (Z, h) if want_h else Z


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 64, 65, 200])
def test_rows_are_bitwise_the_single_calls(M):
    """M = 1: one lane; 64: a full wave; 65: a second wave of one lane; 200: a padded last wave.  C = 1, 2: fewer contacts than
    contact-waves; 129: past the by-value path of the single call.  ldc > C and ldz > M, the padding holding sentinels."""
    import torch
    d = fields(M)
    pad_c, pad_z = 3, 5
    for Cn in (1, 2, 7, 20, 129):
        for K in (1, 2, 7, 11):
            host = contacts(K, Cn, seed=100 * Cn + K)
            inp = padded_inputs(host, Cn + pad_c)
            rc, Z, arg, _ = raw(d, inp, Cn, ldz=M + pad_z, want_arg=True)
            assert rc == OK, (Cn, K)
            assert bool(torch.all(Z[:, M:] == Z_SENTINEL)) and bool(torch.all(arg[:, M:] == ARG_SENTINEL)), (Cn, K, "padding written")
            assert bool(torch.all(inp[:, :, Cn:] == IN_SENTINEL))
            rc, Z0, _, _ = raw(d, inp, Cn, ldz=M + pad_z)                     # the kernel without the index
            assert rc == OK and same(Z0, Z), (Cn, K, "with and without arg")
            for k in range(K):
                assert same(Z[k, :M], solo(d, inp, k, Cn)), (Cn, K, k)
            assert bool(torch.all((arg[:, :M] >= 0) & (arg[:, :M] < Cn)))


@pytest.mark.parametrize("Cn", [7, 1])
def test_every_launch_shape_gives_the_same_bits(Cn):
    """C = 1: the contact-waves behind the first get no contact and fold -inf / -1"""
    M, K = 65, 7
    d = fields(M, seed=2)
    inp = padded_inputs(contacts(K, Cn, seed=11), Cn)
    rc, Z, arg, _ = raw(d, inp, Cn, want_arg=True)
    assert rc == OK
    n = 0
    for nw in (0, 1, 2, -1):
        for kc in (1, 2, 3, K, -1):
            rc, Zs, args_, _ = raw(d, inp, Cn, want_arg=True, shape=(nw, kc))
            assert rc == OK, (nw, kc)
            assert same(Zs, Z) and same(args_, arg), (nw, kc)
            rc, Zn, _, _ = raw(d, inp, Cn, shape=(nw, kc))
            assert rc == OK and same(Zn, Z), (nw, kc, "without arg")
            n += 1
    assert n == 20
    for k in range(K):
        assert same(Z[k], solo(d, inp, k, Cn)), k


def test_accuracy_against_the_fp64_oracle():
    from oracle import hopper as oh
    from riskaversetrajopt_amd import hopper
    S, M, K = 30, 200, 3
    f = oh.sample_friction_fields(np.random.RandomState(1), M)
    o, d = oh.Model(*f, method='saa', alpha=0.2, S=S), hopper.Model(M, 'saa', 0.2, S=S, fields=f)
    rng = np.random.RandomState(7)
    Zs = []
    for k in range(K):
        Z = np.zeros(d.num_vars)
        xs = np.zeros((S + 1, 8))
        xs[:, 0] = np.linspace(0, 0.15 * (k + 1), S + 1)
        xs[:, 1] = 1.0
        xs[:, 2] = 0.2 * np.sin(np.linspace(0, 3 + k, S + 1))
        xs[:, 3] = 0.9 + 0.1 * np.cos(np.linspace(0, 2, S + 1))
        us = np.zeros((S, 4))
        us[:, 3] = 32.0 + rng.randn(S)
        us[:, 2] = 0.08 * us[:, 3] + 0.3 * rng.randn(S)
        Z[:(S + 1) * 8], Z[(S + 1) * 8:(S + 1) * 8 + S * 4] = xs.reshape(-1), us.reshape(-1)
        Zs.append(Z)
    px, forces = d.contact_inputs_batch(Zs)
    assert px.shape == (K, 20)
    Zd, rec = d.eval_batch_device(px, forces, want_stats=False)
    assert rec is None and tuple(Zd.shape) == (K, M)
    got = Zd.double().cpu().numpy()
    for k in range(K):
        po, fo = o.contact_inputs(Zs[k])
        assert np.array_equal(po, px[k]) and np.array_equal(fo, forces[k])
        _, Z_o = o.no_slip_constraints_verification(po, fo)
        err = np.abs(got[k] - np.asarray(Z_o)).max()
        print("solution", k, "max |Z - oracle|", err)
        assert err <= H_ATOL, (k, err)


def test_arg_is_the_first_contact_that_attains_the_maximum():
    import torch
    M, K, Cn = 200, 4, 9
    d = fields(M, seed=3)
    host = contacts(K, Cn, seed=21)
    c1, c2 = 2, 6
    host[1, 1, c1] = host[1, 1].max() + 5.0             # fx of solution 1: contact c1 wins everywhere ...
    host[:, :, c2] = host[:, :, c1]                     # ... and c2 > c1 has identical (px, fx, fz) in every solution: ties
    host[1, 3, :] = np.nan                              # fx of solution 3: every value NaN
    inp = padded_inputs(host, Cn + 2)
    want_Z, want_arg = [], []
    for k in range(K):
        Zk, h = solo(d, inp, k, Cn, want_h=True)
        h = h.cpu().numpy()
        z = Zk.cpu().numpy()
        if k == 3:
            assert np.all(np.isnan(h)) and np.all(z == -np.inf)
            a = np.full(M, -1)
        else:
            assert np.array_equal(h.max(axis=0), z)
            a = np.argmax(h == z[None, :], axis=0)      # the smallest c whose value equals Z
            assert np.array_equal(h[c1], h[c2]) and not np.any(a == c2)
        want_Z.append(z), want_arg.append(a)
    assert np.all(want_arg[1] == c1) and np.any(want_arg[0] == c1) and len(np.unique(want_arg[0])) > 2
    for shape in (None, (0, 1), (0, K), (1, 2), (2, 3), (2, K)):
        rc, Z, arg, _ = raw(d, inp, Cn, want_arg=True, shape=shape)
        assert rc == OK, shape
        for k in range(K):
            assert Z[k].cpu().numpy().tobytes() == want_Z[k].tobytes(), (shape, k)
            assert np.array_equal(arg[k].cpu().numpy(), want_arg[k]), (shape, k)
    assert bool(torch.all(Z[3] == -np.inf)) and bool(torch.all(arg[3] == -1))


@pytest.mark.parametrize("M", [200, 12289])
def test_records_are_bitwise_risk_stats_row_by_row(M):
    """M = 12,289 is one past the one-workgroup selection: the runs of equal alphas go through the cooperative form"""
    import torch
    from riskaversetrajopt_amd import stats
    alphas = (0.05, 0.05, 0.3, 0.3, 0.3, 1.0)
    K, Cn = len(alphas), 7
    d = fields(M, seed=4)
    inp = padded_inputs(contacts(K, Cn, seed=31), Cn)
    rc, Z, _, rec = raw(d, inp, Cn, alphas=alphas)
    assert rc == OK
    ws = stats.new_workspace(M, DEV)
    for k, a in enumerate(alphas):
        one = stats.risk_stats_device(Z[k], a, workspace=ws)
        torch.cuda.synchronize()
        assert same(rec[k], one), (k, a, rec[k].tolist(), one.tolist())
    r = rec.cpu().numpy()
    assert np.all(np.isfinite(r)) and np.all(r[:5, 1] >= r[:5, 0]) and not np.array_equal(r[0], r[1])
    assert r[5, 0] == r[5, 4], "alpha = 1: the reference's index wraps, VaR is the maximum"
    # the facade: alphas as a sequence with None for the baseline's row (alpha = 1), the same records
    host = inp[:, :, :Cn].cpu().numpy()
    Zf, recf = d.eval_batch_device(host[0], np.stack([host[1], host[2]], axis=-1), alphas=list(alphas[:-1]) + [None])
    assert same(Zf, Z) and same(recf, rec)
    Zs_, recs = d.eval_batch_device(host[0], np.stack([host[1], host[2]], axis=-1), alphas=0.3)
    assert same(Zs_, Z) and same(recs[2:5], rec[2:5]) and not same(recs[0], rec[0])


def test_bad_arguments_are_refused_and_nothing_is_written():
    import torch
    M, K, Cn = 65, 6, 7
    d = fields(M, seed=5)
    inp = padded_inputs(contacts(K, Cn, seed=41), Cn)
    good = (0.05, 0.05, 0.3, 0.3, 0.3, 1.0)

    def refused(rc, Z, arg, rec):
        return rc == EINVAL and bool(torch.all(Z == Z_SENTINEL)) and (arg is None or bool(torch.all(arg == ARG_SENTINEL))) and \
            (rec is None or bool(torch.all(rec == -5.0)))
    assert refused(*raw(d, inp, Cn, alphas=(0.05, 0.05, 0.0, 0.3, 0.3, 1.0))), "an alpha of 0 in the middle"
    assert refused(*raw(d, inp, Cn, alphas=(0.05, 0.05, 0.3, 0.3, 0.3, 1.5))) and refused(*raw(d, inp, Cn, alphas=(np.nan,) * K))
    assert refused(*raw(d, inp, Cn, alphas="missing")), "stats_out without alphas"
    assert refused(*raw(d, inp, Cn, ldz=M, ldz_arg=M - 1, want_arg=True)), "ldz < M"
    for shape in ((3, 1), (-2, 1), (0, 0), (0, K + 1), (1, -2)):
        assert refused(*raw(d, inp, Cn, want_arg=True, shape=shape)), shape
    assert refused(*raw(d, inp, Cn, M=0)) and refused(*raw(d, inp, Cn, K=0)) and refused(*raw(d, inp, 0))
    assert refused(*raw(d, inp, Cn + 1)), "ldc < C"
    # the fold of 161 solutions with arg needs 322 KiB of LDS; without a split the same chunk needs none
    big = padded_inputs(contacts(161, 2, seed=42), 2)
    assert refused(*raw(d, big, 2, want_arg=True, shape=(1, 161)))
    rc, Z, arg, _ = raw(d, big, 2, want_arg=True, shape=(0, 161))
    assert rc == OK and not bool(torch.any(Z == Z_SENTINEL))
    rc, Z, arg, rec = raw(d, inp, Cn, want_arg=True, alphas=good)
    assert rc == OK and not bool(torch.any(Z == Z_SENTINEL)) and not bool(torch.any(rec == -5.0))
    with pytest.raises(ValueError, match="alphas"):
        d.eval_batch_device(np.zeros((K, Cn)), np.zeros((K, Cn, 2)), alphas=[0.1, 0.2])
    with pytest.raises(ValueError, match="px must be"):
        d.eval_batch_device(np.zeros((K, Cn)), np.zeros((K, Cn + 1, 2)))


def test_a_captured_call_reads_its_inputs_at_replay():
    import torch
    from riskaversetrajopt_amd import stats
    M, K, Cn = 200, 5, 7
    d = fields(M, seed=6)
    first, second = contacts(K, Cn, seed=51), contacts(K, Cn, seed=52)
    inp = torch.from_numpy(first).to(DEV)
    alphas = [0.1, 0.1, 0.5, 0.5, None]
    bufs = {}
    Z, rec, arg = d.eval_batch_inputs_device(inp, Cn, alphas=alphas, want_arg=True, out=bufs)    # allocates, outside the capture
    torch.cuda.synchronize()
    ref_first = [t.clone() for t in (Z, rec, arg)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Zc, recc, argc = d.eval_batch_inputs_device(inp, Cn, alphas=alphas, want_arg=True, out=bufs)
    assert Zc.data_ptr() == Z.data_ptr() and recc.data_ptr() == rec.data_ptr() and argc.data_ptr() == arg.data_ptr()
    inp.copy_(torch.from_numpy(second).to(DEV))         # in place: the graph holds the pointer, not the values
    Z.fill_(Z_SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (Z, rec, arg)]
    want = d.eval_batch_inputs_device(torch.from_numpy(second).to(DEV), Cn, alphas=alphas, want_arg=True)
    torch.cuda.synchronize()
    for name, a, b, old in zip(("Z", "records", "arg"), got, want, ref_first):
        assert same(a, b), name
    assert not same(got[0], ref_first[0])
    assert stats.N_STATS == rec.shape[1]


# ---- 2. the report and the experiments ----------------------------------------------------------------------------------------
S_EXP, M_EXP, M_MC, CAP = 30, 4, 200, 40
EXP_ALPHAS = (0.1, 0.5)


@functools.lru_cache(maxsize=None)
def experiment():
    """``hopper_experiment`` at S = 30 with two alphas and 200 validation fields (computed once; do not modify).  The iteration
    cap keeps the solves short: no status is required, a problem that has not converged is validated like the others."""
    from riskaversetrajopt_amd import scp
    return scp.hopper_experiment(alphas=EXP_ALPHAS, M=M_EXP, S=S_EXP, seed=1, max_iter=CAP, M_mc=M_MC)


def test_saa_experiment_is_bitwise_the_same_under_both_validations(tmp_path):
    from riskaversetrajopt_amd import scp
    kw = dict(alphas=EXP_ALPHAS, num_repeats=2, M=M_EXP, S=S_EXP, M_mc=M_MC, max_iter=CAP)
    a = scp.hopper_saa_experiment(validate='solo', **kw)
    b = scp.hopper_saa_experiment(validate='batch', results_dir=str(tmp_path), **kw)
    for name in ("status", "jump", "safe_fraction", "var", "avar"):
        assert a[name].shape == (2, 2) and a[name].tobytes() == b[name].tobytes(), name
    assert np.all(np.isfinite(b["var"])) and np.all(b["avar"] >= b["var"]) and np.all((0 <= b["safe_fraction"]) & (b["safe_fraction"] <= 1))
    for i in range(2):
        for r in range(2):
            assert a["results"][i][r][0].tobytes() == b["results"][i][r][0].tobytes()
    rep = scp.load_results(str(tmp_path / scp.HOPPER_SAA_REPORT), len(scp.HOPPER_SAA_REPORT_ARRAYS))
    for name, arr in zip(scp.HOPPER_SAA_REPORT_ARRAYS, rep):
        assert np.array_equal(arr, np.asarray(b[name])), name
    with pytest.raises(ValueError, match="validate"):
        scp.hopper_saa_experiment(validate='both', **kw)


def test_report_is_bitwise_the_per_solution_loop():
    from riskaversetrajopt_amd import hopper, scp
    e = experiment()
    mc = hopper.Model(M_MC, 'saa', S=S_EXP, fields=e["mc_fields"])
    Zs = [r["Z"] for r in e["results"]] + [e["base"]["Z"]]
    alphas = list(EXP_ALPHAS) + [None]
    a = scp.hopper_monte_carlo_report(mc, Zs, alphas, batch=True)
    b = scp.hopper_monte_carlo_report(mc, Zs, alphas, batch=False)
    for name in ("alphas", "jump", "frac_satisfied", "var", "avar", "arg_counts"):
        assert a[name].tobytes() == b[name].tobytes(), (name, a[name], b[name])
        assert a[name].tobytes() == e["monte_carlo"][name].tobytes(), name
    K, Cn = len(Zs), 20
    assert a["arg_counts"].shape == (K, Cn) and a["arg_counts"].dtype == np.int64
    unsafe = np.rint((1.0 - a["frac_satisfied"]) * M_MC).astype(np.int64)
    assert np.array_equal(a["arg_counts"].sum(axis=1), unsafe), "every sample that slips names one contact"
    for k, Z in enumerate(Zs):
        assert a["jump"][k] == mc.convert_z_to_xs_us_mats(Z)[0][-1, 0]
    assert a["wall_s"] > 0 and list(a["alphas"]) == list(EXP_ALPHAS) + [0.0]


def test_experiment_reports_the_alphas_and_then_the_baseline(tmp_path, capsys):
    from riskaversetrajopt_amd import hopper, scp
    e = experiment()
    rep = e["monte_carlo"]
    assert list(rep["alphas"]) == list(EXP_ALPHAS) + [0.0]
    assert np.isnan(rep["avar"][-1]) and np.isnan(rep["var"][-1]) and np.all(np.isfinite(rep["avar"][:-1]))
    assert np.all(np.isfinite(rep["frac_satisfied"])) and rep["jump"][-1] == e["base"]["xs"][-1, 0]
    draws, mc_fields = scp.draw_hopper_saa_fields(1, M_EXP, M_MC, seed=1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(e["mc_fields"], mc_fields))
    # the model's fields are the first draw, as without M_mc: the baseline does not read them, the SAA problems do
    plain = hopper.sample_friction_fields(M_EXP, np.random.RandomState(1))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(draws[0], plain))
    # the file, and the script's lines
    path = scp.save_hopper_monte_carlo_report(str(tmp_path), rep)
    for name, arr in zip(scp.HOPPER_MC_REPORT_ARRAYS, scp.load_results(path, 5)):
        assert arr.tobytes() == rep[name].tobytes(), name
    mc = hopper.Model(M_MC, 'saa', S=S_EXP, fields=mc_fields)
    scp.hopper_monte_carlo_report(mc, [e["base"]["Z"], e["results"][0]["Z"]], [None, EXP_ALPHAS[0]], verbose=True)
    lines = capsys.readouterr().out.splitlines()
    assert sum(l.startswith("Monte-Carlo: alpha =") for l in lines) == 2 and sum(l.startswith("avar =") for l in lines) == 1
    assert sum(l.startswith("jumped distance =") for l in lines) == 2 and sum(l.startswith("B_satisfied_vec =") for l in lines) == 2


def test_the_report_at_its_own_size():
    """M = 10,000 fields, 20 contacts, 120 solutions, synthetic inputs: rows 0, 59 and 119 against the single call"""
    M, Cn, K = 10_000, 20, 120
    d = fields(M, seed=8)
    inp = padded_inputs(contacts(K, Cn, seed=61), Cn)
    nw, kc, gx, gy = d.eval_batch_plan(Cn, K)
    print("plan", nw, kc, gx, gy)
    rc, Z, arg, rec = raw(d, inp, Cn, want_arg=True, alphas=[0.05] * 60 + [0.5] * 60)
    assert rc == OK
    for k in (0, 59, 119):
        assert same(Z[k], solo(d, inp, k, Cn)), k
    r = rec.cpu().numpy()
    assert np.all(np.isfinite(r)) and np.all(r[:, 1] >= r[:, 0])

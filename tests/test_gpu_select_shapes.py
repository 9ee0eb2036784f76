"""GPU: the exact selection (csrc/rato_select.h: rs_small_body<NT>, rs_coop_body<NT>) at the workgroup sizes production
runs it at -- 512 threads at the end of the row-parallel linearize launches, 256 at the end of the tiled eval launches --
on DESIGNED Z: ties, constants, signed zeros, NaNs of both signs, clusters, a candidate list at its cap, alpha = 1 (VaR
wraps to the maximum) and an empty tail, at the sizes where each body changes its shape.  tests/test_gpu_stats.py feeds
such inputs to the 1024-thread launches only, tests/test_gpu_fused_stats.py reaches the other two sizes only with smooth
rollouts.  (a) and (b) go through rato_risk_stats_shaped (the bodies with no producer), (c) through the real launches
(``step_device(fused=True)``, ``mc_step_device(in_launch=True)``) with models whose samples are identical within a group.

Reference everywhere: NumPy on the Z read back from the device -- np.sort for VaR and t*, counts for the integer slots,
oracle.stats in fp64 for CVaR.  The exactly defined slots are compared for equality, the fp64 sums with the tolerances of
tests/test_gpu_stats.py (designed distributions: rtol 1e-11, atol 1e-30)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EXACT = [0, 2, 4, 5, 7, 8, 9, 10]          # var, frac_satisfied, max, count_satisfied, rank, count_above, count_at, t_star
SUMS = [1, 3, 6]                           # cvar, mean, tail_sum (fp64 sums: equal to summation order)
NTS = (256, 512)                           # tiled eval launches / row-parallel linearize launches
RS_SMALL_MAX, COOP_MAX_WG, COOP_KEYS = 12288, 64, 16          # csrc/rato_select.h
THR = 1e-6
DESIGNED = dict(rtol=1e-11, atol=1e-30)    # test_risk_stats_edge_distributions
RS_MAGIC = 0x52A70517


# ---- host references -----------------------------------------------------------------------------------------------------
def _rank(M, alpha):
    return max(M - int(np.floor(alpha * M)) - 1, 0)


def _host_record(Z32, alpha):
    """the record of rato_saa.h (RATO_N_STATS = 11) from NumPy: sort, counts, fp64 sums"""
    from oracle import stats as ostats
    M = Z32.size
    Z = Z32.astype(np.float64)
    k = _rank(M, alpha)
    t = np.sort(Z32)[k]
    rec = np.empty(11)
    rec[0] = ostats.monte_carlo_var(Z, alpha)
    rec[1] = ostats.monte_carlo_avar(Z, alpha)
    rec[2] = np.mean(Z32 <= np.float32(THR))
    rec[3] = Z.mean()
    rec[4] = Z.max()
    rec[5] = np.sum(Z32 <= np.float32(THR))
    rec[6] = np.sum(np.maximum(Z - float(t), 0.0))
    rec[7] = k
    rec[8] = np.sum(Z32 > t)
    rec[9] = np.sum(Z32 == t)
    rec[10] = t
    return rec


def _check_record(got, ref, what):
    assert np.array_equal(got[EXACT], ref[EXACT]), (what, got, ref)
    np.testing.assert_allclose(got[SUMS], ref[SUMS], err_msg=str(what), **DESIGNED)


def _check_alpha_edges(got, Z32, alpha, what):
    M = Z32.size
    if int(np.floor(alpha * M)) == M:              # VaR wraps to the maximum, the minimiser stays the minimum
        assert got[0] == Z32.max() and got[10] == Z32.min() and got[8] + got[9] == M, what
    if int(np.floor(alpha * M)) == 0:              # empty tail
        assert got[1] == got[0] == Z32.max() and got[8] == 0 and got[7] == M - 1, what


def _workspace_words(ws):
    import torch
    return ws.view(torch.int32).cpu().numpy().view(np.uint32)


def _assert_workspace_clean(ws, what=None):
    w = _workspace_words(ws)                       # csrc/rato_select.h: Workspace = hist1..3 | blockpart | tstar nblocks magic ticket | sig[8]
    assert not w[:2048 + 2048 + 1024].any(), what  # the three histograms
    assert w[-10] == RS_MAGIC and w[-9] == 0 and not w[-8:].any(), what     # still tagged; ticket and signal words at zero


# ---- (a) designed distributions through the shaped entry ----------------------------------------------------------------------
DISTRIBUTIONS = ("constant", "ties", "signed_zero", "wide", "tiny", "clustered", "sorted_desc", "two_bins", "one_outlier",
                 "negative_cluster")


@functools.lru_cache(maxsize=None)
def _distribution(name, M):
    """the ten cases of test_risk_stats_edge_distributions, at any M >= 1"""
    Z = {
        "constant": lambda: np.full(M, -1.25, np.float32),
        "ties": lambda: np.repeat(np.float32([-3.0, -1.0, 0.0, 2.5]), (M + 3) // 4)[:M],
        "signed_zero": lambda: np.concatenate([np.full(M // 2, -0.0, np.float32), np.full(M - M // 2, 0.0, np.float32)]),
        "wide": lambda: (np.random.RandomState(1).randn(M) * 1e4).astype(np.float32),
        "tiny": lambda: (np.random.RandomState(2).randn(M) * 1e-30).astype(np.float32),
        "clustered": lambda: (1.0 + 1e-6 * np.random.RandomState(3).rand(M)).astype(np.float32),
        "sorted_desc": lambda: np.linspace(5, -5, M).astype(np.float32),
        "two_bins": lambda: (1.25 + 1e-4 * (np.random.RandomState(5).rand(M) - 0.5)).astype(np.float32),
        "one_outlier": lambda: np.concatenate([np.full(M - 1, 0.5, np.float32), np.float32([1e6])]),
        "negative_cluster": lambda: (-2.0 - 1e-5 * np.random.RandomState(6).rand(M)).astype(np.float32),
    }[name]()
    assert Z.size == M and Z.dtype == np.float32
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=None)
def _distribution_record(name, M, alpha):
    rec = _host_record(_distribution(name, M), alpha)
    rec.setflags(write=False)
    return rec


def _edge_sizes(nt):
    """the edges of each body at nt threads: one workgroup up to 12,288 (its last M), the first cooperative M, 64 workgroups
    of 4 keys per thread and one more (the keys per thread start to grow), the capacity of 16 keys per thread"""
    return (1, nt - 1, nt, nt + 1, RS_SMALL_MAX - 1, RS_SMALL_MAX, RS_SMALL_MAX + 1, COOP_MAX_WG * 4 * nt,
            COOP_MAX_WG * 4 * nt + 1, COOP_MAX_WG * COOP_KEYS * nt)


@pytest.mark.parametrize("nt,M", [(nt, M) for nt in NTS for M in _edge_sizes(nt)])
def test_designed_distributions_at_256_and_512_threads(nt, M):
    import torch
    from riskaversetrajopt_amd import stats
    dev = torch.device("cuda:0")
    ws, ws_ref = stats.new_workspace(M, dev), stats.new_workspace(M, dev)       # one workspace each for all the calls below
    alphas = (0.05, 0.5, 1.0, 0.5 / M)
    got = torch.empty((len(DISTRIBUTIONS), len(alphas), stats.N_STATS), dtype=torch.float64, device=dev)
    base = torch.empty_like(got)
    back = []
    for i, name in enumerate(DISTRIBUTIONS):
        Zd = torch.from_numpy(_distribution(name, M).copy()).to(dev)
        for j, alpha in enumerate(alphas):
            stats.risk_stats_shaped_device(Zd, alpha, nt, workspace=ws, out=got[i, j])
            stats.risk_stats_device(Zd, alpha, workspace=ws_ref, out=base[i, j])     # the 1024-thread launches
        back.append(Zd.cpu().numpy())
    got, base = got.cpu().numpy(), base.cpu().numpy()
    for i, name in enumerate(DISTRIBUTIONS):
        Z = back[i]                                                                   # the Z that was on the device
        assert np.array_equal(Z.view(np.uint32), _distribution(name, M).view(np.uint32))
        for j, alpha in enumerate(alphas):
            what = (name, nt, M, alpha)
            _check_record(got[i, j], _distribution_record(name, M, alpha), what)
            _check_alpha_edges(got[i, j], Z, alpha, what)
            assert np.array_equal(got[i, j][EXACT], base[i, j][EXACT]), (what, got[i, j], base[i, j])
    _assert_workspace_clean(ws, (nt, M))


@pytest.mark.parametrize("nt", NTS + (1024,))
def test_one_more_than_the_capacity_is_refused_and_nothing_is_written(nt):
    import torch
    from riskaversetrajopt_amd import _lib, stats
    lib = _lib.load()
    dev = torch.device("cuda:0")
    M = COOP_MAX_WG * COOP_KEYS * nt + 1
    Z = torch.zeros(M, dtype=torch.float32, device=dev)
    ws = stats.new_workspace(M, dev)
    out = torch.full((stats.N_STATS,), -77.0, dtype=torch.float64, device=dev)

    def call(m, alpha, n, w=ws, o=out, nbytes=ws.numel()):
        return lib.rato_risk_stats_shaped(_lib.ptr(Z), m, alpha, THR, _lib.ptr(w), nbytes, _lib.ptr(o), _lib.current_stream(), n)

    assert call(M, 0.1, nt) == -1                                      # RATO_EINVAL
    for bad_nt in (0, 64, 128, 255, 257, 2048, -256):
        assert call(1000, 0.1, bad_nt) == -1
    assert call(0, 0.1, nt) == -1 and call(1000, 0.0, nt) == -1 and call(1000, 1.5, nt) == -1     # rato_risk_stats' own
    assert call(1000, 0.1, nt, w=None) == -1 and call(1000, 0.1, nt, o=None) == -1 and call(1000, 0.1, nt, nbytes=16) == -1
    with pytest.raises(_lib.RatoError):
        stats.risk_stats_shaped_device(Z, 0.1, nt, workspace=ws, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -77.0).all()
    _assert_workspace_clean(ws)
    assert call(M - 1, 0.1, nt) == 0                                   # the capacity itself runs
    torch.cuda.synchronize()
    assert out[0].item() == 0.0 and out[7].item() == _rank(M - 1, 0.1)


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("M", [10000, 50000])          # one workgroup / cooperating workgroups
def test_signed_zeros_at_the_threshold_at_256_and_512_threads(nt, M):
    """the band of test_signed_zeros_at_the_threshold: +0.0 and -0.0 are one value for the counts and the threshold"""
    import torch
    from riskaversetrajopt_amd import stats
    rng = np.random.RandomState(M)
    Z = rng.randn(M).astype(np.float32)
    k = int(0.1 * M)                                       # alpha M samples strictly above zero, then a band of zeros
    order = np.argsort(-Z)
    Z[order[:k - 5]] = np.abs(Z[order[:k - 5]]) + 1.0
    zeros = order[k - 5:k + 6]
    Z[zeros] = np.where(np.arange(zeros.size) % 2 == 0, 0.0, -0.0).astype(np.float32)
    Z[order[k + 6:]] = -np.abs(Z[order[k + 6:]]) - 1.0
    Zd = torch.from_numpy(Z).cuda()
    st = stats.risk_stats_shaped_device(Zd, 0.1, nt).cpu().numpy()
    base = stats.risk_stats_device(Zd, 0.1).cpu().numpy()
    Zh = Zd.cpu().numpy()
    assert st[0] == 0.0 and st[10] == 0.0
    assert st[8] == float(np.sum(Zh > 0.0)) == k - 5
    assert st[9] == float(np.sum(Zh == 0.0)) == 11
    tail = np.sort(Zh.astype(np.float64))[::-1][:k]
    np.testing.assert_allclose(st[1], tail.mean(), rtol=1e-12, atol=1e-12)
    _check_record(st, _host_record(Zh, 0.1), (nt, M))
    assert np.array_equal(st[EXACT], base[EXACT])


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("M", [3000, 12288])
def test_nans_of_both_signs_at_256_and_512_threads(nt, M):
    """test_selection_with_nans_of_both_signs_and_a_key_range_near_the_full_word at the other two sizes: the key range spans
    almost the whole word, and the selection returns the key of the requested rank in the order of the kernels' key map
    (emulated here).  Rank and VaR only: sums over NaNs mean nothing."""
    import torch
    from riskaversetrajopt_amd import stats
    rng = np.random.RandomState(M)
    Z = (rng.randn(M) * 0.5).astype(np.float32)
    n_nan = max(M // 100, 2)
    bits = Z.view(np.uint32).copy()
    idx = rng.permutation(M)
    bits[idx[:n_nan]] = 0xffc00001                       # -NaN: the smallest keys
    bits[idx[n_nan:2 * n_nan]] = 0x7fc00001              # +NaN: the largest keys
    bits[idx[2 * n_nan]] = 0xff800000                    # -inf
    bits[idx[2 * n_nan + 1]] = 0x7f800000                # +inf
    Zd = torch.from_numpy(bits.view(np.float32)).cuda()
    u = Zd.cpu().numpy().view(np.uint32).copy()
    assert np.array_equal(u, bits)
    order = np.sort(_keys(u))
    for alpha in (0.1, 0.3, 0.004):
        k = _rank(M, alpha)
        want_val = _values(order[k:k + 1])[0]
        st = stats.risk_stats_shaped_device(Zd, alpha, nt).cpu().numpy()
        base = stats.risk_stats_device(Zd, alpha).cpu().numpy()
        assert st[7] == k == base[7]
        if np.isnan(want_val):
            assert np.isnan(st[0]) and np.isnan(base[0])
        else:
            assert st[0] == want_val == base[0], (nt, M, alpha, st[0], want_val)


@pytest.mark.parametrize("nt", NTS)
def test_a_workspace_serves_three_calls_in_a_row(nt):
    """the cooperative form zeroes its histograms and its ticket behind itself: equal records, a clean workspace"""
    import torch
    from riskaversetrajopt_amd import stats
    dev = torch.device("cuda:0")
    for M in (5000, RS_SMALL_MAX + 1, 50000, COOP_MAX_WG * 4 * nt + 1):
        Zh = _distribution("ties", M) + _distribution("clustered", M)
        Zd = torch.from_numpy(Zh).to(dev)
        ws = stats.new_workspace(M, dev)
        recs = []
        for rep in range(3):
            recs.append(stats.risk_stats_shaped_device(Zd, 0.05, nt, workspace=ws).cpu().numpy())
            _assert_workspace_clean(ws, (nt, M, rep))
        assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2]), (nt, M)
        _check_record(recs[0], _host_record(Zd.cpu().numpy(), 0.05), (nt, M))


# ---- (b) the candidate list at its cap -----------------------------------------------------------------------------------
def _keys(bits):
    """csrc/rato_select.h key_of: the order-preserving key of a float's bit pattern (-0.0 takes the key of +0.0)"""
    u = bits.astype(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def _values(keys):
    """value_of: the float of a key"""
    k = keys.astype(np.uint32)
    return np.where(k & 0x80000000, k & 0x7fffffff, ~k).astype(np.uint32).view(np.float32)


def _first_level(bits, k):
    """rs_small_body's first pass: 2048 bins of (key - lo) >> sh over the occupied key range -> (sh, the bin that holds
    ascending rank k, its member count)"""
    key = _keys(bits).astype(np.int64)
    lo, hi = int(key.min()), int(key.max())
    sh = max((hi - lo).bit_length() - 11, 0)
    hist = np.bincount((key - lo) >> sh, minlength=2048)
    assert hist.size == 2048
    b = int(np.searchsorted(np.cumsum(hist), k, side="right"))
    return sh, b, int(hist[b])


@pytest.mark.parametrize("nt", NTS + (1024,))
@pytest.mark.parametrize("c", [255, 256, 257])
def test_candidate_list_at_its_cap(nt, c):
    """A first pass that leaves exactly c members in the chosen bin: c <= RS_CAND_MAX = 256 are ranked pairwise, one thread
    per candidate (at 256 threads: every thread of the workgroup), c = 257 is binned again on single keys."""
    import torch
    from riskaversetrajopt_amd import stats
    B, k = 0x3f800000, 1100
    bits = np.concatenate([B + 1024 * np.arange(2048), B + 1000 * 1024 + np.arange(1, c)]).astype(np.uint32)
    M = bits.size
    assert M == 2047 + c and np.unique(bits).size == M
    np.random.RandomState(c).shuffle(bits)
    assert _first_level(bits, k) == (10, 1000, c)          # the case is what it claims to be
    alpha = (M - k - 0.5) / M
    assert _rank(M, alpha) == k
    Zd = torch.from_numpy(bits.view(np.float32)).cuda()
    Zh = Zd.cpu().numpy()
    assert np.array_equal(Zh.view(np.uint32), bits) and np.isfinite(Zh).all()
    want = np.sort(Zh)[k]
    assert want == np.float32(1.122082233428955)
    st = stats.risk_stats_shaped_device(Zd, alpha, nt).cpu().numpy()
    assert st[7] == k and st[0] == want and st[10] == want, (nt, c, st)
    _check_record(st, _host_record(Zh, alpha), (nt, c))
    base = stats.risk_stats_device(Zd, alpha).cpu().numpy()            # the 1024-thread launch
    assert np.array_equal(base, st) if nt == 1024 else np.array_equal(base[EXACT], st[EXACT]), (nt, c, st, base)


# ---- (c) the producer-wait path on designed Z, through the real launches ------------------------------------------------------
S_STEPS = 3                                # the statistics do not depend on S; the rows kernel needs S >= 2


def drone_group_inputs(M, n_groups, S=S_STEPS):
    """Host arrays of a drone batch in kernel layout (dW [S][3][ld], mass [ld], Qsym [n_obs][3][ld]) whose samples are
    identical inputs within each of n_groups groups: no noise, the obstacles' quadratic forms scaled per group (the
    trajectory does not depend on them, so Z = 1 - q c - tol is strictly decreasing in the scale q), and -- up to four
    groups -- a mass per group."""
    from riskaversetrajopt_amd import drone_params as P
    ld = (M + 3) // 4 * 4
    grp = np.minimum(np.arange(ld) * n_groups // M, n_groups - 1)
    q = (0.75 + 0.5 * grp / n_groups).astype(np.float32)
    mass = np.full(ld, P.mass_nom, np.float32)
    if n_groups <= 4:
        mass += (grp - 1.5).astype(np.float32)
    Qsym = np.zeros((P.n_obs, 3, ld), np.float32)
    for j in range(P.n_obs):
        Qsym[j, 0] = Qsym[j, 2] = np.float32(1.0 / P.obs_radii[j] ** 2) * q
    return np.zeros((S, 3, ld), np.float32), mass, Qsym


def driving_group_inputs(M, n_groups, S=S_STEPS):
    """The same for a driving batch (dW [S][2][M], x0_ped [4][M], w_speed [M], w_rep [M]): the pedestrian starts two to
    three metres to the left of its nominal place, by group -- with three steps the pair is then closest after the first
    one, on the car's side of the pedestrian, and that distance shrinks strictly with the offset -- and, up to four
    groups, the two gains differ by group as well."""
    from riskaversetrajopt_amd import driving_params as P
    grp = np.minimum(np.arange(M) * n_groups // M, n_groups - 1)
    x0 = np.repeat(np.asarray(P.state_init[4:], np.float32)[:, None], M, axis=1)
    x0[0] -= (2.0 + grp / n_groups).astype(np.float32)
    w_speed = np.full(M, P.omega_speed_nom, np.float32)
    w_rep = np.full(M, P.omega_repulsive_nom, np.float32)
    if n_groups <= 4:
        w_speed += (0.01 * grp).astype(np.float32)
        w_rep += (0.005 * grp).astype(np.float32)
    return np.zeros((S, 2, M), np.float32), np.ascontiguousarray(x0), w_speed, w_rep


def group_controls(system, S=S_STEPS):
    return np.full((S, 3), 0.05) if system == "drone" else np.full((S, 2), 0.01)


def _group_model(system, M, n_groups):
    import torch
    from riskaversetrajopt_amd import drone_risk, driving
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a).to(dev)
    if system == "drone":
        dW, mass, Qsym = drone_group_inputs(M, n_groups)
        return drone_risk.Model.from_device(S_STEPS, up(dW), up(mass), up(Qsym), 'saa', 0.1, M=M)
    dW, x0, w_speed, w_rep = driving_group_inputs(M, n_groups)
    return driving.Model.from_device(S_STEPS, up(dW), up(x0), up(w_speed), up(w_rep), 'saa', 0.05)


@pytest.mark.parametrize("M", [1, 300, 12288, 12289, 40000])
@pytest.mark.parametrize("carrier", ["rows", "eval"])
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_statistics_workgroups_of_the_real_launches_on_grouped_samples(system, carrier, M):
    """One group (constant Z: the cooperative form finds all M keys in one bin in all three passes), four groups (ties) and
    M distinct values, at alpha 0.3, 1 and 0.5 / M on ONE workspace: the record the launch leaves against NumPy on its Z,
    against the same body with no producer at the same workgroup size (every slot: same order of sums), the signal words
    back at zero."""
    import torch
    from riskaversetrajopt_amd import stats
    nt = 512 if carrier == "rows" else 256
    us = group_controls(system)
    for n_groups in sorted({1, min(4, M), M}):
        d = _group_model(system, M, n_groups)
        lib = d._lib
        if carrier == "rows":
            assert (lib.rato_drone_stats_in_launch if system == "drone" else lib.rato_car_stats_in_launch)(M, S_STEPS)
        else:
            assert (lib.rato_drone_eval_stats_in_launch if system == "drone" else lib.rato_car_eval_stats_in_launch)(M)
        ws = stats.new_workspace(M, d.device)
        Zh = None
        for alpha in (0.3, 1.0, 0.5 / M):                                   # the second and third step reuse the workspace
            if carrier == "rows":
                r, rec = d.step_device(us, alpha=alpha, workspace=ws, fused=True)
                Z = r["Z"]
            else:
                Z, rec = d.mc_step_device(us, alpha=alpha, workspace=ws, in_launch=True)
            torch.cuda.synchronize()
            what = (system, carrier, M, n_groups, alpha)
            got = rec.cpu().numpy()
            if Zh is None:
                Zh = Z.cpu().numpy().copy()
                assert Zh.size == M and np.isfinite(Zh).all()
                assert np.unique(Zh).size == n_groups, (what, np.unique(Zh).size)     # the design holds on the device
            else:
                assert np.array_equal(Z.cpu().numpy(), Zh), what
            _check_record(got, _host_record(Zh, alpha), what)
            _check_alpha_edges(got, Zh, alpha, what)
            alone = stats.risk_stats_shaped_device(Z.contiguous(), alpha, nt).cpu().numpy()
            assert np.array_equal(got, alone), (what, got, alone)
            base = stats.risk_stats_device(Z, alpha).cpu().numpy()      # the 1024-thread launches
            assert np.array_equal(got[EXACT], base[EXACT]), (what, got, base)
            _assert_workspace_clean(ws, what)

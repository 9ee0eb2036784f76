"""GPU: rato_risk_stats_rows (csrc/stats_rows.hip) -- the records of K rows of Z, every row at its own alpha, in one launch
while a row fits the one-workgroup form (M <= 12,288) and in five launches over (workgroups of a row) x (rows) beyond -- and
what is built on it: ``stats.risk_stats_rows*``, ``eval_batch_device(alphas=...)`` of the drone and driving Models,
``scp.monte_carlo_report_grid``, ``mc='grid'`` of the SAA experiments and ``selection='rows'`` of the hopper.

References.  The one-workgroup form is rato_risk_stats on the row with the row's alpha: all 11 entries, bit for bit.  The pass
form is rato_risk_stats_recover on the row (the same workgroups per row, the same fold): all 11 entries, bit for bit; its
exactly defined entries (VaR, fraction, max, count, rank, #{Z > t}, #{Z == t}, t) are also those of rato_risk_stats and of
NumPy in fp64 (np.sort at the reference's index, counts).  The fp64 sums are held against math.fsum with the bound of ANY
summation order of n terms x_i in fp64, n 2^-53 sum |x_i|: nothing measured enters a tolerance.  CVaR is the closed form
t + (tail / M) / alpha of the record's own tail sum, evaluated in Python with the same three IEEE operations.

Every Z here has ldz = M + 5 with the padding filled with NaN: a read past column M of a row poisons the row's sums."""
import math

import numpy as np
import pytest

from test_gpu_fused_stats import _model, _us
from test_gpu_select_shapes import _distribution, _keys, _values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = [0, 2, 4, 5, 7, 8, 9, 10]          # var, frac_satisfied, max, count_satisfied, rank, count_above, count_at, t_star
N = 11
PAD = 5
THR = 1e-6
U = 2.0 ** -53
RS_SMALL_MAX = 12288
WS_WORDS = (2048 + 2048 + 1024) + 1024 * 6 * 2 + 4 + 8          # csrc/rato_select.h: Workspace, in 32-bit words
RS_MAGIC = 0x52A70517


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _padded(rows):
    """rows (K, M) fp32 host (bit patterns kept) -> device (K, M + PAD), the padding NaN"""
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    K, M = rows.shape
    Z = torch.full((K, M + PAD), float("nan"), dtype=torch.float32, device=DEV)
    Z[:, :M] = torch.from_numpy(rows.view(np.int32)).to(DEV).view(torch.float32)
    assert bool(torch.isnan(Z[:, M:]).all())
    return Z


def _random_rows(K, M, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(K, M) * (1.0 + np.arange(K)[:, None]) - 0.3).astype(np.float32)


def _rows_call(Z, M, alphas, ws=None, out=None):
    from riskaversetrajopt_amd import stats
    return stats.risk_stats_rows_device(Z, alphas, thr=THR, workspace=ws, out=out, M=M).cpu().numpy()


def _single(Z, M, alphas, how):
    """the single-row call ``how`` (stats.risk_stats_device / risk_stats_recover_device) on every row -> (K, 11)"""
    import torch
    from riskaversetrajopt_amd import stats
    K = Z.shape[0]
    ws = stats.new_workspace(M, Z.device)
    out = torch.empty((K, N), dtype=torch.float64, device=Z.device)
    for k in range(K):
        how(Z[k, :M].contiguous(), float(alphas[k]), thr=THR, workspace=ws, out=out[k])
    return out.cpu().numpy()


def _bitwise(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _rank(M, alpha):
    return max(M - int(np.floor(alpha * M)) - 1, 0)


def _different_alphas(K):
    return [(k + 1.0) / (K + 1.0) for k in range(K)]


def _check_against_numpy(rec, z32, alpha, what):
    """the exactly defined entries against NumPy in fp64, the sums against math.fsum within the any-order bound"""
    M = z32.size
    z = z32.astype(np.float64)
    k = _rank(M, alpha)
    srt = np.sort(z32)
    t = float(srt[k])
    wraps = int(np.floor(alpha * M)) == M
    assert rec[0] == (float(srt[-1]) if wraps else t), what          # np.sort(Z)[M - floor(alpha M) - 1], -1 wrapping
    assert rec[10] == t and rec[7] == k, what
    assert rec[2] == np.mean(z32 <= np.float32(THR)) and rec[5] == np.sum(z32 <= np.float32(THR)), what
    assert rec[4] == z.max() and rec[8] == np.sum(z32 > srt[k]) and rec[9] == np.sum(z32 == srt[k]), what
    sumabs = math.fsum(np.abs(z))
    assert abs(rec[3] - math.fsum(z) / M) <= M * U * sumabs / M, (what, "mean")
    terms = (z - t)[z32 > srt[k]]                                    # the kernels' summands: (double)z - (double)t, z > t
    assert abs(rec[6] - math.fsum(terms)) <= min(terms.size * U * math.fsum(np.abs(terms)), M * U * sumabs), (what, "tail sum")
    assert rec[1] == t + (rec[6] / M) / alpha, (what, "CVaR is the closed form of the tail sum")


# ---- 1. the one-workgroup form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 130])
@pytest.mark.parametrize("M", [1, 63, 12288])
def test_one_workgroup_form_is_bitwise_risk_stats_row_by_row(M, K):
    from riskaversetrajopt_amd import stats
    host = _random_rows(K, M, seed=M + K)
    Z = _padded(host)
    alphas = _different_alphas(K)
    got = _rows_call(Z, M, alphas)
    want = _single(Z, M, alphas, stats.risk_stats_device)
    assert np.isfinite(got).all(), "a read past column M would have met the NaN padding"
    assert _bitwise(got, want), (M, K, np.argwhere(got != want))
    for k in sorted({0, K // 2, K - 1}):
        _check_against_numpy(got[k], host[k], alphas[k], (M, K, k))


# ---- 2. the pass form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(12289, 1), (12289, 3), (262144, 1), (262144, 3), (262145, 1), (262145, 3), (4194305, 2)])
def test_pass_form_is_bitwise_the_launch_per_pass_single_row_call(M, K):
    """12,289: the first M of the form (13 workgroups per row); 262,144 / 262,145: the last M at 4 elements per thread and the
    first at 16 (256 workgroups both); 4,194,305: the first M whose rows run on the 1024-workgroup cap"""
    from riskaversetrajopt_amd import stats
    host = _random_rows(K, M, seed=M + K)
    Z = _padded(host)
    alphas = [0.05, 0.37, 0.8][:K] if K > 1 else [0.1]
    got = _rows_call(Z, M, alphas)
    assert np.isfinite(got).all(), "a read past column M would have met the NaN padding"
    recover = _single(Z, M, alphas, stats.risk_stats_recover_device)
    assert _bitwise(got, recover), (M, K, got, recover)
    base = _single(Z, M, alphas, stats.risk_stats_device)
    assert _bitwise(got[:, EXACT], base[:, EXACT]), (M, K, got, base)
    for k in range(K):
        _check_against_numpy(got[k], host[k], alphas[k], (M, K, k))


# ---- 3. designed rows in one batch ----------------------------------------------------------------------------------------------
def _designed_rows(M):
    """constant | a tie that straddles the rank | +0 and -0 | +inf and -inf | NaNs of both signs (the key range spans almost the
    whole word: test_gpu_select_shapes) -> (rows (5, M) fp32, alphas)"""
    rng = np.random.RandomState(M)
    inf = (rng.randn(M) * 0.5).astype(np.float32)
    inf[rng.permutation(M)[:6]] = np.float32([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf])
    bits = (rng.randn(M) * 0.5).astype(np.float32).view(np.uint32).copy()
    idx, n_nan = rng.permutation(M), max(M // 100, 2)
    bits[idx[:n_nan]] = 0xffc00001                       # -NaN: the smallest keys
    bits[idx[n_nan:2 * n_nan]] = 0x7fc00001              # +NaN: the largest keys
    rows = np.stack([_distribution("constant", M), _distribution("ties", M), _distribution("signed_zero", M), inf,
                     bits.view(np.float32)])
    return rows, [0.3, 0.1, 0.5, 0.2, 0.004]


@pytest.mark.parametrize("M", [3000, 12288, 12289])
def test_designed_rows_equal_the_single_row_call(M):
    from riskaversetrajopt_amd import stats
    rows, alphas = _designed_rows(M)
    Z = _padded(rows)
    assert _bitwise(Z[:, :M].cpu().numpy(), rows)
    got = _rows_call(Z, M, alphas)
    how = stats.risk_stats_device if M <= RS_SMALL_MAX else stats.risk_stats_recover_device
    want = _single(Z, M, alphas, how)
    assert _bitwise(got, want), (M, got, want)
    # and they are what they are meant to be
    assert got[0, 0] == -1.25 and got[0, 9] == M and got[0, 8] == 0                       # constant: everything ties
    k1 = _rank(M, alphas[1])
    srt = np.sort(rows[1])
    assert got[1, 0] == srt[k1] and got[1, 9] == np.sum(rows[1] == srt[k1]) > 1 and srt[k1 - 1] == srt[k1] == srt[k1 + 1]
    assert got[2, 0] == 0.0 and got[2, 9] == M and got[2, 8] == 0                         # +0 and -0 are one value
    assert got[3, 4] == np.inf and got[3, 0] == np.sort(rows[3])[_rank(M, alphas[3])]
    k4 = _rank(M, alphas[4])                                                              # rank and VaR only: sums over NaN mean nothing
    want4 = _values(np.sort(_keys(rows[4].view(np.uint32)))[k4:k4 + 1])[0]
    assert got[4, 7] == k4 and (np.isnan(got[4, 0]) if np.isnan(want4) else got[4, 0] == want4)


# ---- 4. alphas ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1000, 12289])
def test_alpha_edges_and_equal_alphas_in_non_adjacent_rows(M):
    from riskaversetrajopt_amd import stats
    alphas = [1.0, 1.0 / M, 0.5 / M, 0.3, 0.7, 0.3]
    K = len(alphas)
    host = _random_rows(K, M, seed=M)
    host[5] = host[3]                                    # the same row at the same alpha, two rows apart
    Z = _padded(host)
    got = _rows_call(Z, M, alphas)
    how = stats.risk_stats_device if M <= RS_SMALL_MAX else stats.risk_stats_recover_device
    assert _bitwise(got, _single(Z, M, alphas, how))
    for k in range(K):
        _check_against_numpy(got[k], host[k], alphas[k], (M, k))
    assert got[0, 0] == host[0].max() and got[0, 10] == host[0].min() and got[0, 7] == 0, "alpha = 1: VaR wraps to the maximum"
    assert got[1, 7] == _rank(M, 1.0 / M) and got[1, 7] in (M - 2, M - 1)
    assert got[2, 7] == M - 1 and got[2, 0] == host[2].max() and got[2, 8] == 0, "alpha < 1 / M: the rank is M - 1"
    assert _bitwise(got[3], got[5])


def _assert_histograms_zero_and_tagged(ws, K, what):
    import torch
    w = ws.view(torch.int32).cpu().numpy().view(np.uint32).reshape(K, WS_WORDS)
    assert not w[:, :5120].any(), what
    assert np.all(w[:, -10] == RS_MAGIC), what


@pytest.mark.parametrize("M", [1000, 12289])
def test_invalid_alphas_give_nan_records_in_exactly_those_rows(M):
    from riskaversetrajopt_amd import stats
    alphas = [0.3, 0.0, 0.2, -0.5, 1.5, 0.1, float("nan"), 0.4]
    bad = [1, 3, 4, 6]
    good = [0, 2, 5, 7]
    K = len(alphas)
    host = _random_rows(K, M, seed=7 * M)
    Z = _padded(host)
    ws = stats.new_rows_workspace(M, K, DEV)
    assert ws.numel() == (K * WS_WORDS * 4 if M > RS_SMALL_MAX else 0)
    got = _rows_call(Z, M, alphas, ws=ws)
    assert np.isnan(got[bad]).all() and np.isfinite(got[good]).all()
    how = stats.risk_stats_device if M <= RS_SMALL_MAX else stats.risk_stats_recover_device
    want = _single(Z[good], M, [alphas[k] for k in good], how)
    assert _bitwise(got[good], want)
    if M > RS_SMALL_MAX:
        _assert_histograms_zero_and_tagged(ws, K, "after a call with invalid rows")
    valid = _different_alphas(K)
    again = _rows_call(Z, M, valid, ws=ws)               # the same workspace, every alpha valid
    assert _bitwise(again, _single(Z, M, valid, how))
    if M > RS_SMALL_MAX:
        _assert_histograms_zero_and_tagged(ws, K, "after the second call")


# ---- 5. workspace and replay ------------------------------------------------------------------------------------------------------
def test_three_calls_on_one_workspace_are_bitwise_equal():
    from riskaversetrajopt_amd import stats
    M, K = 12289, 3
    Z = _padded(_random_rows(K, M, seed=5))
    alphas = [0.05, 0.5, 1.0]
    ws = stats.new_rows_workspace(M, K, DEV)
    recs = [_rows_call(Z, M, alphas, ws=ws) for _ in range(3)]
    assert np.isfinite(recs[0]).all() and _bitwise(recs[0], recs[1]) and _bitwise(recs[0], recs[2])
    _assert_histograms_zero_and_tagged(ws, K, "after three calls")


def test_an_untagged_workspace_gives_nan_in_every_row():
    import torch
    M, K = 12289, 3
    Z = _padded(_random_rows(K, M, seed=6))
    ws = torch.zeros(K * WS_WORDS * 4, dtype=torch.uint8, device=DEV)      # the right size, never initialised
    got = _rows_call(Z, M, [0.1, 0.2, 0.3], ws=ws)
    assert np.isnan(got).all()


def test_a_captured_call_replayed_twice_equals_the_eager_call():
    """M = 12,289: a linear chain of five kernels in one hipGraph"""
    import torch
    from riskaversetrajopt_amd import stats
    M, K = 12289, 3
    first, second = _random_rows(K, M, seed=8), _random_rows(K, M, seed=9)
    Z = _padded(first)
    alphas = torch.tensor([0.05, 0.5, 1.0], dtype=torch.float64, device=DEV)
    ws = stats.new_rows_workspace(M, K, DEV)
    out = torch.empty((K, N), dtype=torch.float64, device=DEV)
    eager_first = _rows_call(Z, M, alphas, ws=ws, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stats.risk_stats_rows_device(Z, alphas, thr=THR, workspace=ws, out=out, M=M)
    for rep in range(2):
        out.fill_(-5.0)
        g.replay()
        torch.cuda.synchronize()
        assert _bitwise(out.cpu().numpy(), eager_first), rep
    Z[:, :M] = torch.from_numpy(second).to(DEV)          # in place: the graph holds the pointers
    alphas.copy_(torch.tensor([0.3, 0.2, 0.1], dtype=torch.float64))
    g.replay()
    torch.cuda.synchronize()
    replayed = out.cpu().numpy().copy()
    assert _bitwise(replayed, _rows_call(Z, M, alphas, ws=stats.new_rows_workspace(M, K, DEV)))
    assert not _bitwise(replayed, eager_first)


def test_host_wrapper_returns_the_dicts_of_risk_stats():
    from riskaversetrajopt_amd import stats
    M, K = 700, 4
    host = _random_rows(K, M, seed=11)
    Z = _padded(host)[:, :M].contiguous()
    alphas = [0.1, 0.2, 0.1, 1.0]
    recs = stats.risk_stats_rows(Z, alphas, thr=THR)
    assert len(recs) == K
    for k in range(K):
        assert recs[k] == stats.risk_stats(Z[k], alphas[k], thr=THR), k
    with pytest.raises(ValueError, match="alphas"):
        stats.risk_stats_rows_device(Z, [0.1, 0.2])
    with pytest.raises(stats._lib.RatoError):
        stats.risk_stats_rows_device(Z.cpu(), alphas)


# ---- 6. the facades -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system,M,S,K", [("drone", 300, 20, 8), ("drone", 12289, 20, 3), ("driving", 300, 20, 8)])
def test_eval_batch_device_with_alphas_equals_the_call_per_alpha(system, M, S, K):
    import torch
    d, n_u = _model(system, M, S)
    us = np.stack([_us(S, n_u, k) for k in range(K)])
    alphas = ([0.05, 0.1, 0.2, 0.3] * 2)[:K] if K == 8 else [0.05, 0.3, 0.05]
    Zg, recg = d.eval_batch_device(us, alphas=alphas)
    torch.cuda.synchronize()
    assert tuple(Zg.shape) == (K, M) and tuple(recg.shape) == (K, N)
    Zg_h, recg_h = Zg.cpu().numpy(), recg.cpu().numpy()
    for a in sorted(set(alphas)):
        idx = [k for k in range(K) if alphas[k] == a]
        Za, reca = d.eval_batch_device(us[idx], alpha=a)
        Za_h, reca_h = Za.cpu().numpy(), reca.cpu().numpy()
        assert _bitwise(Zg_h[idx], Za_h), (a, "Z")
        if M <= RS_SMALL_MAX:
            assert _bitwise(recg_h[idx], reca_h), (a, recg_h[idx], reca_h)
        else:
            assert _bitwise(recg_h[idx][:, EXACT], reca_h[:, EXACT]), (a, recg_h[idx], reca_h)
            for j, k in enumerate(idx):
                _check_against_numpy(recg_h[k], Za_h[j], a, (system, M, k))
    with pytest.raises(ValueError, match="alpha"):
        d.eval_batch_device(us, alpha=0.1, alphas=alphas)
    with pytest.raises(ValueError, match="alphas"):
        d.eval_batch_device(us, alphas=alphas[:-1])
    Zn, recn = d.eval_batch_device(us)                   # without alphas nothing changes
    assert _bitwise(Zn.cpu().numpy(), Zg_h) and tuple(recn.shape) == (K, N)


# ---- 7. the reports ---------------------------------------------------------------------------------------------------------------
def _same_reports(a, b):
    assert list(a) == list(b)
    for alpha in a:
        assert sorted(a[alpha]) == sorted(b[alpha]), alpha
        for key, v in a[alpha].items():
            assert _bitwise(np.asarray(v), np.asarray(b[alpha][key])), (alpha, key, v, b[alpha][key])


def test_report_grid_equals_the_report_per_alpha():
    from riskaversetrajopt_amd import scp
    A, R, S, M_mc = 2, 3, 20, 300
    mc, n_u = _model("drone", M_mc, S)
    alphas = [0.1, 0.3]
    us_grid = np.stack([np.stack([_us(S, n_u, i * R + r) for r in range(R)]) for i in range(A)])
    grid = scp.monte_carlo_report_grid(mc, us_grid, alphas)
    loop = {a: scp.monte_carlo_report(mc, list(us_grid[i]), a) for i, a in enumerate(alphas)}
    _same_reports(grid, loop)
    assert all(np.isfinite(grid[a]["avar"]).all() and len(grid[a]["avar"]) == R for a in alphas)
    with pytest.raises(ValueError, match="alphas"):
        scp.monte_carlo_report_grid(mc, us_grid, alphas[:1])


def test_saa_experiment_reports_are_the_same_under_both_mc_modes():
    from riskaversetrajopt_amd import scp
    S = 20
    mc, _ = _model("drone", 300, S)
    kw = dict(alphas=(0.1, 0.3), num_repeats=2, M=10, S=S, iters=3, seed=0, mc_model=mc)
    a = scp.drone_saa_experiment(**kw)
    b = scp.drone_saa_experiment(mc='grid', **kw)
    assert _bitwise(a["us"], b["us"])
    _same_reports(a["reports"], b["reports"])
    with pytest.raises(ValueError, match="mc must be"):
        scp.drone_saa_experiment(mc='both', **kw)


# ---- 8. hopper ----------------------------------------------------------------------------------------------------------------------
def _hopper(M, seed):
    from riskaversetrajopt_amd import hopper
    return hopper.Model.from_device(*hopper.sample_friction_fields_device(M, seed=seed, device=DEV))


def _hopper_contacts(K, Cn, seed):
    rng = np.random.RandomState(seed)
    px = rng.uniform(-3, 3, (K, Cn))
    fz = 32.0 + rng.randn(K, Cn)
    fx = 0.1 * fz + 0.3 * rng.randn(K, Cn)
    return px, np.stack([fx, fz], axis=-1)


@pytest.mark.parametrize("M,K", [(500, 7), (12289, 3)])
def test_hopper_rows_selection_equals_the_entry_points_selection(M, K):
    d = _hopper(M, seed=3)
    px, forces = _hopper_contacts(K, 7, seed=M)
    alphas = ([0.05, 0.05, 0.3, None, 0.3, 0.75, 0.05])[:K] if K == 7 else [0.3, None, 0.05]
    Ze, rece, arge = d.eval_batch_device(px, forces, alphas=alphas, want_arg=True)
    Zr, recr, argr = d.eval_batch_device(px, forces, alphas=alphas, want_arg=True, selection='rows')
    assert _bitwise(Ze.cpu().numpy(), Zr.cpu().numpy()) and _bitwise(arge.cpu().numpy(), argr.cpu().numpy())
    e, r = rece.cpu().numpy(), recr.cpu().numpy()
    assert np.isfinite(r).all()
    if M <= RS_SMALL_MAX:
        assert _bitwise(e, r), (e, r)
    else:
        assert _bitwise(e[:, EXACT], r[:, EXACT]), (e, r)
    none = alphas.index(None)
    assert r[none, 0] == r[none, 4], "a None alpha is selected at 1.0: VaR is the maximum"
    with pytest.raises(ValueError, match="selection"):
        d.eval_batch_device(px, forces, alphas=alphas, selection='both')


def test_hopper_report_is_bitwise_the_same_under_both_selections():
    from riskaversetrajopt_amd import scp
    M, K = 500, 7
    mc = _hopper(M, seed=4)
    rng = np.random.RandomState(12)
    Zs = [mc.initial_guess() * (1.0 + 0.05 * rng.randn(mc.num_vars)) for _ in range(K)]
    alphas = [0.05, 0.1, 0.2, 0.3, 0.5, 0.75, None]
    a = scp.hopper_monte_carlo_report(mc, Zs, alphas)
    b = scp.hopper_monte_carlo_report(mc, Zs, alphas, selection='rows')
    for name in ("alphas", "jump", "frac_satisfied", "var", "avar", "arg_counts"):
        assert _bitwise(a[name], b[name]), (name, a[name], b[name])
    assert np.isfinite(b["var"][:-1]).all() and np.isnan(b["var"][-1])

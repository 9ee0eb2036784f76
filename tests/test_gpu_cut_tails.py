"""GPU: the tail-rows kernels of the cut oracle (csrc/cvar.hip) at ties, full tails and empty tails against fp64.

The kernels turn a cut's tail weighting into the cut's gradient and offset; their control flow depends on how many tail
samples fall into one block of 256 samples (n_tail, work_waves, the chunks of 64 the rollout forms walk) and on the
horizon.  They take the m values, the arg-max rows and the statistics record as inputs, so tests/_tail_patterns.py designs
them: pack(n) (n = 0 .. 256 tail samples in block 0: work_waves 0 .. 4, every chunk-count edge, an empty block), ties
(lambda = 1, 1/2, 2/3, 3/4, 0.04, 1/481, 0.2; a tie group across a block edge; all samples equal), fractional alpha M (the
last block one sample), alpha = 1 (every weight 1) and alpha M = 1/2, each with arg-max rows that are random, all at
step 0, all at step S - 1, one per 64 at S - 1, or of one row group.  tests/test_tail_patterns.py shows that every mistake
such a kernel could make moves the reference by >= 1000 tolerances.

Reference of the rollout forms: the fp64 oracle's dense rows on the same fp32-rounded samples, under the bounds those
kernels already had (gradient rtol 1e-7 + 1e-8 max(1, max|grad|); offset 1e-8 (w.|g| + 1)) plus what carrying lambda as a
float costs, |float(lam) - lam| sum_ties |entry| (<= 2^-24 lam sum_ties |entry|; 0 where lambda is 1).  Reference of the table
forms: fp64 sums over the device's own fp32 tables read back, bound 4 N eps64 sum |w entry| + the same float-lambda term.

Horizons of the per-cut drone kernel, by the arithmetic of tail_rows_lds: the LDS of the sums and the e22 table is
8 (2 (S - 1) + 1) + 512 S bytes, the per-lane term table 2 (S - 1) 65 8 bytes more; term table while both + 4096 <= 81920,
i.e. S <= 50 (S = 50: 81448, S = 51: 83016); lane registers while S - 1 <= 64, i.e. 51 <= S <= 65; LDS read-modify-write from
S = 66.  Hence S in {50, 51, 65, 66} beside 2, 3 and 20.  The table kernel gathers 8 columns per batch: S - 1 in {1, 8, 9, 19}.

Largest observed error on the MI355X, next to the bound it was held to (records, not tolerances):
  rollout forms vs the fp64 oracle (per-cut launches and the `slots` launch give the same figures)
    drone,   no lambda to round (pack, alpha = 1):  gradient 1.35e-08 of max(1, max|grad|) = 0.123 of its bound,
                                                    offset 6.6e-16 of (w.|g| + 1) = 6.6e-08 of its bound
    drone,   ties / fractional / alpha M = 1/2:     gradient 3.77e-08 (0.261 of its bound), offset 2.97e-08 (0.748)
    driving, no lambda to round:                    gradient 6.61e-09 (0.060), offset 3.7e-16 (3.7e-08)
    driving, ties / fractional / alpha M = 1/2:     gradient 4.08e-08 (0.272), offset 2.73e-08 (0.732)
  drone union form vs one launch per cut:           3.9e-16 of the row's max (bound 1e-12); driving: 0 (the same kernel)
  rato_saa_tail_rows_batch vs fp64 sums of its tables: explicit, factored and R = 1 reach 1.00 of the bound on ties (the
    float-lambda term is attained where the tied entries of a column share a sign); without ties explicit 0 (exact),
    factored 1.1e-02 of 4 N eps64 sum |w entry|
  rato_drone_tail_rows_implicit vs the explicit kernel: a22_axes 2: 3.1e-08, a22_axes 3: 2.5e-07 of max(1, row max)
    (bound rtol 2e-5 + 2e-6)
  rato_kkt_sums: 1.00 of n_eq |float(lam) - lam| + 4 M eps64 alpha M on ties (attained), 3.1e-04 of it without
No kernel had to change for these tests.  They do fail on wrong kernels: with the carry across chunks dropped (term-table,
register and LDS path of the per-cut kernel, the driving kernel), the k0 offset of the second union launch lost, only the
first wave's row summed in the table kernels and lambda = 1 in rato_kkt_sums, 49 of the 51 cases failed (by ~7e6 bounds for
the rollout forms); the two that passed are the ones those mistakes do not touch.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _tail_patterns as tp

pytestmark = pytest.mark.gpu

N_STATS = 11


class Ring:
    """K cuts (pattern x arg kind) in ring rows chosen by a permutation: m values, arg-max rows and the statistics record the
    device computes from the m values"""

    def __init__(self, patterns, S, R, M, alpha, device, seed=0, K_min=0, kinds=None):
        import torch
        from riskaversetrajopt_amd import stats
        rng = np.random.RandomState(seed)
        cuts = [(p, kind) for p in patterns for kind in (kinds or tp.arg_kinds(R))]
        cuts += [cuts[i % len(cuts)] for i in range(max(0, K_min - len(cuts)))]
        self.cuts, self.K, self.M, self.S, self.alpha, self.alphaM = cuts, len(cuts), M, S, alpha, alpha * M
        self.row = rng.permutation(self.K)                          # cut k lives in ring row row[k]: not the identity
        if self.K > 1 and np.array_equal(self.row, np.arange(self.K)):
            self.row = self.row[::-1].copy()
        self.arg = [tp.args(kind, S, R, M, rng) for _, kind in cuts]
        m_np, a_np = np.empty((self.K, M), np.float32), np.empty((self.K, M), np.int32)
        for k, (p, _) in enumerate(cuts):
            assert p.M == M and p.alpha == alpha
            m_np[self.row[k]], a_np[self.row[k]] = p.m, self.arg[k]
        self.m_base = torch.as_tensor(m_np, device=device)
        self.arg_base = torch.as_tensor(a_np, device=device)
        self.stats_base = torch.zeros((self.K, N_STATS), dtype=torch.float64, device=device)
        ws = stats.new_workspace(M, device)
        for j in range(self.K):
            stats.risk_stats_device(self.m_base[j], alpha, workspace=ws, out=self.stats_base[j])
        self.slots = torch.as_tensor(self.row.astype(np.int32), device=device)
        # the weights the kernels derive from the device's record are the reference's (both in fp64, same formula).  The
        # WEIGHTS are compared, not the record: where alpha M is an integer and the ceil(alpha M)-th largest value is untied,
        # every t down to the next value minimises the Rockafellar-Uryasev function, and a record that names the other end
        # of that interval (n_gt = alpha M, lambda = 0) describes the same weighting
        rec = self.stats_base.cpu().numpy()
        self.w, self.tie, self.lam = [], [], []
        for k, (p, _) in enumerate(cuts):
            w, t, n_gt, n_eq, lam = p.weights()
            st = rec[self.row[k]]
            td, lam_d = np.float32(st[10]), (min(max((self.alphaM - st[8]) / st[9], 0.0), 1.0) if st[9] > 0 else 0.0)
            assert np.array_equal((p.m > td) * 1.0 + (p.m == td) * lam_d, w), (p.name, st[8:11], (t, n_gt, n_eq))
            if alpha == 1.0:
                assert st[10] == p.m.min()                         # slot 10 of the record is min(m) when every sample is in the tail
            self.w.append(w), self.tie.append(p.m == np.float32(t)), self.lam.append(lam)

    def refs(self, Gc, g):
        return [tp.cut_sums(Gc, g, self.w[k], self.arg[k], self.tie[k], self.lam[k]) for k in range(self.K)]


def _check_rollout(form, ring, part, refs, worst):
    """part (nblk, K, nc) of one form against the fp64 oracle's sums: bounds, and the outcomes that are exact"""
    nw = part.shape[2] - 1
    for k, (p, kind) in enumerate(ring.cuts):
        ref, sums = refs[k], part[:, k].sum(axis=0)
        assert np.isfinite(part[:, k]).all(), (form, p.name, kind)
        tol_grad, tol_off = tp.rollout_tolerance(ref)
        e_grad, e_off = np.abs(sums[:nw] - ref["grad"]), abs(sums[nw] - ref["off"])
        scale = max(1.0, np.abs(ref["grad"]).max(initial=0.0))
        worst["grad"] = max(worst.get("grad", 0.0), float(np.max(e_grad / tol_grad)))
        worst["grad_rel"] = max(worst.get("grad_rel", 0.0), float(e_grad.max()) / scale)
        worst["off"] = max(worst.get("off", 0.0), e_off / tol_off)
        worst["off_rel"] = max(worst.get("off_rel", 0.0), e_off / (ref["abs_off"] + 1.0))
        assert np.all(e_grad <= tol_grad), (form, p.name, kind, float(np.max(e_grad / tol_grad)))
        assert e_off <= tol_off, (form, p.name, kind, e_off / tol_off)
        if kind == "step0":                                        # no control enters g_0: every gradient column is exactly 0
            assert np.all(part[:, k, :nw] == 0.0), (form, p.name)
        for b, c in enumerate(p.counts):                           # a block with an empty tail: its row of part is exactly 0
            if c == 0:
                assert np.all(part[b, k] == 0.0), (form, p.name, kind, b)


def _run_rollout(system, S, grp):
    import torch
    from riskaversetrajopt_amd import _lib
    if system == "drone":
        from riskaversetrajopt_amd import drone_risk
        rows, R, name = tp.drone_rows(S), 3, "rato_drone_tail_rows_rollout"
    else:
        from riskaversetrajopt_amd import driving
        rows, R, name = tp.driving_rows(S), 1, "rato_car_tail_rows_rollout"
    nw = 2 * (S - 1)
    nc = nw + 1
    # the oracle's dense rows grow with S^2: the shorter pack list n in {0, 64, 65, 256} at S >= 50.  M stays 600 there (the
    # oracle takes 0.8 s at S = 66): with M = 300 the second block has 44 samples, too few to hold the tail pack(0) moves out
    # of block 0, and the tie patterns (100,500), (119,481), (0,600) need 600 samples
    short = S >= 50
    for M, alpha, patterns in tp.group(grp, short=short):
        smp = [a[:M] for a in rows["samples"]]
        if system == "drone":
            d = drone_risk.Model(S, *smp, 'saa', alpha)
            dW, mass, Qsym, _ = d._inputs(None)
            p, inputs = d._params(M, mass.numel()), (dW, mass, Qsym)
        else:
            d = driving.Model(M, 'saa', alpha, S=S, samples=smp)
            p, inputs = d._params(M), (d._dW, d._x0, d._ws, d._wr)
        dev, lib = d.device, d._lib
        uk_d = torch.as_tensor(rows["uk"], dtype=torch.float64, device=dev).contiguous()
        # alpha = 1: K = 17 cuts, so the union launcher splits 16 + 1 and a wave takes the cuts `wave` and `wave + 8`
        ring = Ring(patterns, S, R, M, alpha, dev, seed=S, K_min=17 if grp == "everything" else 0)
        K, nblk = ring.K, (M + 255) // 256
        refs = ring.refs(rows["Gc"][:M], rows["g"][:M])

        def launch(m_base, arg_base, stats_base, slots, k, part):
            _lib.check(getattr(lib, name)(C.byref(p), _lib.ptr(uk_d), *[_lib.ptr(a) for a in inputs], _lib.ptr(m_base),
                                          _lib.ptr(arg_base), _lib.ptr(stats_base), N_STATS, _lib.ptr(slots), k, ring.alphaM,
                                          _lib.ptr(part), _lib.current_stream()), name)

        # one launch per cut: slots = NULL, K = 1, the pointers are the ring row (the per-cut kernel)
        one = torch.full((K, nblk, nc), np.nan, dtype=torch.float64, device=dev)
        for k in range(K):
            j = int(ring.row[k])
            launch(ring.m_base[j], ring.arg_base[j], ring.stats_base[j], None, 1, one[k])
        # all cuts in one launch through `slots` (drone: the union kernel, chunks of 16 cuts; driving: gridDim.y = K)
        allk = torch.full((nblk, K, nc), np.nan, dtype=torch.float64, device=dev)
        launch(ring.m_base, ring.arg_base, ring.stats_base, ring.slots, K, allk)
        torch.cuda.synchronize()
        one, allk = one.cpu().numpy().transpose(1, 0, 2), allk.cpu().numpy()
        for form, part in (("per cut", one), ("slots", allk)):
            worst = {}
            _check_rollout(f"{system} {form}", ring, part, refs, worst)
            print(f"OBS {system:<8s}rollout {form:<8s} S={S:<3d} {grp:<10s} M={M:<4d} K={K:<3d} gradient: max|err|/max(1,max|grad|) "
                  f"{worst['grad_rel']:.2e}, err/bound {worst['grad']:.2e};  offset: |err|/(w.|g|+1) {worst['off_rel']:.2e}, "
                  f"err/bound {worst['off']:.2e}")
        # the two launch forms against each other: same rollout arithmetic, the same fp64 sums in another order
        a, b = allk.sum(axis=0), one.sum(axis=0)
        err = np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)
        print(f"OBS {system:<8s}rollout slots vs per cut S={S} {grp} M={M}: max|diff|/row max {err.max():.2e}")
        assert err.max() < 1e-12


# (S, group): every group at S = 20; pack / ties / everything on both sides of the two regime edges of the per-cut kernel
DRONE_CASES = [(20, g) for g in tp.GROUPS] + [(S, g) for S in (2, 3, 50, 51, 65, 66) for g in ("pack", "ties", "everything")]
CAR_CASES = [(20, g) for g in tp.GROUPS] + [(S, g) for S in (2, 66) for g in ("pack", "ties", "everything")]


@pytest.mark.parametrize("S,grp", sorted(DRONE_CASES))
def test_drone_rollout_tail_rows_vs_fp64_oracle(S, grp):
    _run_rollout("drone", S, grp)


@pytest.mark.parametrize("S,grp", sorted(CAR_CASES))
def test_driving_rollout_tail_rows_vs_fp64_oracle(S, grp):
    _run_rollout("driving", S, grp)


# ---- table forms ---------------------------------------------------------------------------------------------------
def _check_table(form, ring, part, refs):
    nw = part.shape[2] - 1
    worst = 0.0
    for k, (p, kind) in enumerate(ring.cuts):
        ref, sums = refs[k], part[:, k].sum(axis=0)
        tol_grad, tol_off = tp.table_tolerance(ref)
        e_grad, e_off = np.abs(sums[:nw] - ref["grad"]), abs(sums[nw] - ref["off"])
        ratio = max(float(np.max(e_grad / np.maximum(tol_grad, 1e-300), initial=0.0)), e_off / max(tol_off, 1e-300))
        worst = max(worst, ratio)
        assert np.all(e_grad <= tol_grad), (form, p.name, kind, ratio)
        assert e_off <= tol_off, (form, p.name, kind, ratio)
        if kind == "step0":
            assert np.all(part[:, k, :nw] == 0.0), (form, p.name)
        for b, c in enumerate(p.counts):
            if c == 0:
                assert np.all(part[b, k] == 0.0), (form, p.name, kind, b)
    return worst


def _factored_dense(r, S, M):
    """double(W) * double(Phi) from the factored tables read back: (M, 3 S, 2 (S - 1))"""
    from riskaversetrajopt_amd.drone_risk import untile
    Phi = untile(r["G"], M).double().cpu().numpy()                  # (n_pairs, 2, M)
    W = r["W"].double().cpu().numpy()                               # (3, S, 2, M)
    Gc = np.zeros((M, 3, S, S - 1, 2))
    for t in range(1, S):
        off = t * (t - 1) // 2
        Gc[:, :, t, :t, :] = np.transpose(W[:, t][:, None] * Phi[off:off + t][None], (3, 0, 1, 2))
    return Gc.reshape(M, 3 * S, 2 * (S - 1))


@pytest.mark.parametrize("S", [2, 9, 10, 20])
@pytest.mark.parametrize("grp", ["pack", "ties", "everything"])
def test_table_tail_rows_vs_fp64_sums_of_the_device_tables(grp, S):
    """rato_saa_tail_rows_batch (R = 3 explicit, R = 3 factored, R = 1 from the driving row kernel) against fp64 sums over
    the very fp32 tables the kernel read; rato_drone_tail_rows_implicit (a22_axes 2 and 3) against the explicit kernel."""
    import torch
    from riskaversetrajopt_amd import _lib, drone_risk, driving
    nw = 2 * (S - 1)
    nc = nw + 1
    for M, alpha, patterns in tp.group(grp):
        nblk = (M + 255) // 256
        rng = np.random.RandomState(S)
        r32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        from oracle import drone as od, driving as ocar
        # ---- drone
        d = drone_risk.Model(S, *[r32(a) for a in od.sample_uncertain_parameters(rng, 'saa', M=M, S=S)], 'saa', alpha)
        dev, lib = d.device, d._lib
        uk = tp.graze(S)
        ring = Ring(patterns, S, 3, M, alpha, dev, seed=100 + S)
        K = ring.K
        mass = d._inputs(None)[1]
        ld = mass.numel()
        p = d._params(M, ld)

        def batch(G, W, ldim, tile, R, base, rg):
            part = torch.full((nblk, rg.K, nc), np.nan, dtype=torch.float64, device=dev)
            _lib.check(lib.rato_saa_tail_rows_batch(_lib.ptr(G), _lib.ptr(W), ldim, tile, R, S, M, _lib.ptr(base),
                                                    _lib.ptr(rg.m_base), _lib.ptr(rg.arg_base), _lib.ptr(rg.stats_base), N_STATS,
                                                    _lib.ptr(rg.slots), rg.K, rg.alphaM, _lib.ptr(part), _lib.current_stream()),
                       "rato_saa_tail_rows_batch")
            return part

        def implicit(r, axes):
            part = torch.full((nblk, K, nc), np.nan, dtype=torch.float64, device=dev)
            _lib.check(lib.rato_drone_tail_rows_implicit(C.byref(p), _lib.ptr(mass), _lib.ptr(r["_A22"]), axes, _lib.ptr(r["_W"]),
                                                         _lib.ptr(r["_g_up"]), _lib.ptr(ring.m_base), _lib.ptr(ring.arg_base),
                                                         _lib.ptr(ring.stats_base), N_STATS, _lib.ptr(ring.slots), K, ring.alphaM,
                                                         _lib.ptr(part), _lib.current_stream()), "rato_drone_tail_rows_implicit")
            return part

        ex = d.linearize_device(uk, factored=False, rows_out=1)
        fa = d.linearize_device(uk, want_A22=True, rows_out=1)
        gen = d.linearize_generators_device(uk, rows_out=1)
        assert not ex["factored"] and fa["factored"] and ex["_W"] is None
        p_ex = batch(ex["G"], None, ld, ex["tile"], 3, ex["_g_up"], ring)
        p_fa = batch(fa["G"], fa["_W"], ld, fa["tile"], 3, fa["_g_up"], ring)
        p_i2, p_i3 = implicit(fa, 2), implicit(gen, 3)
        torch.cuda.synchronize()
        base = lambda r: r["g_up"].permute(2, 0, 1).double().cpu().numpy().reshape(M, 3 * S)
        Gc_ex = d.expand_g_obs_du(ex).reshape(M, 3 * S, S, 3)[:, :, :S - 1, :2].reshape(M, 3 * S, nw)
        w_ex = _check_table("explicit", ring, p_ex.cpu().numpy(), ring.refs(Gc_ex, base(ex)))
        w_fa = _check_table("factored", ring, p_fa.cpu().numpy(), ring.refs(_factored_dense(fa, S, M), base(fa)))
        print(f"OBS table R=3 explicit S={S} {grp} M={M} K={K}: max err/bound {w_ex:.2e};  factored: {w_fa:.2e}")
        # the rows regenerated in fp64 from the fp32 A22 table against the stored fp32 entries: equal to their rounding
        b = p_ex.sum(0).cpu().numpy()
        for axes, pi in ((2, p_i2), (3, p_i3)):
            a = pi.sum(0).cpu().numpy()
            for k, (pt, kind) in enumerate(ring.cuts):
                tol = 2e-5 * np.abs(b[k]) + 2e-6 * max(1.0, np.abs(b[k]).max())
                assert np.all(np.abs(a[k] - b[k]) <= tol), (axes, pt.name, kind, float(np.max(np.abs(a[k] - b[k]) / tol)))
                if kind == "step0":
                    assert np.all(pi[:, k, :nw].cpu().numpy() == 0.0)
            print(f"OBS table implicit a22_axes={axes} vs explicit S={S} {grp} M={M}: max|diff|/max(1,row max) "
                  f"{np.max(np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))):.2e}")
        # ---- driving (R = 1, ld = M)
        c = driving.Model(M, 'saa', alpha, S=S, samples=[r32(a) for a in ocar.sample_uncertain_parameters(rng, M, 'saa', S)])
        ring1 = Ring(patterns, S, 1, M, alpha, dev, seed=200 + S)
        rc = c.linearize_device(tp.driving_uk(S), rows_out=1)
        p_c = batch(rc["G"], None, M, rc["tile"], 1, rc["g_up"], ring1)
        torch.cuda.synchronize()
        Gc_c = c.expand_g_obs_du(rc["G"], M).reshape(M, S, S, 2)[:, :, :S - 1].reshape(M, S, nw)
        w_c = _check_table("driving", ring1, p_c.cpu().numpy(), ring1.refs(Gc_c, rc["g_up"].t().double().cpu().numpy()))
        print(f"OBS table R=1 driving  S={S} {grp} M={M} K={ring1.K}: max err/bound {w_c:.2e}")


# ---- the weights alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grp", tp.GROUPS)
def test_kkt_sums_weights_vs_the_counts(grp):
    """rato_kkt_sums uses the same tail weighting: column [K + k] = sum_i w_ki = n_gt + n_eq lam, column [k] =
    sum_i w_ki (m*_i - v)^+ for an m* and v of the test's choosing"""
    import torch
    from riskaversetrajopt_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda:0")
    for M, alpha, patterns in tp.group(grp):
        ring = Ring(patterns, 2, 1, M, alpha, dev, seed=7, kinds=("step0",))
        K, nblk = ring.K, (M + 255) // 256
        rng = np.random.RandomState(11)
        m_star32 = rng.randn(M).astype(np.float32)
        v = 0.1
        lam = torch.as_tensor(rng.uniform(0.1, 1.0, size=K), dtype=torch.float64, device=dev)
        part = torch.full((nblk, 2 * K + 2), np.nan, dtype=torch.float64, device=dev)
        _lib.check(lib.rato_kkt_sums(_lib.ptr(torch.as_tensor(m_star32, device=dev)), M, _lib.ptr(ring.m_base),
                                     _lib.ptr(ring.stats_base), N_STATS, _lib.ptr(ring.slots), _lib.ptr(lam), K, ring.alphaM, v,
                                     _lib.ptr(part), _lib.current_stream()), "rato_kkt_sums")
        torch.cuda.synchronize()
        sums = part.sum(0).cpu().numpy()
        ex = np.maximum(m_star32.astype(np.float64) - v, 0.0)
        worst = 0.0
        for k, (p, _) in enumerate(ring.cuts):
            bound = p.n_eq * tp.float_lambda_error(p.lam) + 4 * M * tp.EPS64 * ring.alphaM
            e_w = abs(sums[K + k] - (p.n_gt + p.n_eq * p.lam))
            e_x = abs(sums[k] - float(ring.w[k] @ ex))
            worst = max(worst, e_w / bound, e_x / (bound * ex.max()))
            assert e_w <= bound, (p.name, e_w, bound)
            assert e_x <= bound * ex.max(), (p.name, e_x, bound * ex.max())
        assert abs(sums[2 * K] - ex.sum()) <= 4 * M * tp.EPS64 * ex.sum()
        print(f"OBS kkt_sums {grp} M={M} K={K}: max err/bound {worst:.2e}")

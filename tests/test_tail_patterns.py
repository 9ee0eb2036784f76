"""CPU: the reference of tests/test_gpu_cut_tails.py checked by itself.  Every designed pattern yields the counts it
declares and weights that sum to alpha M; and on the fp64 oracle's dense rows each mistake a tail-rows kernel could
make (tests/_tail_patterns.WRONG_RULES) moves the cut's gradient by >= 1000 x the tolerance the GPU test applies to that
comparison -- which is what makes the GPU tests able to fail."""
import numpy as np
import pytest

from tests import _tail_patterns as tp


def _all_patterns(short=False):
    return [p for name in tp.GROUPS for _, _, ps in tp.group(name, short) for p in ps]


def test_every_pattern_yields_the_counts_it_declares():
    seen = set()
    for p in _all_patterns() + _all_patterns(short=True):
        w, t, n_gt, n_eq, lam = p.check().weights()
        assert p.m.dtype == np.float32 and p.m.shape == (p.M,)
        assert (n_gt, n_eq) == (p.n_gt, p.n_eq) and abs(lam - p.lam) <= 1e-13
        assert tuple(tp.block_counts(w != 0, p.M)) == p.counts
        seen.add(p.name)
    # the cases the kernels' control flow turns on
    assert {f"pack({n})" for n in tp.PACK_N} <= seen and {f"ties({a},{b})" for a, b in tp.TIES} <= seen
    packs = {p.name: p for p in tp.group("pack")[0][2]}
    assert [-(-packs[f"pack({n})"].counts[0] // tp.WAVE) for n in (0, 1, 64, 65, 128, 129, 192, 193, 256)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    t = {p.name: p for p in tp.group("ties")[0][2]}
    assert np.array_equal(np.flatnonzero(t["ties(118,3)"].m == tp.TIE_VALUE), [255, 256, 257])      # straddles a block edge
    p = t["ties(100,500)"]                                     # block 0: one wave above the threshold, then waves of ties
    assert np.all(p.m[:64] > tp.TIE_VALUE) and np.all(p.m[64:256] == tp.TIE_VALUE)
    assert np.all(t["ties(0,600)"].m == tp.TIE_VALUE)
    lams = sorted(p.lam for p in t.values())
    np.testing.assert_allclose(lams, sorted([1, 1 / 2, 2 / 3, 3 / 4, 0.04, 1 / 481, 0.2]), rtol=1e-13)
    f = {p.name: p for p in tp.group("fractional")[0][2]}
    assert all(abs(p.lam - 0.6) < 1e-12 and p.n_gt == 102 and p.M == 513 for p in f.values())
    assert f["fractional(a)"].counts == (70, 33, 0) and f["fractional(b)"].counts[2] == 1 and f["fractional(c)"].counts[2] == 1
    assert f["fractional(c)"].m[512] == tp.TIE_VALUE and f["fractional(b)"].m[512] > tp.TIE_VALUE
    for M, alpha, ps in tp.group("everything"):
        for p in ps:
            assert alpha == 1.0 and np.all(p.weights()[0] == 1.0) and p.weights()[1] == p.m.min()
    l = tp.group("lt1")[0][2]
    assert [p.lam for p in l[:3]] == [0.5] * 3 and abs(l[3].lam - 1 / 6) < 1e-15
    assert [p.counts for p in l] == [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]


def test_weights_sum_to_alpha_M():
    for p in _all_patterns():
        w = p.weights()[0]
        assert 0.0 < p.alphaM <= p.M
        assert abs(w.sum() - p.alphaM) <= 1e-12 * max(1.0, p.alphaM), (p.name, w.sum(), p.alphaM)
        assert w.min() >= 0.0 and w.max() <= 1.0


def test_weights_agree_with_the_host_cut_solver():
    """the same rule as tests/_host_cuts.HostCutSolver._weights (which the all-fp64 SCP legs use)"""
    from tests._host_cuts import HostCutSolver
    for p in _all_patterns():
        hs = HostCutSolver.__new__(HostCutSolver)
        hs.alphaM, hs.mode = p.alphaM, 'saa'
        w_h, _ = hs._weights(p.m.astype(np.float64))
        assert np.array_equal(w_h, p.weights()[0]), p.name


def test_args_kinds():
    rng = np.random.RandomState(0)
    for R, S in ((3, 20), (1, 20), (3, 2)):
        for kind in tp.arg_kinds(R):
            a = tp.args(kind, S, R, 600, rng)
            assert a.dtype == np.int32 and a.min() >= 0 and a.max() < R * S
            t, r = a % S, a // S
            if kind == "step0":
                assert np.all(t == 0)
            if kind == "last":
                assert np.all(t == S - 1)
            if kind == "sparse":
                assert np.array_equal(np.flatnonzero(t), np.arange(0, 600, 64))
            if kind.startswith("group"):
                assert np.all(r == int(kind[5:]))
            if R == 3 and not kind.startswith("group"):
                assert set(r) == {0, 1, 2}


# which mistakes each pattern class has to expose (a rule that leaves a class's weights unchanged cannot be seen there:
# 'pack' has lam = 1 on a single threshold sample, 'lt1' has at most three tail samples)
EXPOSES = {
    "pack": ("lam=0 on ties", "tail beyond the first 64 of a block dropped", "last block dropped"),
    "ties": ("lam=1 on ties", "lam=0 on ties", ">= in place of >", "tail beyond the first 64 of a block dropped",
             "last block dropped"),
    "fractional": ("lam=1 on ties", "lam=0 on ties", ">= in place of >", "tail beyond the first 64 of a block dropped",
                   "last block dropped"),
    "everything": ("lam=0 on ties", "tail beyond the first 64 of a block dropped", "last block dropped"),
    "lt1": ("lam=1 on ties", "lam=0 on ties", ">= in place of >", "last block dropped"),
}


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_wrong_rules_move_the_reference_by_1000_tolerances(system):
    S, R = 20, (3 if system == "drone" else 1)
    rows = tp.drone_rows(S) if system == "drone" else tp.driving_rows(S)
    rng = np.random.RandomState(3)
    worst = {}
    for name in tp.GROUPS:
        for M, alpha, ps in tp.group(name):
            Gc, g = rows["Gc"][:M], rows["g"][:M]
            rules = EXPOSES[name] + (("row group forced to 0",) if R > 1 else ())
            for rule in rules:
                kinds = ("group1", "group2", "last") if rule.startswith("row group") else ("last",)
                exposed = 0
                for p in ps:
                    w, t, n_gt, n_eq, lam = p.weights()
                    for kind in kinds:
                        arg = tp.args(kind, S, R, M, rng)
                        w_bad, arg_bad = tp.WRONG_RULES[rule](p, arg, S)
                        if np.array_equal(w_bad, w) and np.array_equal(arg_bad[w != 0], arg[w != 0]):
                            continue                 # this pattern does not meet the mistake (e.g. no tail in the last block)
                        ref = tp.cut_sums(Gc, g, w, arg, p.m == np.float32(t), lam)
                        bad = tp.cut_sums(Gc, g, w_bad, arg_bad)
                        tol, _ = tp.rollout_tolerance(ref)              # the widest tolerance the GPU test applies
                        margin = np.abs(bad["grad"] - ref["grad"]).max() / tol.max()
                        worst[(name, rule)] = min(worst.get((name, rule), np.inf), margin)
                        assert margin >= 1000.0, (system, p.name, rule, kind, margin)
                        exposed += 1
                assert exposed > 0, (system, name, rule)
    for k, v in sorted(worst.items()):
        print(f"{system}: {k[0]:>10s} | {k[1]:<44s} smallest margin {v:9.2e} x tolerance")

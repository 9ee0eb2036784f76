"""Test helper (host only, NumPy): designed inputs for the cut oracle's tail-rows kernels (csrc/cvar.hip) and their fp64
reference.

The kernels take the m values, the arg-max rows and the statistics record of a cut as INPUTS, so every branch of their
control flow can be reached with m arrays whose large values sit at chosen sample indices:
  * how many tail samples (weight != 0) fall into one block of 256 samples decides ``n_tail``, ``work_waves`` and the number
    of 64-sample chunks the rollout forms walk;
  * how many samples tie with the threshold decides lambda = clamp((alpha M - n_gt) / n_eq, 0, 1).
``weights`` restates the documented rule (rato_saa.h; tests/_host_cuts.HostCutSolver._weights) in fp64.  Every pattern
comes with the (n_gt, n_eq, lambda, tail count per block) it is meant to produce and asserts them from ``weights`` when it is
built -- before anything is launched.  ``WRONG_RULES`` are the mistakes a kernel could make; tests/test_tail_patterns.py
checks that each of them moves the reference by >= 1000 x the tolerance tests/test_gpu_cut_tails.py applies.
Checker only: nothing in the package imports this."""
import functools
import math
from dataclasses import dataclass

import numpy as np

BLOCK, WAVE = 256, 64          # RATO_BLOCK, RATO_WAVE: samples per workgroup / per chunk of the compacted tail
EPS32 = 2.0 ** -24             # the tie weight lambda travels as a float: relative rounding of one fp32 conversion
EPS64 = 2.0 ** -53


def weights(m32, alpha, M):
    """-> (w (M,) fp64, t, n_gt, n_eq, lam): 1 above the threshold t = the ceil(alpha M)-th largest value, lam on ties"""
    m32 = np.asarray(m32, dtype=np.float32)
    assert m32.shape == (M,)
    aM = alpha * M
    rank = min(max(int(math.ceil(aM - 1e-12)), 1), M)
    t = np.sort(m32)[::-1][rank - 1]
    gt, eq = m32 > t, m32 == t
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    lam = min(max((aM - n_gt) / n_eq, 0.0), 1.0)
    return gt * 1.0 + eq * lam, float(t), n_gt, n_eq, lam


def block_counts(mask, M):
    """number of set samples per block of 256"""
    return np.bincount(np.flatnonzero(mask) // BLOCK, minlength=(M + BLOCK - 1) // BLOCK)


@dataclass
class Pattern:
    name: str
    cls: str            # pattern class (pack / ties / fractional / everything / lt1)
    m: np.ndarray       # (M,) fp32
    alpha: float
    M: int
    n_gt: int
    n_eq: int
    lam: float
    counts: tuple       # tail samples (weight != 0) per block of 256

    @property
    def alphaM(self):
        return self.alpha * self.M

    def weights(self):
        return weights(self.m, self.alpha, self.M)

    def check(self):
        w, t, n_gt, n_eq, lam = self.weights()
        assert (n_gt, n_eq) == (self.n_gt, self.n_eq), (self.name, n_gt, n_eq)
        assert abs(lam - self.lam) <= 1e-13, (self.name, lam, self.lam)
        assert tuple(block_counts(w != 0.0, self.M)) == tuple(self.counts), (self.name, block_counts(w != 0.0, self.M))
        return self


TIE_VALUE = 1.0


def _build(name, cls, M, alpha, gt_idx, eq_idx, lam, rng):
    """gt_idx: distinct values above the tie value; eq_idx: the tie value; every other sample a distinct value below.
    All values are multiples of 2^-10 (exact in fp32); their order is unrelated to the sample order."""
    gt_idx, eq_idx = np.asarray(gt_idx, dtype=np.int64), np.asarray(eq_idx, dtype=np.int64)
    assert np.intersect1d(gt_idx, eq_idx).size == 0 and np.unique(gt_idx).size == gt_idx.size
    m = np.empty(M, dtype=np.float32)
    low = np.setdiff1d(np.arange(M), np.concatenate([gt_idx, eq_idx]))
    m[low] = -1.0 - rng.permutation(low.size) / 1024.0
    m[eq_idx] = TIE_VALUE
    m[gt_idx] = 2.0 + rng.permutation(gt_idx.size) / 1024.0
    tail = np.zeros(M, bool)
    tail[gt_idx] = True
    if lam > 0.0:
        tail[eq_idx] = True
    return Pattern(name, cls, m, alpha, M, gt_idx.size, eq_idx.size, lam, tuple(block_counts(tail, M))).check()


PACK_N = (0, 1, 63, 64, 65, 128, 129, 192, 193, 255, 256)
PACK_N_SHORT = (0, 64, 65, 256)


def pack(n, M=600, alpha=0.5, seed=1):
    """the alpha M tail samples: the first n indices of block 0 plus the rest spread over blocks 1 and 2 (n = 0: block 0 has
    an empty tail; work_waves of block 0 = ceil(n / 64) = 0 .. 4).  No ties: the threshold is the last of the n."""
    rng = np.random.RandomState(seed + n)
    aM = int(round(alpha * M))
    assert alpha * M == aM and 0 <= n <= BLOCK and aM - n <= M - BLOCK
    rest = np.sort(rng.choice(np.arange(BLOCK, M), size=aM - n, replace=False))
    tail = np.concatenate([np.arange(n), rest])
    thr = n - 1 if n > 0 else 0
    p = _build(f"pack({n})", "pack", M, alpha, np.delete(tail, thr), tail[thr:thr + 1], 1.0, rng)
    assert p.counts[0] == n and all(c > 0 for c in p.counts[1:])
    return p


TIES = ((119, 1), (119, 2), (118, 3), (117, 4), (100, 500), (119, 481), (0, 600))


def ties(n_gt, n_eq, M=600, alpha=0.2, seed=2):
    rng = np.random.RandomState(seed + 7 * n_gt + n_eq)
    aM = alpha * M
    lam = (aM - n_gt) / n_eq
    if (n_gt, n_eq) == (118, 3):          # the tie group straddles the edge between blocks 0 and 1
        eq = np.array([255, 256, 257])
        gt = rng.choice(np.setdiff1d(np.arange(M), eq), size=n_gt, replace=False)
    elif (n_gt, n_eq) == (100, 500):      # block 0: one wave of samples above the threshold, then three waves of ties
        gt = np.concatenate([np.arange(WAVE), rng.choice(np.arange(BLOCK, M), size=n_gt - WAVE, replace=False)])
        eq = np.setdiff1d(np.arange(M), gt)
    else:
        perm = rng.permutation(M)
        gt, eq = perm[:n_gt], perm[n_gt:n_gt + n_eq]
    return _build(f"ties({n_gt},{n_eq})", "ties", M, alpha, gt, eq, lam, rng)


def fractional(which, M=513, alpha=0.2, seed=3):
    """alpha M = 102.6: 102 samples above the threshold, the threshold sample carries 0.6; the last block is sample 512 alone.
    'a': 70 tail samples in block 0 (two chunks), 33 in block 1, none in the last block;
    'b': sample 512 is above the threshold (the only tail sample of its block);  'c': sample 512 IS the threshold sample."""
    rng = np.random.RandomState(seed + ord(which))
    n_gt = int(math.floor(alpha * M))
    lam = alpha * M - n_gt
    if which == 'a':
        tail = np.concatenate([rng.choice(BLOCK, size=70, replace=False), BLOCK + rng.choice(BLOCK, size=n_gt + 1 - 70, replace=False)])
        gt, eq = tail[:-1], tail[-1:]
    elif which == 'b':
        body = rng.choice(M - 1, size=n_gt, replace=False)
        gt, eq = np.concatenate([body[:-1], [M - 1]]), body[-1:]
    else:
        gt, eq = rng.choice(M - 1, size=n_gt, replace=False), np.array([M - 1])
    return _build(f"fractional({which})", "fractional", M, alpha, gt, eq, lam, rng)


EVERYTHING_M = (256, 257, 600)


def everything(M, n_eq=1, seed=4):
    """alpha = 1: every weight is 1 (the threshold is min(m), n_eq samples share it); a full block is four chunks"""
    rng = np.random.RandomState(seed + M + n_eq)
    perm = rng.permutation(M)
    return _build(f"everything(M={M},n_eq={n_eq})", "everything", M, 1.0, perm[n_eq:], perm[:n_eq], 1.0, rng)


def less_than_one(where, M=600, seed=5):
    """alpha M = 0.5: the maximum alone carries the cut (lam = 0.5), or three tied maxima (lam = 1/6), one per block;
    ``where``: the block of the single maximum, or 'tied'"""
    rng = np.random.RandomState(seed)
    alpha = 0.5 / M
    if where == 'tied':
        eq = np.array([rng.randint(0, BLOCK), BLOCK + rng.randint(0, BLOCK), 2 * BLOCK + rng.randint(0, M - 2 * BLOCK)])
    else:
        lo, hi = where * BLOCK, min((where + 1) * BLOCK, M)
        eq = np.array([rng.randint(lo, hi)])
    return _build(f"less_than_one({where})", "lt1", M, alpha, np.zeros(0, int), eq, alpha * M / eq.size, rng)


def group(name, short=False):
    """-> list of rings [(M, alpha, [patterns])]: the patterns of one ring share M and alpha (ring slots of one launch)"""
    if name == "pack":
        return [(600, 0.5, [pack(n) for n in (PACK_N_SHORT if short else PACK_N)])]
    if name == "ties":
        return [(600, 0.2, [ties(a, b) for a, b in TIES])]
    if name == "fractional":
        return [(513, 0.2, [fractional(c) for c in "abc"])]
    if name == "everything":
        return [(M, 1.0, [everything(M, 1), everything(M, 3)]) for M in EVERYTHING_M]
    if name == "lt1":
        return [(600, 0.5 / 600, [less_than_one(w) for w in (0, 1, 2, 'tied')])]
    raise KeyError(name)


GROUPS = ("pack", "ties", "fractional", "everything", "lt1")


def arg_kinds(R):
    return ("uniform", "step0", "last", "sparse") + (tuple(f"group{r}" for r in range(R)) if R > 1 else ())


def args(kind, S, R, M, rng):
    """arg-max rows r * S + t of M samples (int32).  'uniform': random rows, as the existing tests use; 'step0': all at
    step 0 -- no control enters g_0, so every gradient column is exactly 0 and t_hi = 0; 'last': all at step S - 1;
    'sparse': one sample per 64 at S - 1, the others at 0 (t_hi comes from one lane); 'group<r>': random steps of row
    group r.  Where the kind does not fix it the row group cycles with the sample index."""
    i = np.arange(M)
    r = i % R
    if kind == "uniform":
        return rng.randint(0, R * S, size=M).astype(np.int32)
    if kind == "step0":
        t = np.zeros(M, int)
    elif kind == "last":
        t = np.full(M, S - 1)
    elif kind == "sparse":
        t = np.where(i % WAVE == 0, S - 1, 0)
    elif kind.startswith("group"):
        r = np.full(M, int(kind[5:]))
        assert r[0] < R
        t = rng.randint(0, S, size=M)
    else:
        raise KeyError(kind)
    return (r * S + t).astype(np.int32)


# ---- the reference sums -------------------------------------------------------------------------------------------
def cut_sums(Gc, g, w, arg, tie=None, lam=0.0):
    """Gc (M, R S, nw) the gradient columns the kernels emit, g (M, R S) the offsets -> dict:
    grad (nw,) = sum_i w_i Gc[i, arg_i], off = sum_i w_i g[i, arg_i], abs_off = sum_i w_i |g|, and the rounding of a
    float lambda: tie_grad (nw,) = 2^-24 lam sum_{ties} |entry|, tie_off likewise"""
    idx = np.arange(Gc.shape[0])
    rows, gv = Gc[idx, arg], g[idx, arg]
    out = {"grad": (w[:, None] * rows).sum(axis=0), "off": float(w @ gv), "abs_off": float(w @ np.abs(gv)),
           "abs_grad": (w[:, None] * np.abs(rows)).sum(axis=0), "n": int((w != 0).sum())}
    if tie is None:
        tie = np.zeros(Gc.shape[0], bool)
    dl = float_lambda_error(lam)
    out["tie_grad"] = dl * np.abs(rows[tie]).sum(axis=0)
    out["tie_off"] = dl * float(np.abs(gv[tie]).sum())
    return out


def float_lambda_error(lam):
    """|float(lam) - lam| <= 2^-24 lam: what carrying the tie weight as a float costs (0 for 1, 1/2, 3/4, ...)"""
    dl = abs(float(np.float32(lam)) - lam)
    assert dl <= EPS32 * lam
    return dl


def rollout_tolerance(ref, tie_term=True):
    """the bounds the rollout kernels already have against the fp64 oracle (tests/test_gpu_scp.py) + the float lambda:
    gradient: rtol 1e-7, atol 1e-8 max(1, max |grad|);  offset: 1e-8 (w . |g| + 1)"""
    k = 1.0 if tie_term else 0.0
    tol_grad = 1e-7 * np.abs(ref["grad"]) + 1e-8 * max(1.0, np.abs(ref["grad"]).max(initial=0.0)) + k * ref["tie_grad"]
    tol_off = 1e-8 * (ref["abs_off"] + 1.0) + k * ref["tie_off"]
    return tol_grad, tol_off


def table_tolerance(ref):
    """fp64 sums over the same fp32 table entries: only the order of N additions and the float lambda are left"""
    n = max(ref["n"], 1)
    return 4 * n * EPS64 * ref["abs_grad"] + ref["tie_grad"], 4 * n * EPS64 * ref["abs_off"] + ref["tie_off"]


# ---- the mistakes a kernel could make ------------------------------------------------------------------------------
def _rule(p, lam=None):
    w, t, n_gt, n_eq, l = p.weights()
    gt, eq = p.m > np.float32(t), p.m == np.float32(t)
    return gt * 1.0 + eq * (l if lam is None else lam)


def _first_wave_only(p):
    w = _rule(p)
    out = np.zeros_like(w)
    for b in range(0, p.M, BLOCK):
        nz = b + np.flatnonzero(w[b:b + BLOCK])[:WAVE]
        out[nz] = w[nz]
    return out


def _no_last_block(p):
    w = _rule(p).copy()
    w[(p.M - 1) // BLOCK * BLOCK:] = 0.0
    return w


# name -> (weights of the wrong rule, arg rows of the wrong rule)
WRONG_RULES = {
    "lam=1 on ties": lambda p, arg, S: (_rule(p, 1.0), arg),
    "lam=0 on ties": lambda p, arg, S: (_rule(p, 0.0), arg),
    ">= in place of >": lambda p, arg, S: ((p.m >= np.float32(p.weights()[1])) * 1.0, arg),
    "tail beyond the first 64 of a block dropped": lambda p, arg, S: (_first_wave_only(p), arg),
    "last block dropped": lambda p, arg, S: (_no_last_block(p), arg),
    "row group forced to 0": lambda p, arg, S: (_rule(p), arg % S),
}


# ---- the fp64 oracle's dense rows on fp32-rounded samples ----------------------------------------------------------
def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def graze(S):
    t = np.arange(S)[:, None]
    return np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)


def driving_uk(S):
    t = np.arange(S)[:, None]
    return np.hstack([0.4 * np.cos(0.3 * t) + 0.1, 0.03 * np.sin(0.5 * t) + 0.004]) * (20.0 / S)


@functools.lru_cache(maxsize=1)
def drone_rows(S, M=600, seed=0):
    """-> dict: samples (DWs, masses, Q rounded to fp32: both legs see the same numbers), uk, Gc (M, 3 S, 2 (S - 1)), g (M, 3 S)"""
    from oracle import drone as od
    DWs, masses, Q = [_r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(seed), 'saa', M=M, S=S)]
    o = od.Model(S, DWs, masses, Q, 'saa', 0.2)
    uk = graze(S)
    _, _, _, gdu, gup = o.get_all_constraints_coeffs(uk)
    G = gdu.reshape(M, 3 * S, 3 * S)
    g = -(gup.reshape(M, 3 * S) - G @ uk.reshape(-1))
    G4 = G.reshape(M, 3 * S, S, 3)
    assert np.all(G4[:, :, S - 1] == 0.0) and np.all(G4[:, :, :, 2] == 0.0)     # what the kernels do not emit is zero
    return {"samples": (DWs, masses, Q), "uk": uk, "Gc": np.ascontiguousarray(G4[:, :, :S - 1, :2]).reshape(M, 3 * S, -1), "g": g}


@functools.lru_cache(maxsize=1)
def driving_rows(S, M=600, seed=0):
    """-> dict: samples (fp32-rounded), uk, Gc (M, S, 2 (S - 1)), g (M, S)"""
    from oracle import driving as ocar
    samples = [_r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(seed), M, 'saa', S)]
    o = ocar.Model(*samples, method='saa', alpha=0.2)
    uk = driving_uk(S)
    _, _, _, gdu, gup = o.get_all_constraints_coeffs(uk)
    G = gdu.reshape(M, S, 2 * S)
    g = -(gup.reshape(M, S) - G @ uk.reshape(-1))
    G4 = G.reshape(M, S, S, 2)
    assert np.all(G4[:, :, S - 1] == 0.0)                                        # u_{S-1} enters no row
    return {"samples": samples, "uk": uk, "Gc": np.ascontiguousarray(G4[:, :, :S - 1]).reshape(M, S, -1), "g": g}

"""Per-workgroup checker of the hopper slip kernel's Hessian partials (part_hess of rato_hopper_slip /
rato_hopper_slip_hessian): pure NumPy, no GPU.

The totals the existing tests compare (sum over all M samples) cannot see one sample once M is large: one sample's
share of D2 at M = 5e4 is ~1e-2, below the tolerance of the total.  Each workgroup's partial is a sum over at most 256
samples, and is compared here against an fp64 sum over exactly the samples that workgroup owns, with a limit derived
from the arithmetic and checked (``sensitivity``) to stay below the median |term| of that workgroup: a dropped,
duplicated or mis-indexed sample, a transposed or shifted lambda, a NaN or a zero partial all fail, with the workgroup
and the contact named.

Slots of part[b][c][:] (hopper.hip): 0 = D1 = sum lam d2h/(dpx dfz) = -sum lam mu',  1 = D2 = sum lam d2h/dpx^2 =
-sum lam fz mu'',  2 (HC = 3 only) = D0 = sum lam dh/dpx.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import hopper as oh

WAVE, BLOCK = 64, 256
U = 2.0 ** -24                      # fp32 unit roundoff
# Accumulation bound of one partial, |part - sum t_i| <= GAMMA * sum |t_i| + TINY, for terms t_i built from the device's
# own per-sample values (D0, D1).  The device forms each term in fp32 and sums:
#   terms   D1: fl(lam s1) against lam fl(s1 fz) / fz -> 2 roundings;  D0: fl(fl(lam s1) fz) against lam fl(s1 fz) -> 3
#   wave    rato::wave_sum_dpp: row_shr 1, 2, 4, 8, row_bcast 15, 31 -- every sample passes through 6 fp32 additions,
#           each off by <= u times a partial sum that is itself <= sum |t_i|
#   fold    the SW <= 4 sample-waves of the workgroup, added in a fixed order from 0: <= 3 more roundings
#   store   the fold's fp32 result is stored as is (exact)
# -> 12 u to first order; 16 u leaves room for the second-order terms (12 u)^2 and the clamped lanes' exact zeros.
GAMMA = 16 * U
TINY = 1e-30
# Effective per-term error of the kernel's trig path, eps in |mu_dev - mu| <= eps sum_k |a_k| (hardware v_cos_f32 on the
# phase in revolutions, the fp32 phase FMA and the 30-term fp32 sum included), on the device's own fp32 inputs: measured
# 2.5e-7 on MI355X over 2e5 samples x 40 contacts (tests/test_gpu_hopper_shapes.py reports it under RATO_TOL_REPORT=1); 3x.
EPS_TRIG = 7.5e-7
SLOTS = ("D1", "D2", "D0")


class Blocks:
    """Sample ranges [lo[b], hi[b]) of the workgroups of one launch."""

    def __init__(self, M, spw, nblocks):
        self.M, self.spw, self.nblocks = M, spw, nblocks
        self.lo = np.arange(nblocks, dtype=np.int64) * spw
        self.hi = np.minimum(self.lo + spw, M)

    def __repr__(self):
        return f"Blocks(M={self.M}, {self.spw} samples x {self.nblocks} workgroups)"


def default_nw_log2(M):
    """hopper_nw_log2 of hopper.hip restated: 4 contact-waves per sample-wave while ceil(M / 64) < 1536, then 2."""
    return 2 if (M + WAVE - 1) // WAVE < 1536 else 1


def block_of(M, nblocks, nw_log2=None):
    """The workgroups' sample ranges for a launch over M samples.  ``nblocks``: rato_hopper_nblocks(M) as the library
    answered it (or part.shape[0], which was sized by it); ``nw_log2``: the launch shape in force (RATO_HOPPER_NW_LOG2),
    default the library's own rule.  A workgroup is 4 waves = (4 >> nw_log2) sample-waves of 64 samples: 64, 128 or
    256 samples per workgroup."""
    nw_log2 = default_nw_log2(M) if nw_log2 is None else int(nw_log2)
    assert nw_log2 in (0, 1, 2), nw_log2
    spw = BLOCK >> nw_log2
    expect = (M + spw - 1) // spw
    assert int(nblocks) == expect, (f"rato_hopper_nblocks({M}) = {nblocks}, but {spw} samples per workgroup "
                                    f"(nw_log2 = {nw_log2}) make {expect} workgroups")
    return Blocks(M, spw, expect)


def _workers():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(8, n))


class SampleTerms:
    """Per-sample fp64 terms of the three partial slots, layout [C][M] like the device arrays, plus the oracle's mu,
    mu', mu'' at the same inputs and what the per-term trig bound of D2 needs.  The oracle runs in sample chunks
    (2e5 samples x 40 contacts x 30 features do not fit one temporary), chunks on a few threads."""

    def __init__(self, lam, px, fx, fz, fields, dh_dpx=None, chunk_elems=1 << 21):
        lam = np.asarray(lam, dtype=np.float64)
        C, M = lam.shape
        px, fx, fz = (np.asarray(v, dtype=np.float64).reshape(C) for v in (px, fx, fz))
        a, th, tau = (np.asarray(f, dtype=np.float64) for f in fields)
        assert a.shape == th.shape == tau.shape and a.shape[0] == M, (a.shape, M)
        self.C, self.M, self.px, self.fx, self.fz, self.lam = C, M, px, fx, fz, lam
        self.mu, self.dmu, self.d2mu = (np.empty((C, M)) for _ in range(3))
        self.w2 = np.empty((C, M))                      # |lam fz| sum_k |a_k| theta_k^2: D2's per-term trig weight
        self.sum_a = np.abs(a).sum(axis=1)              # (M,): mu's per-term trig weight
        step = max(1, chunk_elems // (C * a.shape[1]))

        def work(s):
            e = min(s + step, M)
            mu, dmu, d2mu = oh.friction_derivatives(px, a[s:e], th[s:e], tau[s:e])      # (n, C) each
            self.mu[:, s:e], self.dmu[:, s:e], self.d2mu[:, s:e] = mu.T, dmu.T, d2mu.T
            self.w2[:, s:e] = (np.abs(a[s:e]) * th[s:e] ** 2).sum(axis=1)[None, :]
        with ThreadPoolExecutor(_workers()) as ex:
            list(ex.map(work, range(0, M, step)))
        self.w2 *= np.abs(lam * fz[:, None])
        self.t2 = -lam * fz[:, None] * self.d2mu                                 # D2 terms: the fp64 oracle
        self.set_device_dh_dpx(dh_dpx)

    def head(self, M):
        """the terms of the first M samples (views): the per-sample values do not depend on the batch size"""
        t = object.__new__(SampleTerms)
        t.__dict__.update(self.__dict__)
        t.M, t.lam, t.sum_a = M, self.lam[:, :M], self.sum_a[:M]
        for k in ("mu", "dmu", "d2mu", "w2", "t2", "t1", "t0"):
            setattr(t, k, getattr(self, k)[:, :M])
        return t

    def set_device_dh_dpx(self, dh_dpx):
        """D1 / D0 terms from the device's own fp32 dh/dpx ([C][M]): lam dh_dpx / fz and lam dh_dpx.  Without it (CPU
        tests) from the oracle's, rounded to fp32 as the device would store it."""
        if dh_dpx is None:
            dh_dpx = (-self.dmu * self.fz[:, None]).astype(np.float32)
        d = np.asarray(dh_dpx, dtype=np.float64)
        assert d.shape == (self.C, self.M), d.shape
        self.t0 = self.lam * d
        self.t1 = self.t0 / self.fz[:, None]

    def h(self):
        return self.fx[:, None] - self.mu * self.fz[:, None]

    def dh_dfz(self):
        return -self.mu

    def dh_dpx(self):
        return -self.dmu * self.fz[:, None]

    def trig_eps(self, dh_dfz_dev):
        """The trig path's measured effective per-term error: max over (sample, contact) of |mu_dev - mu| / sum_k |a_k|,
        mu_dev = -dh_dfz of the device."""
        err = np.abs(-np.asarray(dh_dfz_dev, dtype=np.float64) - self.mu)
        return float(np.max(err / np.maximum(self.sum_a[None, :], 1e-300)))


def _block_reduce(x, blocks):
    """(C, M) -> (nblocks, C) sums over each workgroup's samples"""
    return np.add.reduceat(x, blocks.lo, axis=1).T


def _block_median_abs(x, blocks):
    """(C, M) -> (nblocks, C) median |x| over each workgroup's samples"""
    C, M = x.shape
    out = np.empty((blocks.nblocks, C))
    nfull = M // blocks.spw
    ax = np.abs(x)
    if nfull:
        out[:nfull] = np.median(ax[:, :nfull * blocks.spw].reshape(C, nfull, blocks.spw), axis=2).T
    if nfull < blocks.nblocks:
        out[nfull] = np.median(ax[:, nfull * blocks.spw:], axis=1)
    return out


def references(terms, blocks, hc, eps_trig=EPS_TRIG):
    """-> [(name, ref (nb, C), limit (nb, C), median |term| (nb, C))] per slot of part[b][c][:hc]"""
    assert blocks.M == terms.M
    out = []
    for slot in range(hc):
        t = (terms.t1, terms.t2, terms.t0)[slot]
        lim = GAMMA * _block_reduce(np.abs(t), blocks) + TINY
        if slot == 1:
            lim = lim + eps_trig * _block_reduce(terms.w2, blocks)
        out.append((SLOTS[slot], _block_reduce(t, blocks), lim, _block_median_abs(t, blocks)))
    return out


def check_partials(part, terms, blocks, what="part_hess", eps_trig=EPS_TRIG, sensitivity=True):
    """part: (nblocks, C, HC) fp32 per-workgroup partials.  Asserts every one within its limit of the fp64 reference
    over the samples its workgroup owns, and (sensitivity) that every limit is below the median |term| of its
    workgroup.  -> {slot: max |part - ref| / limit} for the report."""
    part = np.asarray(part)
    nb, C, hc = part.shape
    assert (nb, C) == (blocks.nblocks, terms.C), (part.shape, blocks, terms.C)
    worst = {}
    for slot, (name, ref, lim, med) in enumerate(references(terms, blocks, hc, eps_trig)):
        p = part[:, :, slot].astype(np.float64)
        err = np.abs(p - ref)
        bad = ~(err <= lim)                         # NaN fails
        if bad.any():
            b, c = np.argwhere(bad)[0]
            raise AssertionError(
                f"{what} {name}: {int(bad.sum())} of {bad.size} partials off; first: workgroup {b} (samples "
                f"{blocks.lo[b]}..{blocks.hi[b] - 1}), contact {c}: part {p[b, c]!r}, reference {ref[b, c]!r}, "
                f"|err| {err[b, c]:.3e} > limit {lim[b, c]:.3e}")
        if sensitivity:
            blind = ~(lim < med)
            if blind.any():
                b, c = np.argwhere(blind)[0]
                raise AssertionError(
                    f"{what} {name}: the limit cannot see one sample: workgroup {b}, contact {c}: limit "
                    f"{lim[b, c]:.3e} >= median |term| {med[b, c]:.3e}")
        worst[name] = float(np.max(err / lim))
    return worst

"""GPU: the grid Cholesky (csrc/chol_grid.hip) OFF the co-resident schedule.

The in-place hazard rule of the kernel -- no workgroup reads an entry another workgroup of its launch writes -- cannot be
seen to fail on a free chip: a launch at n = 400 is at most 27 workgroups per problem, all of them resident at once, all of
them load at the top and store at the end, so a workgroup that read what a neighbour writes would still read the old value.
Here the factorization meets the chip as the solver does beside other streams: busy.  L and X must be bitwise those of a free
chip and those of the workgroup kernels, and within Higham's elementwise bounds (Thm 10.3 / 10.4).

The crowd (DESIGN §7.ak has the measurements).  ``rato_device_occupy`` holds HOG_BLOCKS of the 512 1024-lane blocks that fill
the chip's wave slots, for 0.3 s.  A hog alone cannot give a schedule with a few free slots: workgroups are dealt to the parts
of the chip in a fixed rotation, and one that is dealt to a part without room waits there, with every workgroup behind it, until
the hog ends, however much room there is elsewhere.  Measured, above 480 held blocks some launch of the factorization ends with
the hog, not beside it, and at 480 and below it is not slowed at all (what the hog leaves holds the 81 workgroups of the largest
launch here).  So 480 blocks are held for good, and what is left is held in PULSES: on PULSE_STREAMS more streams,
PULSE_LAUNCHES launches one behind the other of PULSE_BLOCKS blocks for PULSE_US microseconds each.  A workgroup of the launch
under test that is dealt to a part a pulse holds waits for that pulse to end, and so do the workgroups behind it, while those
dealt before it have run, and stored: one launch's workgroups run at different times, which is what the rule is about.  Events
behind the hog and behind every pulse stream must still be pending when the factorizations and solves under test have ended: they
ran in the crowd, not after it.  Two streams of a process can share a hardware queue; the run then waits for its neighbour to
end and shows nothing, so up to ATTEMPTS crowds are made, on fresh streams, until one outlasted the run -- and the results of
every attempt, crowded or not, are held to the same bits.  The test bites: with row block 0's store of the factored diagonal
block sent straight into A as well (a change of values only), three of these four cases fail, on pivots that fail, while
test_grid_cholesky_and_solve_at_the_workloads_sizes passes."""
import time

import numpy as np
import pytest

from _hopper_ipm import gamma
from test_gpu_chol_grid import chol, lower, padded, same, spd, untouched

pytestmark = pytest.mark.gpu
LD = np.longdouble
HOG_BLOCKS = 480                                                      # of 512: the most beside which every launch still runs
HOG_US = 300000                                                       # the factorization is milliseconds even serialized tenfold
PULSE_STREAMS, PULSE_LAUNCHES, PULSE_BLOCKS, PULSE_US = 2, 150, 24, 100
REPEATS = 3
ATTEMPTS = 3
K, PAD, NRHS = 3, 3, 3


def factor_and_solve(A0, bh, crowd=False):
    """REPEATS times ``chol_factor`` and ``chol_solve`` (method='grid') of fresh copies on a stream of their own; ``crowd``: beside
    the hog and the pulses, each on a stream of its own -> the Ls, the Xs, the infos, the first factorization's milliseconds
    (events on its stream), and per member of the crowd (the hog first) whether it had ended when the last solve had"""
    import torch
    from riskaversetrajopt_amd import _lib
    m = chol()
    n = A0.shape[1]
    Ls = [A0.clone() for _ in range(REPEATS)]
    Xs = [torch.as_tensor(bh, device=A0.device) for _ in range(REPEATS)]
    work = m.chol_grid_work(n, K, A0.device)
    run = torch.cuda.Stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    behind, infos = [], []
    if crowd:
        hog, pulses = torch.cuda.Stream(), [torch.cuda.Stream() for _ in range(PULSE_STREAMS)]
    torch.cuda.synchronize()
    if crowd:
        lib = _lib.load()
        with torch.cuda.stream(hog):
            _lib.check(lib.rato_device_occupy(HOG_BLOCKS, HOG_US, _lib.current_stream()), "rato_device_occupy")
            behind.append(torch.cuda.Event())
            behind[-1].record()
        time.sleep(0.02)                                              # the hog is resident before anything else is queued
        for s in pulses:
            with torch.cuda.stream(s):
                for _ in range(PULSE_LAUNCHES):
                    _lib.check(lib.rato_device_occupy(PULSE_BLOCKS, PULSE_US, _lib.current_stream()), "rato_device_occupy")
                behind.append(torch.cuda.Event())
                behind[-1].record()
    with torch.cuda.stream(run):
        for i, (L, X) in enumerate(zip(Ls, Xs)):
            if i == 0:
                t0.record()
            infos.append(m.chol_factor(L, method='grid', work=work))
            if i == 0:
                t1.record()
            m.chol_solve(L, X, method='grid')
    run.synchronize()
    ended = [e.query() for e in behind]                               # all False: the whole crowd outlasted the last launch
    torch.cuda.synchronize()                                          # the crowd ends
    return Ls, Xs, [info.cpu().tolist() for info in infos], t0.elapsed_time(t1), ended


@pytest.mark.parametrize("kind", ["bbt", "graded"])
@pytest.mark.parametrize("n", [130, 400])
def test_grid_cholesky_and_solve_on_a_crowded_chip(n, kind):
    import torch
    m = chol()
    As = [spd(kind, n, 10 * n + k) for k in range(K)]                 # three distinct problems
    A0 = padded(As, n + PAD)
    bh = np.full((K, NRHS, n + 2), np.nan)
    bh[:, :, :n] = np.random.RandomState(n).uniform(-1, 1, (K, NRHS, n))
    factor_and_solve(A0, bh)                                          # warm: the kernels are loaded
    Lfs, Xfs, info_f, ms_free, _ = factor_and_solve(A0, bh)
    Lw, Xw = A0.clone(), torch.as_tensor(bh, device=A0.device)
    assert m.chol_factor(Lw, method='workgroup').cpu().tolist() == [0] * K
    m.chol_solve(Lw, Xw, method='workgroup')
    assert info_f == [[0] * K] * REPEATS and all(same(L, Lw) for L in Lfs) and all(same(X, Xw) for X in Xfs)
    for attempt in range(ATTEMPTS):
        Lcs, Xcs, info_c, ms_crowded, ended = factor_and_solve(A0, bh, crowd=True)
        print(f"n={n} K={K} {kind}: grid factorization {ms_free:.3f} ms on a free chip, {ms_crowded:.3f} ms (x {ms_crowded / ms_free:.1f}) "
              f"beside {HOG_BLOCKS} of 512 held blocks and the pulses; ended before it (hog, pulses): {ended}")
        assert info_c == [[0] * K] * REPEATS
        for Lc, Xc in zip(Lcs, Xcs):                                  # bitwise the free chip's, which are the workgroup kernels'
            assert same(Lc, Lw) and same(Xc, Xw)
            assert untouched(Lc, n)
        if not any(ended):
            break
    assert not any(ended), "no factorization and solve ended while the hog and the pulses were running: nothing was tested"
    Lc, Xc = Lcs[-1], Xcs[-1]
    Lh, xh = Lc.cpu().numpy(), Xc.cpu().numpy()
    assert np.all(np.isnan(xh[:, :, n:]))
    for k in range(K):
        Lk = lower(Lh[k], n)
        LL = np.abs(Lk) @ np.abs(Lk).T
        err = np.abs(Lk.astype(LD) @ Lk.T.astype(LD) - As[k].astype(LD))
        assert np.all(err <= gamma(n + 1) * LL.astype(LD)), (k, float(err.max()))
        for j in range(NRHS):
            x = xh[k, j, :n]
            res = np.abs(bh[k, j, :n].astype(LD) - As[k].astype(LD) @ x.astype(LD))
            assert np.all(res <= gamma(3 * n + 1) * (LL @ np.abs(x)).astype(LD)), (k, j, float(res.max()))

"""CPU: the per-workgroup checker of the hopper Hessian partials (tests/_hopper_check.py) accepts partials built from the
fp64 oracle and rounded to fp32 as the device stores them, and rejects each way a workgroup can lose, repeat or
mis-weight a sample -- naming the workgroup and the contact."""
import numpy as np
import pytest

from oracle import hopper as oh
from tests import _hopper_check as hc

M, C = 300, 257
FAIL = r"workgroup \d+ \(samples \d+\.\.\d+\), contact \d+"


@pytest.fixture(scope="module")
def terms():
    rng = np.random.RandomState(11)
    fields = tuple(f.astype(np.float32) for f in oh.sample_friction_fields(np.random.RandomState(1), M))
    px = np.linspace(-3.0, 3.0, C).astype(np.float32)
    fz = (32.0 + rng.randn(C)).astype(np.float32)
    fx = (0.08 * fz + 0.3 * rng.randn(C)).astype(np.float32)
    lam = rng.uniform(0.5, 1.0, (C, M)).astype(np.float32)
    t = hc.SampleTerms(lam, px, fx, fz, fields)
    t.fields = fields
    return t


def device_like(terms, blocks, nslots, t=None):
    """fp32 per-workgroup partials as an exact kernel would store them: fp64 sums of the terms, rounded once"""
    t = (terms.t1, terms.t2, terms.t0) if t is None else t
    return np.stack([np.add.reduceat(t[s], blocks.lo, axis=1).T for s in range(nslots)], axis=2).astype(np.float32)


def blocks_for(nw_log2):
    spw = 256 >> nw_log2
    return hc.block_of(M, (M + spw - 1) // spw, nw_log2=nw_log2)


SHAPES = [(2, 2), (1, 2), (0, 2), (2, 3), (1, 3)]     # (nw_log2, HC): 64, 128, 256 samples per workgroup


def test_block_mapping_follows_the_library():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    for m, nb, spw in ((1, 1, 64), (300, 5, 64), (98239, 1535, 64), (98240, 1535, 64), (98241, 768, 128),
                       (196672, 1537, 128), (200003, 1563, 128)):
        assert lib.rato_hopper_nblocks(m) == nb, m
        b = hc.block_of(m, lib.rato_hopper_nblocks(m))
        assert b.spw == spw and b.nblocks == nb and b.hi[-1] == m and np.all(b.hi > b.lo)
        assert np.array_equal(b.lo[1:], b.hi[:-1])
    with pytest.raises(AssertionError, match="rato_hopper_nblocks"):
        hc.block_of(98241, 1536)                         # 64 samples per workgroup where the library takes 128
    assert hc.block_of(98241, 384, nw_log2=0).spw == 256


@pytest.mark.parametrize("nw_log2,nslots", SHAPES)
def test_exact_partials_pass(terms, nw_log2, nslots):
    b = blocks_for(nw_log2)
    worst = hc.check_partials(device_like(terms, b, nslots), terms, b)
    assert set(worst) == set(hc.SLOTS[:nslots]) and max(worst.values()) <= 1.0


@pytest.mark.parametrize("nw_log2,nslots", SHAPES)
def test_dropped_sample_is_rejected(terms, nw_log2, nslots):
    b = blocks_for(nw_log2)
    part = device_like(terms, b, nslots)
    i = b.lo[1] + 17                                       # one sample of workgroup 1, all contacts
    for s in range(nslots):
        part[1, :, s] = (part[1, :, s] - (terms.t1, terms.t2, terms.t0)[s][:, i]).astype(np.float32)
    with pytest.raises(AssertionError, match=r"workgroup 1 \(samples \d+\.\.\d+\), contact \d+"):
        hc.check_partials(part, terms, b)


@pytest.mark.parametrize("nw_log2,nslots", SHAPES)
def test_clamped_lanes_repeating_the_last_sample_are_rejected(terms, nw_log2, nslots):
    """lam read without ``valid``: every clamped lane of the last workgroup adds the last sample's term once more"""
    b = blocks_for(nw_log2)
    clamped = b.nblocks * b.spw - M
    assert clamped > 0
    part = device_like(terms, b, nslots)
    for s in range(nslots):
        part[-1, :, s] = (part[-1, :, s] + clamped * (terms.t1, terms.t2, terms.t0)[s][:, M - 1]).astype(np.float32)
    with pytest.raises(AssertionError, match=r"workgroup %d \(samples \d+\.\.299\), contact \d+" % (b.nblocks - 1)):
        hc.check_partials(part, terms, b)


@pytest.mark.parametrize("nw_log2,nslots", SHAPES)
@pytest.mark.parametrize("how", ["transposed", "next_sample", "previous_sample"])
def test_misindexed_lambda_is_rejected(terms, nw_log2, nslots, how):
    b = blocks_for(nw_log2)
    lam = terms.lam
    if how == "transposed":                                # lam[m * C + c] read for lam[c * M + m]
        wrong = lam.reshape(-1).reshape(M, C).T
    elif how == "next_sample":
        wrong = lam[:, np.minimum(np.arange(M) + 1, M - 1)]
    else:
        wrong = lam[:, np.maximum(np.arange(M) - 1, 0)]
    t = tuple(x * (wrong / lam) for x in (terms.t1, terms.t2, terms.t0))
    with pytest.raises(AssertionError, match=FAIL):
        hc.check_partials(device_like(terms, b, nslots, t), terms, b)


@pytest.mark.parametrize("nw_log2,nslots", SHAPES)
@pytest.mark.parametrize("value", [np.nan, 0.0])
def test_nan_or_zero_workgroup_is_rejected(terms, nw_log2, nslots, value):
    b = blocks_for(nw_log2)
    part = device_like(terms, b, nslots)
    wg = b.nblocks // 2
    part[wg] = value
    with pytest.raises(AssertionError, match=r"workgroup %d \(samples \d+\.\.\d+\), contact 0" % wg):
        hc.check_partials(part, terms, b)
    part = device_like(terms, b, nslots)
    part[wg, 100, nslots - 1] = value                       # one contact, last slot only
    with pytest.raises(AssertionError, match=r"%s: 1 of \d+ partials off; first: workgroup %d \(samples \d+\.\.\d+\), "
                                             r"contact 100" % (hc.SLOTS[nslots - 1], wg)):
        hc.check_partials(part, terms, b)


def test_limit_that_cannot_see_one_sample_fails_loudly(terms):
    """an eps_trig so large that D2's limit exceeds the median |term| of a workgroup: the checker refuses to pass"""
    b = blocks_for(2)
    part = device_like(terms, b, 2)
    with pytest.raises(AssertionError, match=r"D2: the limit cannot see one sample: workgroup \d+, contact \d+"):
        hc.check_partials(part, terms, b, eps_trig=1e-2)


def test_terms_match_the_oracle_sums(terms):
    """the checker's terms summed over all samples are the oracle's D1 / D2 totals (Model.slip_hessian_sums)"""
    o = oh.Model(*terms.fields, method='saa')
    forces = np.stack([terms.fx, terms.fz], axis=1)
    D1_o, D2_o = o.slip_hessian_sums(terms.px, forces, terms.lam.T)
    np.testing.assert_allclose(terms.t2.sum(axis=1), D2_o, rtol=1e-12, atol=1e-12)
    # D1's terms come from dh/dpx rounded to fp32: one rounding per term
    assert np.all(np.abs(terms.t1.sum(axis=1) - D1_o) <= hc.U * np.abs(terms.t1).sum(axis=1) + 1e-15)
    h_o, dfz_o, dpx_o = o.slip_partials(terms.px, forces)
    np.testing.assert_allclose(terms.h(), h_o.T, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(terms.dh_dpx(), dpx_o.T, rtol=1e-14, atol=1e-14)

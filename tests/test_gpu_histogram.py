"""GPU: rato_histogram against its float32 bin rule restated in NumPy (tests/_euclid.py), count for count."""
import numpy as np
import pytest

from tests import _euclid as E

pytestmark = pytest.mark.gpu
M_CASES = (1, 255, 256, 257, 100003)
BIN_CASES = (1, 7, 64, 4096)
LO, HI = -0.6, 0.4                         # the main figure's axis (drone_main_plot.py:750)


def device_counts(z, lo, hi, bins, out=None):
    import torch
    from riskaversetrajopt_amd import stats
    Z = torch.as_tensor(np.asarray(z, dtype=np.float32), device='cuda:0')
    c = stats.histogram_device(Z, lo, hi, bins, out=out)
    torch.cuda.synchronize()
    return c.cpu().numpy().view(np.uint32).astype(np.int64)


def edge_values(lo, hi, bins):
    """values exactly at lo, hi, nextafter(hi, -inf), every interior edge (as float32 sees it, and its two neighbours),
    +-inf and NaN"""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    edges = (lo32 + np.arange(1, bins, dtype=np.float32) * ((hi32 - lo32) / np.float32(bins))).astype(np.float32)
    ninf, pinf = np.float32(-np.inf), np.float32(np.inf)
    return np.concatenate([[lo32, hi32, np.nextafter(hi32, ninf), np.nextafter(lo32, ninf), np.nextafter(lo32, pinf), pinf, ninf,
                            np.float32(np.nan), np.float32(0.0), np.float32(-0.0)],
                           edges, np.nextafter(edges, ninf), np.nextafter(edges, pinf)]).astype(np.float32)


def values(M, lo, hi, bins, seed):
    """M values: the edge set first (as much of it as fits), then draws across and beyond the range"""
    rng = np.random.RandomState(seed)
    z = (lo - 0.1 + (hi - lo + 0.2) * rng.rand(M)).astype(np.float32)
    e = edge_values(lo, hi, bins)[:M]
    z[:e.size] = e
    return z


@pytest.mark.parametrize("bins", BIN_CASES)
@pytest.mark.parametrize("M", M_CASES)
def test_counts_equal_the_float32_rule(M, bins):
    z = values(M, LO, HI, bins, seed=M + bins)
    got = device_counts(z, LO, HI, bins)
    assert got.shape == (bins + 3,) and got.sum() == M
    assert np.array_equal(got, E.histogram(z, LO, HI, bins))


@pytest.mark.parametrize("bins", BIN_CASES)
def test_every_edge_value_lands_where_the_rule_puts_it(bins):
    z = edge_values(LO, HI, bins)                          # (3 bins + 7 values: all of them, also at bins = 4096)
    got = device_counts(z, LO, HI, bins)
    assert np.array_equal(got, E.histogram(z, LO, HI, bins)) and got.sum() == z.size
    assert got[bins + 2] == 1 and got[0] == 2 and got[bins + 1] == 2          # NaN | nextafter(lo, -inf), -inf | hi, +inf
    for lo, hi in ((0.0, 1.0), (-3.0, 5.0), (1e-3, 1e-3 + 1e-6), (-1e30, 1e30)):
        z = edge_values(lo, hi, bins)
        assert np.array_equal(device_counts(z, lo, hi, bins), E.histogram(z, lo, hi, bins)), (lo, hi)


@pytest.mark.parametrize("M", M_CASES)
def test_all_equal_values_fill_one_bin(M):
    for bins in (1, 64, 4096):
        for v in (0.123, LO, np.nan, 7.0):
            got = device_counts(np.full(M, v, dtype=np.float32), LO, HI, bins)
            want = E.histogram(np.full(M, v, dtype=np.float32), LO, HI, bins)
            assert np.array_equal(got, want) and got.max() == M and got.sum() == M


def test_a_million_clustered_values():
    """the normal case: the maxima of a validation batch sit in a few bins"""
    rng = np.random.RandomState(7)
    M = 1000000
    z = np.where(rng.rand(M) < 0.9, -0.12 + 0.004 * rng.randn(M), -0.3 + 0.2 * rng.randn(M)).astype(np.float32)
    for bins in (100, 4096):
        got = device_counts(z, LO, HI, bins)
        assert np.array_equal(got, E.histogram(z, LO, HI, bins)) and got.sum() == M


def test_a_poisoned_count_buffer_does_not_matter():
    import torch
    z = values(100003, LO, HI, 64, seed=3)
    want = E.histogram(z, LO, HI, 64)
    out = torch.full((64 + 3,), float("nan"), dtype=torch.float32, device='cuda:0').view(torch.int32)
    assert np.array_equal(device_counts(z, LO, HI, 64, out=out), want)
    assert np.array_equal(device_counts(z, LO, HI, 64, out=out), want)          # the first call's counts do not linger
    out.view(torch.uint8).fill_(0x7f)
    assert np.array_equal(device_counts(z, LO, HI, 64, out=out), want)
    assert np.array_equal(device_counts(z, LO, HI, 64, out=out), want)


def test_host_form_returns_the_edges():
    from riskaversetrajopt_amd import stats
    z = values(257, LO, HI, 7, seed=1)
    counts, edges = stats.histogram(z, LO, HI, 7)
    assert np.array_equal(counts, E.histogram(z, LO, HI, 7)) and counts.dtype == np.int64
    assert edges.dtype == np.float64 and np.array_equal(edges, LO + np.arange(8) * ((HI - LO) / 7))


def test_bad_arguments_are_refused():
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    Z = torch.zeros(16, dtype=torch.float32, device='cuda:0')
    out = torch.full((4096 + 4,), 5, dtype=torch.int32, device='cuda:0')
    call = lambda M, lo, hi, bins, z=Z, o=out: lib.rato_histogram(_lib.ptr(z), M, lo, hi, bins, _lib.ptr(o),
                                                                  _lib.current_stream())
    inf, nan = float("inf"), float("nan")
    for bad in ((16, 0.0, 1.0, 0), (16, 0.0, 1.0, 4097), (16, 0.0, 1.0, -1), (16, 1.0, 1.0, 8), (16, 2.0, 1.0, 8),
                (16, -inf, 1.0, 8), (16, 0.0, inf, 8), (16, nan, 1.0, 8), (16, 0.0, nan, 8), (0, 0.0, 1.0, 8),
                (16, -3e38, 3e38, 8)):                                         # (hi - lo overflows float32)
        assert call(*bad) == -1, bad
    assert call(16, 0.0, 1.0, 8, z=None) == -1 and call(16, 0.0, 1.0, 8, o=None) == -1
    torch.cuda.synchronize()
    assert bool((out == 5).all())                                              # a refused call writes nothing
    assert call(16, 0.0, 1.0, 4096) == 0 and call(16, 0.0, 1.0, 1) == 0
    with pytest.raises(_lib.RatoError):
        from riskaversetrajopt_amd import stats
        stats.histogram_device(Z, 1.0, 0.0, 8)

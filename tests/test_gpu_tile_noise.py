"""GPU: the re-tiled noise copy (rato_drone_tile_noise / rato_car_tile_noise) word for word, padding included.

Only the row-parallel linearize kernels read the copy, and they never look at the lanes beyond M, so the bit-for-bit
linearization tests say nothing about those words.  Here every word of the buffer is compared -- exactly: it is a copy --
with a NumPy re-tiling written from the layout comment of include/rato_saa.h: ceil(M / 64) blocks, each [S][64] (xi_0,
xi_1) pairs and then, for the drone's third axis, [S][64] xi_z; lanes beyond M hold 0.  The buffer starts as NaN, so a
word the kernel leaves out fails the comparison too.  M = 1 (one lane of one tile), 65 (a second tile with one lane),
130 (three tiles); the drone's source rows lie ld > M floats apart, so that a stride taken for M -- or the other way
round -- moves every row but the first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (65, 2), (130, 3)]
LANES = 64


def retile(dW, M):
    """dW [S][n_axes][ld] (host) -> the tiled copy as the header lays it out, flat"""
    S, n_axes, _ = dW.shape
    n_tiles = (M + LANES - 1) // LANES
    padded = np.zeros((S, n_axes, n_tiles * LANES), dtype=np.float32)
    padded[:, :, :M] = dW[:, :, :M]
    by_tile = padded.reshape(S, n_axes, n_tiles, LANES).transpose(2, 0, 1, 3)     # [tile][t][axis][lane]
    pairs = by_tile[:, :, :2, :].transpose(0, 1, 3, 2)                            # [tile][t][lane][2]
    planar = by_tile[:, :, 2:, :].transpose(0, 2, 1, 3)                           # [tile][axis][t][lane]
    return np.concatenate([pairs.reshape(n_tiles, -1), planar.reshape(n_tiles, -1)], axis=1).ravel()


def run(system, M, S):
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    n_axes = 3 if system == "drone" else 2
    ld = (M + 3) // 4 * 4 + 4 if system == "drone" else M
    rng = np.random.RandomState(1000 * M + S)
    dW = rng.standard_normal((S, n_axes, ld)).astype(np.float32)
    src = torch.from_numpy(dW).cuda()
    n = int(getattr(lib, "rato_%s_tiled_noise_floats" % ("drone" if system == "drone" else "car"))(M, S))
    assert n == (M + LANES - 1) // LANES * n_axes * S * LANES
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    if system == "drone":
        _lib.check(lib.rato_drone_tile_noise(_lib.ptr(src), M, ld, S, _lib.ptr(out), _lib.current_stream()), "rato_drone_tile_noise")
    else:
        _lib.check(lib.rato_car_tile_noise(_lib.ptr(src), M, S, _lib.ptr(out), _lib.current_stream()), "rato_car_tile_noise")
    return dW, out.cpu().numpy()


@pytest.mark.parametrize("M,S", SHAPES)
@pytest.mark.parametrize("system", ["drone", "car"])
def test_tile_noise_is_the_headers_layout_word_for_word(system, M, S):
    dW, got = run(system, M, S)
    want = retile(dW, M)
    assert got.shape == want.shape
    assert not np.isnan(got).any(), "a word of the tiled copy was not written"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    n_axes = dW.shape[1]
    blocks = got.reshape(-1, n_axes * S * LANES)                                   # the lanes beyond M hold +0.0
    tail = blocks[-1]
    last = M - (blocks.shape[0] - 1) * LANES
    pad = np.concatenate([tail[:2 * S * LANES].reshape(S, LANES, 2)[:, last:, :].ravel(),
                          tail[2 * S * LANES:].reshape(-1, LANES)[:, last:].ravel()])
    assert pad.size == (LANES - last) * n_axes * S and not pad.view(np.uint32).any()

"""Test helper (host only, NumPy; torch only to hold the buffer): designed packed Jacobians for the three consumers of
the tile-blocked layout (rato_saa_rowmax, rato_emit_csc_values, rato_saa_tail_rows_batch) and NumPy statements of what
they must return, written from the text of include/rato_saa.h and not from the kernels.

The UNTILED packed array is what a test designs:  products [n_pairs][n_g][R][M], factored [n_pairs][n_g][M] (with the
factor W [R][S][n_g][ld]),  pair(t, s) = t (t - 1) / 2 + s for 0 <= s < t < S.  ``tile_pack`` lays it out as the kernels
read it -- [tile][pair][g][r][lane], tiles rato_packed_tile_stride apart, the first one on a 2 MiB boundary when they are
padded -- inside an allocation that is NaN everywhere else: the words between padded tiles, the slack in front of the
first tile, lanes >= M of the last tile.  Whatever a consumer reads that the layout does not give it shows as NaN.

``integer_design`` / ``real_design`` fill the arrays.  Every integer entry is a hash of its own coordinates
(pair, g, r, i) reduced to +-1..8, so that a permutation of any index changes the result; with |x| <= 4 every product
and sum of a row is an integer below 2^24, exact in fp64 and in fp32: the expected outputs are exact.

``csc_run`` is the order rule of rato_emit_csc_values, ``rowmax_ref`` the rows of rato_saa_rowmax in extended precision,
``tail_sums`` the sums of rato_saa_tail_rows_batch.  ``emulate_read`` restates a consumer's index arithmetic with the
mistakes such a kernel could make; tests/test_packed_layout.py shows on the CPU that each of them changes what is read.
Checker only: nothing in the package imports this."""
import numpy as np

ALIGN_FLOATS = (2 << 20) // 4       # padded tiles start on 2 MiB boundaries
MIN_PADDED_BYTES = 1 << 20          # ... once a tile holds 1 MiB or more (rato_saa.h, "Tile stride")
EPS64 = 2.0 ** -53


def num_pairs(S):
    return S * (S - 1) // 2


def pair(t, s):
    return t * (t - 1) // 2 + s


def pad4(M):
    return (M + 3) // 4 * 4


def bytes_per_pair(n_g, RR, tile):
    """RR = row groups stored per (pair, control): R for products, 1 for the factored form"""
    return n_g * RR * tile * 4


def first_padded_S(n_g, RR, tile):
    """the smallest S whose tile holds >= 1 MiB, by the header's rule (the tests compare it with rato_packed_tile_stride)"""
    S = 2
    while num_pairs(S) * bytes_per_pair(n_g, RR, tile) < MIN_PADDED_BYTES:
        S += 1
    return S


def header_stride(payload_floats):
    """rato_saa.h: back to back while a tile is smaller than 1 MiB, otherwise every tile starts on a 2 MiB boundary"""
    if payload_floats * 4 < MIN_PADDED_BYTES:
        return payload_floats
    return (payload_floats + ALIGN_FLOATS - 1) // ALIGN_FLOATS * ALIGN_FLOATS


# ---- the layout ----------------------------------------------------------------------------------------------------
def storage_of(buf):
    """the whole allocation under a packed buffer as a flat fp32 tensor (the buffer itself when it is contiguous)"""
    import torch
    flat = torch.empty(0, dtype=torch.float32, device=buf.device)
    flat.set_(buf.untyped_storage())
    return flat


def tile_pack(untiled, tile, M, device):
    """untiled [rows...][M] (fp32) -> the kernels' buffer [n_tiles][rows...][tile] from _lib.packed_buffer (which applies
    rato_packed_tile_stride and the 2 MiB alignment).  The whole allocation is NaN first, then the payload is copied in,
    then lanes >= M of the last tile are NaN again.  A layout without pairs (S = 1) gets one row of NaN: G must not be NULL."""
    import torch
    from riskaversetrajopt_amd import _lib
    untiled = np.asarray(untiled, dtype=np.float32)
    assert untiled.shape[-1] == M and tile in (64, 256)
    rows = untiled.shape[:-1]
    if rows[0] == 0:
        rows = (1,) + rows[1:]
        untiled = np.full(rows + (M,), np.nan, dtype=np.float32)
    n_tiles = (M + tile - 1) // tile
    buf = _lib.packed_buffer((n_tiles,) + rows + (tile,), device)
    storage_of(buf).fill_(float("nan"))
    padded = np.zeros(rows + (n_tiles * tile,), dtype=np.float32)
    padded[..., :M] = untiled
    tiled = np.moveaxis(padded.reshape(rows + (n_tiles, tile)), -2, 0)
    buf.copy_(torch.from_numpy(np.ascontiguousarray(tiled)))
    if M < n_tiles * tile:
        buf[n_tiles - 1][..., M - (n_tiles - 1) * tile:] = float("nan")
    return buf


# ---- designed data -------------------------------------------------------------------------------------------------
def _mix(h):
    """a 64-bit finaliser (splitmix64) on uint64 arrays"""
    with np.errstate(over="ignore"):
        h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return h ^ (h >> np.uint64(31))


def coord_hash(shape, salt):
    """an array of ``shape`` whose entry is a hash of its own coordinates (and ``salt``): uint64"""
    h = np.full(shape, (int(salt) * 0x9E3779B97F4A7C15 + 1) % 2 ** 64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for ax, n in enumerate(shape):
            idx = np.arange(n, dtype=np.uint64).reshape([-1 if a == ax else 1 for a in range(len(shape))])
            h = _mix(h + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15 + 2 * ax))
    return h


def small_ints(shape, salt, hi=8):
    """non-zero integers in [-hi, hi], each a hash of its coordinates: float64 array"""
    h = coord_hash(shape, salt)
    mag = (h % np.uint64(hi)).astype(np.int64) + 1
    sign = 1 - 2 * ((h >> np.uint64(40)) & np.uint64(1)).astype(np.int64)
    return (mag * sign).astype(np.float64)


class Design:
    """One designed problem: untiled (fp32), W (fp32 [R][S][n_g][ld] or None), base (fp32 [R][S][ld]), x (fp64 [S][n_g]),
    everything beyond lane M of W / base NaN"""

    def __init__(self, S, M, R, n_g, factored, untiled, W, base, x):
        self.S, self.M, self.R, self.n_g, self.factored = S, M, R, n_g, factored
        self.ld = pad4(M) + 4
        self.untiled, self.x = np.asarray(untiled, dtype=np.float32), np.asarray(x, dtype=np.float64)
        self.W = None if W is None else self._rows(W)
        self.base = self._rows(base)

    def _rows(self, a):
        out = np.full(a.shape[:-1] + (self.ld,), np.nan, dtype=np.float32)
        out[..., :self.M] = a
        return out

    def with_base(self, base):
        return Design(self.S, self.M, self.R, self.n_g, self.factored, self.untiled, None if self.W is None else self.W[..., :self.M], base,
                      self.x)


def _shapes(S, M, R, n_g, factored):
    return (num_pairs(S), n_g, M) if factored else (num_pairs(S), n_g, R, M)


def integer_design(S, M, R, n_g=2, factored=False, salt=0):
    """G (or Phi and W) in +-1..8, x in +-1..4, base in +-1..8: a row's value is below 8 * 8 * 4 * n_g * S + 8 < 2^24"""
    assert 8 * 8 * 4 * n_g * S + 8 < 2 ** 24
    untiled = small_ints(_shapes(S, M, R, n_g, factored), 11 + salt)
    W = small_ints((R, S, n_g, M), 12 + salt) if factored else None
    return Design(S, M, R, n_g, factored, untiled, W, small_ints((R, S, M), 13 + salt), small_ints((S, n_g), 14 + salt, hi=4))


def real_design(S, M, R, n_g=2, factored=False, seed=0):
    """standard normals rounded to fp32 (x stays fp64)"""
    rng = np.random.RandomState(seed)
    f32 = lambda a: a.astype(np.float32)
    untiled = f32(rng.standard_normal(_shapes(S, M, R, n_g, factored)))
    W = f32(rng.standard_normal((R, S, n_g, M))) if factored else None
    return Design(S, M, R, n_g, factored, untiled, W, f32(rng.standard_normal((R, S, M))), rng.standard_normal((S, n_g)))


# ---- the contracts -------------------------------------------------------------------------------------------------
def csc_run(untiled, W, scale, S, M, R, n_g):
    """rato_emit_csc_values: "for s = 0..S-2, for g = 0..n_g-1, for sample i, for row-group r, for t = s+1..S-1:
    out = scale * d row(r,t) / d u[s,g]", column (s, g) being M R (S-1-s) consecutive values.  float32 arithmetic:
    float32(G) * float32(scale) for products, float32(float32(Phi * W) * scale) for the factored form.
    -> (values (M R n_g n_pairs,) fp32, offsets of the columns [(s, g)] -> start)"""
    untiled = np.asarray(untiled, dtype=np.float32)
    sc = np.float32(scale)
    out, starts, pos = [], {}, 0
    for s in range(S - 1):
        ts = np.arange(s + 1, S)
        rows = ts * (ts - 1) // 2 + s                               # pair(t, s), t = s+1 .. S-1
        for g in range(n_g):
            if W is None:
                blk = untiled[rows, g]                              # (nt, R, M)
            else:
                w = np.asarray(W, dtype=np.float32)[:, ts, g, :M]   # (R, nt, M)
                blk = (untiled[rows, g][:, None, :] * np.transpose(w, (1, 0, 2))).astype(np.float32)
            run = (np.transpose(blk, (2, 1, 0)) * sc).astype(np.float32).reshape(-1)     # [i][r][t]
            starts[(s, g)] = pos
            pos += run.size
            out.append(run)
    vals = np.concatenate(out) if out else np.zeros(0, np.float32)
    assert vals.size == M * R * n_g * num_pairs(S)
    return vals, starts


def rows_gx(untiled, W, x, S, M, R):
    """(G_i x)_{r,t} for every sample, only controls 0 and 1 entering, and sum |terms| of each: np.longdouble (a 64-bit
    significand where the platform provides one; the bound below never needs more than fp64).  -> two (R, S, M) arrays"""
    LD = np.longdouble
    G = np.asarray(untiled).astype(LD)
    xs = np.asarray(x, dtype=np.float64).astype(LD)
    rows = np.zeros((R, S, M), dtype=LD)
    mag = np.zeros((R, S, M), dtype=LD)
    for t in range(1, S):
        blk = G[pair(t, 0):pair(t, 0) + t]                          # (t, n_g, [R,] M), s = 0 .. t-1
        xt = xs[:t, :2]
        if W is None:
            terms = blk[:, :2] * xt[:, :, None, None]               # (t, 2, R, M)
        else:
            w = np.asarray(W)[:, t, :2, :M].astype(LD)              # (R, 2, M)
            terms = (blk[:, :2] * xt[:, :, None])[:, :, None, :] * np.transpose(w, (1, 0, 2))[None]
        terms = terms.reshape(-1, R, M)
        rows[:, t] = terms.sum(axis=0)
        mag[:, t] = np.abs(terms).sum(axis=0)
    return rows, mag


def rowmax_ref(untiled, W, base, sign, x, S, M, R, gx=None):
    """rato_saa_rowmax: rows r S + t of sample i are (G_i x)_{r,t} + sign base[r,t,i]; m = the maximum, arg = its row
    (smallest row index on ties).  ``gx``: rows_gx(...) of the same arrays, when several signs share it.
    -> (values (M,) longdouble, arg (M,) int64, sum |terms| (R S, M) fp64, rows (R S, M) longdouble)"""
    LD = np.longdouble
    rows, mag = gx if gx is not None else rows_gx(untiled, W, x, S, M, R)
    b = np.asarray(base)[..., :M].astype(LD)
    rows = (rows + LD(sign) * b).reshape(R * S, M)
    mag = (mag + np.abs(b)).reshape(R * S, M)
    return rows.max(axis=0), rows.argmax(axis=0), mag.astype(np.float64), rows    # argmax: the first maximum = smallest row


def ulp32(v):
    """the spacing of float32 in the binade of |v| (normal range)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.frexp(np.maximum(v, 2.0 ** -126))[1] - 1                # 2^e <= |v| < 2^(e+1)
    return np.ldexp(1.0, e - 23)


def rowmax_bound(ref_rows, mag, S):
    """|m_out - ref| <= ulp32(ref) / 2 + (2 S + 6) 2^-53 sum |terms|: one rounding to fp32 of a dot product of 2 (S - 1)
    + 1 terms summed in fp64 in any order, fused or not.  (R S, M) -> per row"""
    return ulp32(ref_rows.astype(np.float64)) / 2 + (2 * S + 6) * EPS64 * mag


def top_two_gap(rows):
    """per sample: value of the largest row minus the second largest"""
    if rows.shape[0] < 2:
        return np.full(rows.shape[1], np.inf)
    srt = np.sort(rows, axis=0)
    return (srt[-1] - srt[-2]).astype(np.float64)


def tail_sums(untiled, W, base, w, arg, S, M, R):
    """rato_saa_tail_rows_batch: [s 2 + g] = sum_i w_i G_i[r_i, (s, g)] (zero for s >= t_i), [2 (S-1)] = sum_i w_i
    base[r_i, t_i, i]; fp64 (exact on the integer design with weights 0 / 1) -> (2 (S - 1) + 1,)"""
    G = np.asarray(untiled, dtype=np.float64)
    out = np.zeros(2 * (S - 1) + 1)
    for i in np.flatnonzero(w):
        r, t = divmod(int(arg[i]), S)
        blk = G[pair(t, 0):pair(t, 0) + t]
        row = blk[:, :, i] * np.asarray(W, dtype=np.float64)[r, t, :, i][None] if W is not None else blk[:, :, r, i]   # (t, 2)
        out[:2 * t] += w[i] * row.reshape(-1)
        out[-1] += w[i] * float(base[r, t, i])
    return out


# ---- a consumer's read, and the mistakes it could make -------------------------------------------------------------
MISTAKES = ("wrong tile width", "un-padded stride", "RR = R on a factored buffer", "pair(t, s) with t and s swapped")


def emulate_read(flat, start, tile, S, M, R, n_g, factored, mistake=None):
    """What a consumer reads from the allocation ``flat`` (1-d fp32, first tile at float ``start``) for every
    (s, g, i, r, t > s), gathered by the kernels' index arithmetic -- tile_base + (i0 % tile) + lane + row * tile with
    row = (pair * n_g + g) * RR + r -- in csc_run's order, without the multiplications (factored: Phi alone, repeated
    for every r).  ``mistake``: one of MISTAKES.  Reads past the allocation come back NaN."""
    RR = 1 if factored else R
    tw = tile
    if mistake == "wrong tile width":
        tw = 64 if tile == 256 else 256
    rr_idx = R if mistake == "RR = R on a factored buffer" else RR
    payload = num_pairs(S) * n_g * rr_idx * tw
    stride = payload if mistake == "un-padded stride" else header_stride(payload)
    i = np.arange(M)
    out = []
    for s in range(S - 1):
        ts = np.arange(s + 1, S)
        prs = (s * (s - 1) // 2 + ts) if mistake == "pair(t, s) with t and s swapped" else (ts * (ts - 1) // 2 + s)
        for g in range(n_g):
            r = np.arange(R) if rr_idx == R else np.zeros(R, dtype=np.int64)
            row = (prs[None, None, :] * n_g + g) * rr_idx + r[None, :, None]                # (1, R, nt)
            idx = start + (i // tw)[:, None, None] * stride + (i % tw)[:, None, None] + row * tw
            ok = (idx >= 0) & (idx < flat.size)
            got = np.where(ok, flat[np.where(ok, idx, 0)], np.float32(np.nan))
            out.append(got.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def unscaled_run(d):
    """csc_run of a design's G alone (scale 1, the factored form without W): what ``emulate_read`` must return"""
    u = d.untiled if not d.factored else np.repeat(d.untiled[:, :, None, :], d.R, axis=2)
    return csc_run(u, None, 1.0, d.S, d.M, d.R, d.n_g)[0]

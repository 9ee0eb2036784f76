"""GPU: the three consumers of the packed tile-blocked Jacobian -- rato_saa_rowmax (csrc/cvar.hip), rato_emit_csc_values
(csrc/assemble.hip), rato_saa_tail_rows_batch -- on buffers DESIGNED on the host (tests/_packed_layout.py) against exact
references.  No model, no rollout: every table is an argument, so a case builds its tables, makes one call and compares.
Everything the layout does not give a consumer is NaN (tile padding, lanes >= M, rows of W / base beyond M, the third
control column of xs), every output carries a NaN / 0x7f guard region that must come back untouched, and ld = pad4(M) + 4.

Why the comparisons may be bit for bit:
  integer design (|G|, |W|, |base| <= 8, |x| <= 4, all non-zero integers, each a hash of its own coordinates): every product
    and every partial sum of a row is an integer below 2^24, so fp64 arithmetic in ANY order, fused or not, is exact, and so
    is the final rounding to fp32: m_out, arg_out (smallest row index on ties -- the integer rows tie often) and the block
    sums of the tail rows (weights 0 or 1) have exactly one correct answer;
  rato_emit_csc_values: a value is ONE correctly rounded fp32 multiply, G * scale (two for the factored form, Phi * W then
    * scale; Phi * W is exact on the integer design) -- nothing to reassociate or fuse; the scales keep every product normal.
The only tolerance is the dot-product bound of the real-valued rowmax cases (standard normals),
    |m_out - ref| <= ulp32(ref) / 2 + (2 S + 6) 2^-53 sum |terms|,
with the arg-max equal to the reference's for every sample; the reference's top two rows are asserted to be more than twice
that bound apart for every sample (the seed of a case is the first one for which they are, found on the host).

Records from the MI355X (records, not tolerances):
  real-valued rowmax (1008 calls: 3 forms x 2 tiles x 6 M x 7 S x 2 signs x 2 n_u), largest error / bound, printed as OBS
  lines: 0.999 - 1.000 for every form and tile with M >= 63 -- the bound is the half ulp of the final rounding to fp32 plus
  an fp64 term ~1e-9 of it, and some sample of a few hundred always rounds by nearly half an ulp (M = 1: 0.0 at S = 1, where
  m = sign * base is already a float, up to 0.96).  That figure says nothing about the fp64 sums, so the test also holds the
  fp64 part on its own: wherever every number within (2 S + 6) 2^-53 sum |terms| of the reference rounds to one float,
  m_out must be that float.  That decided all 129,528 sample values of the sweep (none was closer to a rounding tie than
  the fp64 term), and all were equal bit for bit.  No kernel had to change for these tests.
Outcome at the LDS limit of rato_emit_csc_values, 64 (R (S - 1) + 1) 4 bytes <= 160 KiB = 163,840 B: R = 3, S = 214 and
  R = 1, S = 640 need exactly 163,840 B; both launch and give the right values, S = 215 / 641 return RATO_EINVAL and write
  nothing.  The guard was right and is unchanged; include/rato_saa.h and the comment in csrc/assemble.hip said "S <= 213 /
  639" and now state S <= 214 / 640, as the guard and the two facades (drone_risk.py, driving.py: > 160 * 1024) compute.
  The first horizon that needs the kernel's LDS limit raised (> 65,536 B) is S = 257 for R = 1 and S = 87 for R = 3
  (S = 86 is 65,536 B exactly and still inside the default): 85, 86, 87 and 256, 257 all run here.
Kernel mistakes tried in a scratch build, one per kernel and build, each keeping every access inside the buffers (nothing
of those builds is committed); failing cases of the 43 rowmax and 78 emit cases of this module:
  g0 / g1 swapped in rowmax_kernel              28 of 43: every products case (24 of the sweep, 4 tie cases); the factored
                                                instantiation has no g0 / g1
  the `v == best` tie branch removed            18 of 43: all 6 tie cases and 12 of the sweep (integer rows that tie inside
                                                a wave)
  the cross-wave merge using `>` only           36 of 43: all 6 tie cases and 30 of the sweep (all but M = 1)
  scale applied before the W multiply (emit)    31 of 78: every factored case; products have one multiply either way
  r and dtt exchanged in the LDS row index      46 of 78: every R = 3 case; with R = 1 the exchange is the identity
No mistake went unnoticed, so no case had to be added for them.
"""
import itertools

import numpy as np
import pytest

from tests import _packed_layout as pl
from tests import _tail_patterns as tp

pytestmark = pytest.mark.gpu

TILES = (64, 256)
MS = (1, 63, 64, 65, 257, 321)     # tile 256, M = 321: chunks starting at lanes 64, 128, 192 of tile 0, a full chunk and a one-lane chunk in tile 1
FORMS = {"products R=3": (3, False), "factored R=3": (3, True), "products R=1": (1, False)}     # rowmax_kernel<3,false>, <3,true>, <1,false>
POISON_I32 = 0x7f7f7f7f
N_STATS = 11


def boundary_S(R, factored, tile, n_g=2):
    """(last back-to-back S, first padded S) of a form"""
    Sp = pl.first_padded_S(n_g, 1 if factored else R, tile)
    return (Sp - 1, Sp)


def _dev():
    import torch
    return torch.device("cuda:0")


class Tables:
    """a design on the device: G in the kernels' layout, W, base"""

    def __init__(self, d, tile):
        import torch
        self.d, self.tile, dev = d, tile, _dev()
        self.G = pl.tile_pack(d.untiled, tile, d.M, dev)
        self.W = None if d.W is None else torch.as_tensor(d.W, device=dev)
        self.base = torch.as_tensor(d.base, device=dev)


def _xs(x, n_u):
    """[S][n_u] doubles on the device; control columns >= 2 are NaN: only controls 0 and 1 may enter"""
    import torch
    xs = np.full((x.shape[0], n_u), np.nan)
    xs[:, :2] = x[:, :2]
    return torch.as_tensor(xs, dtype=torch.float64, device=_dev())


def _rowmax_outputs(ld):
    import torch
    return (torch.full((ld,), float("nan"), dtype=torch.float32, device=_dev()),
            torch.full((ld,), POISON_I32, dtype=torch.int32, device=_dev()))


def _rowmax(lib, T, sign, n_u, xs=None, outs=None):
    """one call -> (status, m_out[:M], arg_out[:M]) with the guards checked (entries >= M untouched)"""
    from riskaversetrajopt_amd import _lib
    d = T.d
    xs = _xs(d.x, n_u) if xs is None else xs
    m, a = outs or _rowmax_outputs(d.ld)
    rc = lib.rato_saa_rowmax(_lib.ptr(T.G), _lib.ptr(T.W), T.tile, d.R, d.S, d.M, d.ld, _lib.ptr(T.base), float(sign),
                             _lib.ptr(xs), n_u, _lib.ptr(m), _lib.ptr(a), _lib.current_stream())
    m, a = m.cpu().numpy(), a.cpu().numpy()
    assert np.isnan(m[d.M:]).all() and np.all(a[d.M:] == POISON_I32), "guard entries >= M were written"
    return rc, m[:d.M], a[:d.M]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def real_case(S, M, R, factored, seed0):
    """the first seed >= seed0 whose design separates the top two rows of every sample by more than twice the bound, for both
    signs.  Decided on the host from the reference alone; a design is used only if the condition holds for every sample,
    and the search raising is the assertion failing.  -> (design, {sign: (ref values, arg, bound per sample, the fp64 term
    (2 S + 6) 2^-53 sum |terms| of that bound alone)})"""
    for seed in range(seed0, seed0 + 50):
        d = pl.real_design(S, M, R, 2, factored, seed=seed)
        gx = pl.rows_gx(d.untiled, d.W, d.x, S, M, R)
        refs, ok = {}, True
        for sign in (1.0, -1.0):
            v, arg, mag, rows = pl.rowmax_ref(d.untiled, d.W, d.base, sign, d.x, S, M, R, gx=gx)
            bound = pl.rowmax_bound(rows, mag, S)                                   # (R S, M)
            ok = ok and bool(np.all(pl.top_two_gap(rows) > 2 * bound.max(axis=0)))
            refs[sign] = (v, arg, bound[arg, np.arange(M)], (2 * S + 6) * pl.EPS64 * mag[arg, np.arange(M)])
        if ok:
            return d, refs
    raise AssertionError("no seed separates the top two rows")


def rowmax_S(R, factored, tile):
    return (1, 2, 7, 9, 20) + boundary_S(R, factored, tile)


# ---- rato_saa_rowmax -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_rowmax_on_designed_buffers(form, tile, M):
    """every S of the form (1: no pairs, every row sign * base; 2; 7 and 9: fewer and more rows than waves; 20; both
    sides of the stride boundary) x sign +-1 x n_u 2 / 3: integer design bit for bit, real-valued design within the
    dot-product bound with the reference's arg-max for every sample"""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    R, factored = FORMS[form]
    worst, decided, total = 0.0, 0, 0
    for S in rowmax_S(R, factored, tile):
        d = pl.integer_design(S, M, R, 2, factored, salt=S * 1000 + M)
        T = Tables(d, tile)
        gx = pl.rows_gx(d.untiled, d.W, d.x, S, M, R)
        for sign, n_u in itertools.product((1.0, -1.0), (2, 3)):
            v, arg, _, _ = pl.rowmax_ref(d.untiled, d.W, d.base, sign, d.x, S, M, R, gx=gx)
            assert np.all(np.abs(v) < 2 ** 24)
            rc, m, a = _rowmax(lib, T, sign, n_u)
            assert rc == 0
            assert np.array_equal(_bits(m), _bits(v.astype(np.float64))), (S, sign, n_u)
            assert np.array_equal(a, arg), (S, sign, n_u, np.flatnonzero(a != arg)[:5])
        d, refs = real_case(S, M, R, factored, seed0=S * 100 + M)
        T = Tables(d, tile)
        for sign, n_u in itertools.product((1.0, -1.0), (2, 3)):
            v, arg, bound, term = refs[sign]
            rc, m, a = _rowmax(lib, T, sign, n_u)
            assert rc == 0
            err = np.abs(m.astype(np.longdouble) - v).astype(np.float64)
            ratio = float(np.max(err / bound))
            worst = max(worst, ratio)
            print(f"OBS rowmax real {form} tile={tile} M={M} S={S} sign={sign:+.0f} n_u={n_u}: max err/bound {ratio:.3f}")
            assert not np.isnan(m).any() and np.all(err <= bound), (S, sign, n_u, ratio)
            assert np.array_equal(a, arg), (S, sign, n_u, np.flatnonzero(a != arg)[:5])
            # the fp64 part on its own: wherever every value within the fp64 term of the reference rounds to the same float
            # (the reference is not that close to a rounding tie), m_out must BE that float
            lo, hi = (v - term).astype(np.float32), (v + term).astype(np.float32)
            sure = lo == hi
            assert np.array_equal(_bits(m[sure]), _bits(lo[sure])), (S, sign, n_u, "fp64 part")
            decided, total = decided + int(sure.sum()), total + M
    print(f"OBS rowmax real {form} tile={tile} M={M}: worst err/bound {worst:.3f}; equal to float32(ref) bit for bit in all "
          f"{decided} of {total} samples whose reference is further than the fp64 term from a rounding tie")


def _tie_targets(kind, R, S, M):
    """row values (R, S, M) with designed ties at the maximum -> (targets, expected arg (M,))"""
    tgt = -5.0 - np.abs(pl.small_ints((R, S, M), 77))                     # every other row distinct-ish and far below
    i = np.arange(M)
    if kind == "two rows":                                               # (r = 2, t = 0) and (r = 0, t = 5) -> 5;  R = 1: t = 3 and t = 5
        rows = [(2, 0), (0, 5)] if R == 3 else [(0, 5), (0, 3)]
        for r, t in rows:
            tgt[r, t] = 9.0
        return tgt, np.full(M, min(r * S + t for r, t in rows))
    if kind == "same group, smaller t":                                  # (r, t = 11) and (r, t = 2) of the middle / only row group: a wave
        r = R // 2                                                       # that takes both meets the larger index first and needs the
        tgt[r, 11], tgt[r, 2] = 9.0, 9.0                                 # `v == best` branch; two waves need the merge's
        return tgt, np.full(M, r * S + 2)
    if kind == "far apart in t":                                         # steps 1 and S - 1: taken by different waves (longest first)
        tgt[R - 1, 1], tgt[0, S - 1] = 9.0, 9.0
        return tgt, np.full(M, min((R - 1) * S + 1, S - 1))
    if kind == "one per row group":                                      # a step per sample in every row group
        h = pl.coord_hash((R, M), 5)
        ts = (h % np.uint64(S)).astype(np.int64)
        for r in range(R):
            tgt[r, ts[r], i] = 9.0
        return tgt, ts[0]
    if kind == "two rows per sample":                                    # two distinct rows chosen per sample
        h = pl.coord_hash((2, M), 6)
        a = (h[0] % np.uint64(R * S)).astype(np.int64)
        b = (a + 1 + (h[1] % np.uint64(R * S - 1)).astype(np.int64)) % (R * S)
        flat = tgt.reshape(R * S, M)
        flat[a, i], flat[b, i] = 9.0, 9.0
        return tgt, np.minimum(a, b)
    raise KeyError(kind)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_rowmax_ties_take_the_smallest_row_every_time(form, tile):
    """Designed ties at the maximum on the integer design (the rows are set through base = sign (target - G x), exact):
    all rows equal; (r = 2, t = 0) with (r = 0, t = 5); steps 1 and S - 1, which different waves take; one row per row
    group; two rows per sample; two steps of one row group.  Five calls each: values and arg-max identical every time.
    Which rule a design needs: waves take steps in descending t, so a wave meets the smaller row index AFTER the larger one
    only when both lie in one row group (or, R = 3, the smaller index has the smaller t: r S + t).  For R = 3 "two rows" and
    "far apart in t" put the smaller index on the larger t: they need the cross-wave merge's tie rule alone.  The in-wave
    `v == best` branch is needed by "all rows equal" (every wave with two or more steps), "same group, smaller t", the R = 1
    variants, and part of the samples of "one per row group" / "two rows per sample"."""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    R, factored = FORMS[form]
    S, M = 20, 321
    d0 = pl.integer_design(S, M, R, 2, factored, salt=9)
    gx = pl.rows_gx(d0.untiled, d0.W, d0.x, S, M, R)[0].astype(np.float64)
    cases = []
    zero = pl.Design(S, M, R, 2, factored, np.zeros_like(d0.untiled), None if d0.W is None else d0.W[..., :M],
                     np.full((R, S, M), 3.0), d0.x)                       # G = 0, constant base: every row equal -> arg 0
    cases.append(("all rows equal", zero, {1.0: (np.full(M, 3.0), np.zeros(M, int)), -1.0: (np.full(M, -3.0), np.zeros(M, int))}))
    for kind in ("two rows", "same group, smaller t", "far apart in t", "one per row group", "two rows per sample"):
        tgt, arg = _tie_targets(kind, R, S, M)
        for sign in (1.0, -1.0):
            base = sign * (tgt - gx)
            assert np.all(np.abs(base) < 2 ** 24) and np.array_equal(base, np.round(base))
            cases.append((kind, d0.with_base(base), {sign: (np.full(M, 9.0), arg)}))
    for kind, d, want in cases:
        T = Tables(d, tile)
        for sign, (v, arg) in want.items():
            v_ref, arg_ref, _, _ = pl.rowmax_ref(d.untiled, d.W, d.base, sign, d.x, S, M, R)
            assert np.array_equal(v_ref.astype(np.float64), v) and np.array_equal(arg_ref, arg), kind     # the design does what it says
            for rep in range(5):
                rc, m, a = _rowmax(lib, T, sign, 2 + rep % 2)
                assert rc == 0 and np.array_equal(_bits(m), _bits(v)), (kind, sign, rep)
                assert np.array_equal(a, arg), (kind, sign, rep, np.flatnonzero(a != arg)[:5])


def test_rowmax_refusals_write_nothing():
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    d = pl.integer_design(7, 65, 3, 2, False)
    df = pl.integer_design(7, 65, 3, 2, True)
    d1 = pl.integer_design(7, 65, 1, 2, False)
    T, Tf, T1 = Tables(d, 64), Tables(df, 64), Tables(d1, 64)
    xs2 = _xs(d.x, 2)
    st = _lib.current_stream()

    def call(G=T.G, W=None, tile=64, R=3, S=7, M=65, ld=d.ld, base=T.base, sign=-1.0, xs=xs2, n_u=2, null=None):
        m, a = _rowmax_outputs(d.ld)
        args = dict(G=_lib.ptr(G), W=_lib.ptr(W), base=_lib.ptr(base), xs=_lib.ptr(xs), m=_lib.ptr(m), a=_lib.ptr(a))
        if null:
            args[null] = None
        rc = lib.rato_saa_rowmax(args["G"], args["W"], tile, R, S, M, ld, args["base"], sign, args["xs"], n_u, args["m"],
                                 args["a"], st)
        import torch
        torch.cuda.synchronize()
        assert bool(torch.isnan(m).all()) and bool((a == POISON_I32).all()), "a refused call wrote its outputs"
        return rc

    assert call(R=2) == -1
    assert call(G=T1.G, W=Tf.W, R=1, base=T1.base) == -1                  # R = 1 takes no factor
    assert call(tile=128) == -1
    assert call(ld=64) == -1                                              # ld < M
    assert call(n_u=1) == -1
    assert call(sign=0.5) == -1
    assert call(S=0) == -1 and call(M=0) == -1
    for null in ("G", "base", "xs", "m", "a"):
        assert call(null=null) == -1, null
    rc, m, a = _rowmax(lib, T, -1.0, 2)                                   # and the same tables are accepted as they are
    assert rc == 0 and not np.isnan(m).any()


# ---- rato_emit_csc_values ------------------------------------------------------------------------------------------
SCALES = (1.0, 0.01, 1e-9)


def _emit(lib, T, scale, expect_rc=0):
    """one call -> values (M R n_g n_pairs,), the 64 guard floats behind them checked"""
    import torch
    from riskaversetrajopt_amd import _lib
    d = T.d
    n = d.M * d.R * d.n_g * pl.num_pairs(d.S)
    out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=_dev())
    rc = lib.rato_emit_csc_values(_lib.ptr(T.G), _lib.ptr(T.W), d.ld if T.W is not None else 0, T.tile, d.n_g, d.R, d.S,
                                  d.M, float(scale), _lib.ptr(out), _lib.current_stream())
    assert rc == expect_rc, rc
    out = out.cpu().numpy()
    assert np.isnan(out[n:]).all(), "guard floats behind the values were written"
    return out[:n]


def _check_emit(lib, d, tile, scales=SCALES):
    T = Tables(d, tile)
    tiny = np.finfo(np.float32).tiny
    for scale in scales:
        want, _ = pl.csc_run(d.untiled, d.W, scale, d.S, d.M, d.R, d.n_g)
        assert np.all(np.abs(want) >= tiny) and np.isfinite(want).all()              # every product a normal float32
        got = _emit(lib, T, scale)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (d.S, d.M, d.R, d.n_g, d.factored, tile, scale, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


EMIT_FORMS = {"products R=3": (3, 2, False), "factored R=3": (3, 2, True), "products R=1": (1, 2, False)}


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", sorted(EMIT_FORMS))
def test_emit_csc_on_designed_buffers(form, tile, M):
    """S = 2 (one column pair, nt = 1), 3, 20 and both sides of the stride boundary x scale 1, 0.01, 1e-9, bit for bit"""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    R, n_g, factored = EMIT_FORMS[form]
    for S in (2, 3, 20) + boundary_S(R, factored, tile):
        _check_emit(lib, pl.integer_design(S, M, R, n_g, factored, salt=S * 1000 + M), tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("R,n_g,factored", [(3, 1, False), (3, 1, True), (1, 3, False), (1, 3, True), (1, 2, True)])
def test_emit_csc_other_row_and_control_counts(R, n_g, factored, tile):
    """the ABI takes any n_g > 0 and a factor with any R: (R, n_g) = (3, 1) and (1, 3), and R = 1 with a factor"""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    for S, M in ((9, 321), (20, 65)):
        _check_emit(lib, pl.integer_design(S, M, R, n_g, factored, salt=n_g), tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", sorted(EMIT_FORMS))
def test_emit_csc_real_values_are_single_rounded_products(form, tile):
    """standard normals kept away from zero: G * scale is one correctly rounded multiply whatever the data"""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    R, n_g, factored = EMIT_FORMS[form]
    for S, M in ((9, 321), (20, 65)):
        d = pl.real_design(S, M, R, n_g, factored, seed=S)
        keep = lambda a: (np.sign(a) * np.maximum(np.abs(a), 1e-3)).astype(np.float32)
        d = pl.Design(S, M, R, n_g, factored, keep(d.untiled), None if d.W is None else keep(d.W[..., :M]), d.base[..., :M], d.x)
        _check_emit(lib, d, tile)


# dynamic LDS of the emit kernel: 64 (R (S - 1) + 1) 4 bytes; beyond 65,536 B the launcher raises the kernel's limit first
# (hipFuncSetAttribute).  R = 1: S = 256 is 65,536 B exactly, S = 257 the first beyond.  R = 3: S = 85 is 65,024 B, S = 86
# is 65,536 B exactly (3 * 85 + 1 = 256) and still inside the default, S = 87 (66,304 B) the first beyond.
LDS_CROSSING = [(3, False, 85), (3, False, 86), (3, False, 87), (3, True, 85), (3, True, 86), (3, True, 87),
                (1, False, 256), (1, False, 257), (1, True, 256), (1, True, 257)]
FIRST_RAISED = {3: 87, 1: 257}


def emit_lds_bytes(R, S):
    return 64 * (R * (S - 1) + 1) * 4


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("R,factored,S", LDS_CROSSING)
def test_emit_csc_across_the_default_lds_limit(R, factored, S, tile):
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    assert (emit_lds_bytes(R, S) > 64 * 1024) == (S >= FIRST_RAISED[R]) and emit_lds_bytes(R, FIRST_RAISED[R] - 1) == 64 * 1024
    _check_emit(lib, pl.integer_design(S, 65, R, 2, factored, salt=S), tile, scales=(0.01,))


# the largest S the guard accepts and the first it refuses, by its own arithmetic (160 KiB = 163,840 B)
LDS_LIMIT = 160 * 1024
LARGEST = [(3, False, 214, 65), (3, True, 214, 65), (1, False, 640, 3)]


@pytest.mark.parametrize("R,factored,S,M", LARGEST)
def test_emit_csc_at_the_largest_accepted_horizon(R, factored, S, M):
    """R = 3, S = 214: 64 * 640 * 4 = 163,840 B exactly; R = 1, S = 640: 64 * 640 * 4 likewise.  One tile of 64 for the
    latter (a 105 MB buffer)."""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    assert emit_lds_bytes(R, S) == LDS_LIMIT and emit_lds_bytes(R, S + 1) > LDS_LIMIT
    _check_emit(lib, pl.integer_design(S, M, R, 2, factored, salt=S), 64, scales=(0.01,))


@pytest.mark.parametrize("R,S,M", [(3, 215, 65), (1, 641, 3)])
def test_emit_csc_refuses_the_first_horizon_beyond(R, S, M):
    """returns RATO_EINVAL and writes nothing (full-size buffers, so that a guard that let it through would stay in bounds)"""
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    assert emit_lds_bytes(R, S) > LDS_LIMIT >= emit_lds_bytes(R, S - 1)
    G = _lib.packed_buffer((1 if M <= 64 else 2, pl.num_pairs(S), 2, R, 64), _dev())
    pl.storage_of(G).fill_(1.0)
    n = M * R * 2 * pl.num_pairs(S)
    out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=_dev())
    rc = lib.rato_emit_csc_values(_lib.ptr(G), None, 0, 64, 2, R, S, M, 1.0, _lib.ptr(out), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(out).all())


def test_emit_csc_refusals_write_nothing():
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    d = pl.integer_design(7, 65, 3, 2, False)
    T = Tables(d, 64)
    n = 65 * 3 * 2 * pl.num_pairs(7)
    for kw in (dict(tile=128), dict(S=1), dict(M=0), dict(n_g=0), dict(R=0), dict(G=None), dict(out=None)):
        out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=_dev())
        a = dict(G=T.G, tile=64, n_g=2, R=3, S=7, M=65, out=out)
        a.update(kw)
        rc = lib.rato_emit_csc_values(_lib.ptr(a["G"]), None, 0, a["tile"], a["n_g"], a["R"], a["S"], a["M"], 1.0,
                                      _lib.ptr(a["out"]), _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == -1 and bool(torch.isnan(out).all()), kw


# ---- rato_saa_tail_rows_batch: the layout axis ------------------------------------------------------------------------
TAIL_M = 321
TAIL_A = 107          # alpha = 107 / 321: alpha M = 107.0 exactly in fp64 (asserted), 64 tail samples in block 0, 43 in block 1


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_tail_rows_on_designed_buffers(form, tile):
    """integer design, S on both sides of the stride boundary, M = 321, a tail pattern without ties (tests/_tail_patterns.pack:
    every weight 0 or 1), the record from risk_stats_device on the designed m: the block sums are sums of integers, so
    part.sum(0) equals the fp64 sums over the untiled array bit for bit"""
    import torch
    from riskaversetrajopt_amd import _lib, stats
    lib = _lib.load()
    R, factored = FORMS[form]
    M, alpha = TAIL_M, TAIL_A / TAIL_M
    assert alpha * M == float(TAIL_A)
    p = tp.pack(64, M=M, alpha=alpha)
    w, _, n_gt, n_eq, lam = p.weights()
    assert lam == 1.0 and set(np.unique(w)) == {0.0, 1.0} and n_gt + n_eq == TAIL_A
    m_dev = torch.as_tensor(p.m, device=_dev())
    rec = stats.risk_stats_device(m_dev, alpha)
    st = rec.cpu().numpy()
    lam_d = min(max((alpha * M - st[8]) / st[9], 0.0), 1.0) if st[9] > 0 else 0.0
    assert np.array_equal((p.m > np.float32(st[10])) * 1.0 + (p.m == np.float32(st[10])) * lam_d, w)     # the device's record gives these weights
    nblk = (M + 255) // 256
    for S in boundary_S(R, factored, tile):
        d = pl.integer_design(S, M, R, 2, factored, salt=S)
        T = Tables(d, tile)
        arg = tp.args("uniform", S, R, M, np.random.RandomState(S))
        nc = 2 * (S - 1) + 1
        flat = torch.full((nblk * nc + 64,), float("nan"), dtype=torch.float64, device=_dev())      # part, then 64 guard doubles
        _lib.check(lib.rato_saa_tail_rows_batch(_lib.ptr(T.G), _lib.ptr(T.W), d.ld, tile, R, S, M, _lib.ptr(T.base), _lib.ptr(m_dev),
                                                _lib.ptr(torch.as_tensor(arg, device=_dev())), _lib.ptr(rec), N_STATS, None, 1,
                                                alpha * M, _lib.ptr(flat), _lib.current_stream()), "rato_saa_tail_rows_batch")
        flat = flat.cpu().numpy()
        got = flat[:nblk * nc].reshape(nblk, 1, nc)
        assert np.isnan(flat[nblk * nc:]).all(), "guard doubles behind part were written"
        want = pl.tail_sums(d.untiled, None if d.W is None else d.W[..., :M], d.base[..., :M], w, arg, S, M, R)
        assert np.all(np.abs(want) < 2 ** 53) and np.array_equal(want, np.round(want))
        assert np.array_equal(got[:, 0].sum(axis=0), want), (S, np.flatnonzero(got[:, 0].sum(axis=0) != want)[:5])


# ---- one producer link: the designed layout is the layout the producers write --------------------------------------
@pytest.mark.parametrize("cpt,spl,tile", [(-1, 1, 64), (4, 1, 256)])
def test_producer_buffer_and_its_repacked_copy_give_the_same_outputs(cpt, spl, tile):
    import torch
    from riskaversetrajopt_amd import _lib, drone_risk
    from oracle import drone as od
    S, M = 20, 130
    d = drone_risk.Model(S, *od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=M, S=S), 'saa', 0.1)
    lib = d._lib
    r = d.linearize_device(tp.graze(S), cols_per_thread=cpt, samples_per_lane=spl, factored=False, rows_out=1)
    assert r["tile"] == tile and not r["factored"]
    ld = r["_g_up"].shape[-1]
    Gu = drone_risk.untile(r["G"], M).cpu().numpy()                       # [n_pairs][2][3][M]
    G2 = pl.tile_pack(Gu, tile, M, r["G"].device)
    assert G2.data_ptr() != r["G"].data_ptr()
    xs = torch.as_tensor(tp.graze(S) * 0.1, dtype=torch.float64, device=r["G"].device).contiguous()
    res = []
    for G in (r["G"], G2):
        m, a = _rowmax_outputs(ld)
        _lib.check(lib.rato_saa_rowmax(_lib.ptr(G), None, tile, 3, S, M, ld, _lib.ptr(r["_g_up"]), 1.0, _lib.ptr(xs), 3,
                                       _lib.ptr(m), _lib.ptr(a), _lib.current_stream()), "rato_saa_rowmax")
        n = M * 3 * 2 * pl.num_pairs(S)
        vals = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=G.device)
        _lib.check(lib.rato_emit_csc_values(_lib.ptr(G), None, 0, tile, 2, 3, S, M, 0.01, _lib.ptr(vals), _lib.current_stream()),
                   "rato_emit_csc_values")
        res.append((m.cpu().numpy(), a.cpu().numpy(), vals.cpu().numpy()))
    for x, y in zip(*res):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert not np.isnan(res[0][0][:M]).any() and not np.isnan(res[0][2][:-64]).any() and np.isnan(res[0][2][-64:]).all()
    want, _ = pl.csc_run(Gu, None, 0.01, S, M, 3, 2)                      # and the emission of the producer's own numbers
    assert np.array_equal(_bits(res[0][2][:-64]), _bits(want))

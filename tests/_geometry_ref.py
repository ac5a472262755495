"""Plain statements of the geometry kernels (csrc/geometry.hip, csrc/proj_pred.h) and the inputs that put them at their edges
(test infrastructure; CPU only: imports neither the GPU, nor the library, nor the C oracle).

Everything is integers or fractions.Fraction: no tolerance appears anywhere.  A kernel step that rounds (a product, a sum, a fused
multiply-add) is the exact rational value rounded ONCE to fp32 by fl32(); `exact_log`, when given, collects for every such step
whether the rounding changed the value.  On the dyadic inputs of the edge tests it never does (tests/test_geometry_ref_host.py
asserts that), so neither the order of evaluation nor fma-versus-mul+add can matter there; the only rows where it does are the fp32
neighbours of a range limit, whose roundings are the contract's own (mul, fma, fma, fma: proj_pred.h) and are checked against the
C oracle.  The two divisions u = a0 / a2, v = a1 / a2 are IEEE fp32 divisions (numpy float32)."""
from fractions import Fraction

import numpy as np
import torch

from _elementwise_ref import cast_statement

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- fp32 helpers
def fl32(q, exact_log=None):
    """The rational q rounded to the nearest fp32 number, ties to even (normal and subnormal range; overflow is an error)."""
    q = Fraction(q)
    if q == 0:
        return Fraction(0)
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()           # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                         # 2^e <= a < 2^(e+1)
    assert e <= 127, "fp32 overflow in a statement"
    ulp = Fraction(2) ** (max(e, -126) - 23)
    m = a / ulp
    k = m.numerator // m.denominator
    r = m - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and (k & 1)):
        k += 1
    out = s * k * ulp
    if exact_log is not None:
        exact_log.append(out == q)
    return out


def frac(x):
    """The exact value of a finite float."""
    return Fraction(float(x))


def is_f32(q):
    return fl32(q) == Fraction(q)


def nxt(x, up):
    return F32(np.nextafter(F32(x), F32(np.inf if up else -np.inf)))


# ---------------------------------------------------------------------------------------------------------------- predicates
# the camera-mask suite's calibration: u = 64 - 60 y / x, v = 48 - 60 z / x, a2 = x   (row-major 4x3, p' = [x y z 1] . crt)
CRT_DYADIC = np.array([[64.0, 48.0, 1.0], [-60.0, 0.0, 0.0], [0.0, -60.0, 0.0], [0.0, 0.0, 0.0]], dtype=F32)


def in_range(pts, lim):
    """Strict on all six limits; a NaN compares false, +inf fails its upper limit."""
    p = np.asarray(pts, dtype=F32).reshape(-1, 3)
    l = np.asarray(lim, dtype=F32)
    with np.errstate(invalid="ignore"):
        return (p[:, 0] > l[0]) & (p[:, 0] < l[1]) & (p[:, 1] > l[2]) & (p[:, 1] < l[3]) & (p[:, 2] > l[4]) & (p[:, 2] < l[5])


def proj_chain(row, crt, exact_log=None):
    """(a0, a1, a2) of one finite row as fp32-valued Fractions: fl(x c0) -> fma(y, c3, .) -> fma(z, c6, .) -> fma(1, c9, .)."""
    c = np.asarray(crt, dtype=F32).reshape(4, 3)
    x, y, z = (frac(v) for v in row)
    out = []
    for j in range(3):
        t = fl32(x * frac(c[0, j]), exact_log)
        t = fl32(y * frac(c[1, j]) + t, exact_log)
        t = fl32(z * frac(c[2, j]) + t, exact_log)
        t = fl32(frac(c[3, j]) + t, exact_log)
        out.append(t)
    return out


def _keep_uv_row(row, crt, ulim, vlim, mode, exact_log=None):
    a = [F32(float(t)) for t in proj_chain(row, crt, exact_log)]      # (exact: every t is an fp32 value)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = F32(a[0] / a[2]), F32(a[1] / a[2])
        keep = bool(u > 0) and bool(u < F32(ulim)) and bool(v > 0) and bool(v < F32(vlim))
    if mode == 1:
        keep = keep and bool(a[2] > 0)
    return keep, u, v


def project_keep(pts, lim, crt, ulim, vlim, mode, exact_log=None):
    """Keep mask [n] and (u, v) [n,2] (defined where the row passes the range test) of the projection predicate; mode 0 = compat
    (no depth test), 1 = correct (a2 > 0 as well).  Rows are evaluated once per distinct bit pattern."""
    p = np.ascontiguousarray(np.asarray(pts, dtype=F32).reshape(-1, 3))
    keep = np.zeros(p.shape[0], dtype=bool)
    uv = np.zeros((p.shape[0], 2), dtype=F32)
    rng = in_range(p, lim)
    if not rng.any():
        return keep, uv
    rows = np.flatnonzero(rng)
    uniq, inv = np.unique(p[rows].view(np.uint32), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    ku = np.zeros(uniq.shape[0], dtype=bool)
    uu = np.zeros((uniq.shape[0], 2), dtype=F32)
    for t in range(uniq.shape[0]):
        ku[t], uu[t, 0], uu[t, 1] = _keep_uv_row(uniq[t].view(F32), crt, ulim, vlim, mode, exact_log)
    keep[rows] = ku[inv]
    uv[rows] = uu[inv]
    return keep, uv


def compact(keep):
    """Order-preserving compaction: (src rows int32 [count], count)."""
    src = np.flatnonzero(np.asarray(keep, dtype=bool)).astype(np.int32)
    return src, int(src.shape[0])


def range_filter(pts, lim):
    """-> (kept rows [m,3] bit for bit, src [m], m)."""
    p = np.asarray(pts, dtype=F32).reshape(-1, 3)
    src, m = compact(in_range(p, lim))
    return p[src], src, m


def project_filter(pts, lim, crt, ulim, vlim, mode, exact_log=None):
    """-> (uv [m,2], xyz [m,3], src [m], m)."""
    p = np.asarray(pts, dtype=F32).reshape(-1, 3)
    keep, uv = project_keep(p, lim, crt, ulim, vlim, mode, exact_log)
    src, m = compact(keep)
    return uv[src], p[src], src, m


# the keep patterns of the compaction tests: row i of n -> kept?
CP_TILE = 1024
PATTERNS = ("all", "none", "first", "last", "tile_first", "tile_last", "alternating", "hash_half")


def keep_pattern(name, n):
    i = np.arange(n, dtype=np.int64)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "tile_first":
        return i % CP_TILE == 0
    if name == "tile_last":
        return (i % CP_TILE == CP_TILE - 1) | (i == n - 1)
    if name == "alternating":
        return i % 2 == 1
    if name == "hash_half":
        h = (i * 2654435761 + 12345) & 0xffffffff
        return ((h ^ (h >> 15)) * 2246822519 & 0xffffffff) >> 31 == 1
    raise ValueError(name)


# rows of PRED_LIM / CRT_DYADIC (below) that every predicate keeps (u = 64 - 60 y/x in (0, 124), v in (0, 108), a2 = x > 0) or
# that the range test drops (z on its upper limit); a kept row's x carries its index modulo 8 so that a misplaced row shows
def pattern_rows(keep):
    n = keep.shape[0]
    p = np.empty((n, 3), dtype=F32)
    i = np.arange(n)
    p[:, 0] = 2.0 + (i % 8) * 0.5
    p[:, 1] = np.where(i % 3 == 0, 0.5, -0.25)
    p[:, 2] = np.where(keep, 0.25, 1.0)
    return p


# ---------------------------------------------------------------------------------------------------------------- voxeliser
COMPAT, ACCUM, COMPAT_ROUNDS, OCCUPANCY = 0, 1, 2, 3
VOX_DIMS = (32, 64, 32)                                                # Cz, L, W
VOX_AFF = np.array([4.0, 0.0, 4.0, 16.0, 8.0, 20.0], dtype=F32)        # fx = 4 x, fy = 4 y + 16, fz = 8 z + 20
# more than one cell of margin on every upper side (one cell exactly would not do: the last float below y = 3.75 has
# 4 y + 16 = 31 - 2^-20, a tie that rounds to 31.0)
VOX_LIM = np.array([0.0, 15.5, -4.0, 3.5, -2.5, 1.25], dtype=F32)
# no margin: xl = 63, yl = 31, zl = 31 are reachable.  (The y and z limits stay 1/64 m short of 4 and 1.5: the last float below
# y = 4 has 4 y + 16 = 32 - 2^-20, a tie that rounds to 32.0 -- a CELL outside the grid, which the entries refuse.)
VOX_LIM_TIGHT = np.array([0.0, 16.0, -4.0, 3.984375, -2.5, 1.484375], dtype=F32)


def vox_inside(v, nvox):
    return 0 <= v < nvox


def voxel_corners(row, aff, dims, exact_log=None):
    """The eight (flat index, weight) pairs of one point, in pass order c = z-bit | x-bit << 1 | y-bit << 2 -- the chain
    f = fl(fl(p s) + o), trunc, d = f - floor, a = 1 - d, w = fl(fl(wx wy) wz)."""
    Cz, L, W = dims
    a = [frac(v) for v in np.asarray(aff, dtype=F32)]
    f = [fl32(fl32(frac(row[k]) * a[2 * k], exact_log) + a[2 * k + 1], exact_log) for k in range(3)]
    lo = [int(v) for v in f]                                           # trunc toward zero, like (int)
    d = [fl32(f[k] - lo[k], exact_log) for k in range(3)]
    w1 = [fl32(1 - d[k], exact_log) for k in range(3)]
    out = []
    for c in range(8):
        ez, ex, ey = c & 1, (c >> 1) & 1, (c >> 2) & 1
        wx, wy, wz = (d[0] if ex else w1[0]), (d[1] if ey else w1[1]), (d[2] if ez else w1[2])
        out.append((((lo[2] + ez) * L + lo[0] + ex) * W + lo[1] + ey, fl32(fl32(wx * wy, exact_log) * wz, exact_log)))
    return out


def voxelize(pts, lim, aff, dims, mode, exact_log=None):
    """Sparse grid {flat index: Fraction} of the voxeliser in `mode`; a corner whose flat index is outside [0, nvox) contributes
    nothing.  COMPAT (and COMPAT_ROUNDS: the same statement) is eight literal passes, in each of which every point reads the
    grid as the pass found it and the LAST point (highest index) that writes a voxel wins."""
    Cz, L, W = dims
    nvox = Cz * L * W
    p = np.asarray(pts, dtype=F32).reshape(-1, 3)
    rows = np.flatnonzero(in_range(p, lim))
    cor = [voxel_corners(p[i], aff, dims, exact_log) for i in rows]
    grid = {}
    if mode == OCCUPANCY:
        for c8 in cor:
            if vox_inside(c8[0][0], nvox):
                grid[c8[0][0]] = Fraction(1)
    elif mode == ACCUM:
        for c8 in cor:
            for v, w in c8:
                if vox_inside(v, nvox):
                    grid[v] = grid.get(v, Fraction(0)) + w             # an exact sum: no order
    else:
        for c in range(8):
            wrote = {}
            for c8 in cor:                                             # ascending point index: the last assignment stays
                v, w = c8[c]
                if vox_inside(v, nvox):
                    wrote[v] = fl32(grid.get(v, Fraction(0)) + w, exact_log)
            grid.update(wrote)
    return grid


def dense_grid(grid, dims):
    """fp32 [Cz,L,W] of a sparse grid (every value must be an fp32 number: asserted)."""
    out = np.zeros(dims[0] * dims[1] * dims[2], dtype=F32)
    for v, q in grid.items():
        assert is_f32(q), "voxel %d: %s is not an fp32 value" % (v, q)
        out[v] = F32(float(q))
    return out.reshape(dims)


def grid_nhwc(grid_f32, tdt):
    """[Cz,L,W] fp32 -> [L,W,Cz] of the torch dtype, one round-to-nearest-even store (the rounding of _elementwise_ref)."""
    return cast_statement(torch.from_numpy(np.ascontiguousarray(np.transpose(grid_f32, (1, 2, 0)))), tdt)


def voxel_cell_range(lim, aff, dims):
    """The arithmetic of the entries' host-side check: (lowest, highest flat CELL index an accepted point can reach, accepted?)
    -- the chain at the first float above each lower limit and the last float below each upper one, both ends per axis."""
    Cz, L, W = dims
    lim, aff = np.asarray(lim, dtype=F32), np.asarray(aff, dtype=F32)
    if not (np.isfinite(lim).all() and np.isfinite(aff).all()):
        return None, None, False
    lo, hi = [], []
    for ax in range(3):
        p0, p1 = nxt(lim[2 * ax], True), nxt(lim[2 * ax + 1], False)
        if not p0 <= p1:
            return 0, 0, True
        c = [int(fl32(fl32(frac(p) * frac(aff[2 * ax])) + frac(aff[2 * ax + 1]))) for p in (p0, p1)]
        lo.append(min(c)); hi.append(max(c))
    lo_flat = (lo[2] * L + lo[0]) * W + lo[1]
    hi_flat = (hi[2] * L + hi[0]) * W + hi[1]
    return lo_flat, hi_flat, lo_flat >= 0 and hi_flat < Cz * L * W


def voxel_max_corner(lim, aff, dims):
    """Highest flat index of any CORNER of an accepted point (cell + (L + 1) W + 1 at the upper ends)."""
    _, hi, _ = voxel_cell_range(lim, aff, dims)
    return hi + (dims[1] + 1) * dims[2] + 1


# ---------------------------------------------------------------------------------------------------------------- BEV KNN
KNN_CELLS = (104, 88)                                                  # stride-1 cells: x in [0, 13) m, y in [-8, 3) m
KNN_AFF = np.array([8.0, 0.0, 8.0, 64.0], dtype=F32)                   # xs, xo, ys, yo
KNN_STRIDES = (2, 4, 8, 16)
KNN_UNIT = 8                                                           # coordinates are multiples of 1/8 m, d2 of 1/64 m^2


def knn_site(stride):
    return KNN_CELLS[0] // stride, KNN_CELLS[1] // stride


def knn_d2(xyz, h, w, stride, aff=KNN_AFF):
    """Integer squared distances [h*w, n] in units of 1/64 m^2 between the pixel centres ((i + 0.5) s - o) / scale and the points
    (x, y); every coordinate must be a multiple of 1/8 m (asserted)."""
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    P = np.rint(p[:, :2] * KNN_UNIT).astype(np.int64)
    assert np.array_equal(P.astype(np.float64) / KNN_UNIT, p[:, :2]), "KNN statement: points must be multiples of 1/8 m"
    xs, xo, ys, yo = (int(v) for v in aff)
    assert KNN_UNIT % xs == 0 or xs % KNN_UNIT == 0
    X = [Fraction((2 * i + 1) * stride - 2 * xo, 2 * xs) * KNN_UNIT for i in range(h)]
    Y = [Fraction((2 * j + 1) * stride - 2 * yo, 2 * ys) * KNN_UNIT for j in range(w)]
    assert all(q.denominator == 1 for q in X + Y), "KNN statement: pixel centres must be multiples of 1/8 m"
    X, Y = np.array([int(q) for q in X], dtype=np.int64), np.array([int(q) for q in Y], dtype=np.int64)
    dx = P[None, :, 0] - X[:, None]                                    # [h, n]
    dy = P[None, :, 1] - Y[:, None]                                    # [w, n]
    return ((dx * dx)[:, None, :] + (dy * dy)[None, :, :]).reshape(h * w, P.shape[0])


def knn_rmax2_units(rmax):
    """What the wrappers pass: fl(fl(rmax)^2), here in units of 1/64 m^2 as an exact Fraction (None = no cut)."""
    if rmax is None:
        return None
    return frac(F32(F32(rmax) * F32(rmax))) * KNN_UNIT * KNN_UNIT


def knn_bev(xyz, K, h, w, stride, rmax=None, aff=KNN_AFF):
    """int32 [K,h,w]: the K smallest (d2, index), d2 <= rmax^2 inclusive, -1 where there are fewer."""
    n = np.asarray(xyz).reshape(-1, 3).shape[0]
    out = np.full((h * w, K), -1, dtype=np.int32)
    if n:
        d2 = knn_d2(xyz, h, w, stride, aff)
        key = d2 * n + np.arange(n, dtype=np.int64)[None, :]           # (d2, index) as one integer
        order = np.argsort(key, axis=1, kind="stable")[:, :K]
        best = np.take_along_axis(d2, order, axis=1)
        ok = np.ones_like(best, dtype=bool)
        r2 = knn_rmax2_units(rmax)
        if r2 is not None:
            ok = best <= (r2.numerator // r2.denominator)              # integer d2 <= r2  <=>  d2 <= floor(r2)
        kk = min(K, n)
        out[:, :kk] = np.where(ok, order, -1)[:, :kk]
    return np.ascontiguousarray(out.T.reshape(K, h, w))


def knn_tie_census(xyz, h, w, stride, kmax=8):
    """For K = 1 .. kmax: the fraction of pixels whose ranks K and K+1 hold the same d2 (a kernel that forgets the index there
    may return either point)."""
    d2 = np.sort(knn_d2(xyz, h, w, stride), axis=1)
    return [float((d2[:, k - 1] == d2[:, k]).mean()) for k in range(1, kmax + 1)]


def lattice_cloud(seed=7):
    """Every 1/4 m from x = 1 .. 11 and y = -7 .. 2 (41 x 37 = 1517 points), z a dyadic ramp, index order permuted."""
    xs, ys = np.arange(4, 45) * 0.25, np.arange(-28, 9) * 0.25
    g = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([g, ((np.arange(g.shape[0]) % 16) * 0.125 - 1.0)[:, None]], 1).astype(F32)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])])


def sparse_cloud(seed=8):
    """3 m spacing, phased so that the bisectors between neighbouring points run through stride-2 pixel centres: most pixels find
    the cells around them empty, the block rings decide, and whole rows and columns of pixels see two points (in different 8 x 8
    blocks) at the same d2."""
    g = np.stack(np.meshgrid(np.arange(1.125, 12, 3.0), np.arange(-6.875, 3, 3.0), indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([g, np.zeros((g.shape[0], 1))], 1).astype(F32)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])])


def border_cloud(seed=9):
    """Points on cell borders (multiples of 1/8 m = stride-1 cell edges, and of the coarser strides' edges), on the site's outer
    border, and up to three stride-1 cells outside it on each side (the cell sort clamps those into the border cells)."""
    rows = []
    for x in (0.0, 0.125, 2.0, 4.0, 6.0, 12.875, 13.0):                # site: x in [0, 13], y in [-8, 3]
        for y in (-8.0, -7.875, -6.0, -4.0, 0.0, 2.875, 3.0):
            rows.append((x, y))
    for t in (1, 2, 3):                                                # outside, every side and the corners
        o = t * 0.125
        rows += [(-o, -2.0), (13.0 + o, -2.0), (5.0, -8.0 - o), (5.0, 3.0 + o), (-o, -8.0 - o), (13.0 + o, 3.0 + o),
                 (-o, 3.0 + o), (13.0 + o, -8.0 - o)]
    p = np.array([(x, y, 0.0) for x, y in rows], dtype=F32)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])])


def radius_cloud():
    """Around the stride-2 pixel centre (3.125, -1.875): offsets whose d2 is 16/64 (= 0.5^2), 25/64 (= 0.625^2, by (3/8, 4/8)) and
    26/64 (just past it); the lattice is added by the caller's choice."""
    cx, cy = 3.125, -1.875
    offs = [(0.375, 0.5), (-0.5, 0.375), (0.5, 0.0), (0.0, -0.5), (0.625, 0.0), (0.625, 0.125), (0.125, 0.625), (0.0, 0.0)]
    return np.array([(cx + a, cy + b, 0.0) for a, b in offs], dtype=F32)


# ---------------------------------------------------------------------------------------------------------------- edge inputs
# Family A.  Limits, image bounds and rows of the predicate cases.  With CRT_DYADIC a row (x, y, z) has a0 = 64 x - 60 y,
# a1 = 48 x - 60 z, a2 = x; the base row (4, -1, 0) sits on u = 79, v = 48.  Image bounds 124 x 108: (1, -1, 0) has u = 124 and
# (1, 0, -1) has v = 108 exactly, and one ulp-pair of y (z) away a0 (a1) ROUNDS onto the fp32 neighbours of 124 (108).
# (1.875, 2, 0) has a0 = 0 and (0.625, 0, 0.5) has a1 = 0 exactly; their y (z) neighbours give the nearest attainable u (v) on
# either side of zero, exactly.
PRED_ULIM, PRED_VLIM = 124.0, 108.0
PRED_LIM = np.array([0.5, 16.0, -4.0, 4.0, -2.0, 1.0], dtype=F32)
PRED_LIM_DEPTH = np.array([-16.0, 16.0, -4.0, 4.0, -2.0, 1.0], dtype=F32)      # admits x <= 0: a2 == 0 and a2 < 0


def predicate_cases():
    """-> {group: (lim, rows [n,3] fp32, tags)}; tags[i] = (what, where, rounds): what in x/y/z (a range limit), u/v (an image
    bound: where = (bound, at / inside / outside)), depth, special; rounds = the chain of the row is NOT exact (the contract's roundings decide)."""
    base = (4.0, -1.0, 0.0)
    rows, tags = [], []

    def add(row, what, where, rounds=False):
        rows.append(tuple(F32(v) for v in row)); tags.append((what, where, rounds))

    add(base, "special", "base")
    for ax, name in enumerate("xyz"):
        for side in (0, 1):
            l = PRED_LIM[2 * ax + side]
            for where, val in (("at", l), ("outside", nxt(l, side == 1)), ("inside", nxt(l, side == 0))):
                r = list(((0.0, 0.25, 0.0), (8.0, 0.0, 0.0), base)[ax]); r[ax] = val      # (u, v stay well inside the image)
                add(r, name, (side, where), rounds=(where == "inside"))
    e = F32(2.0 ** -23)
    for where, y in (("at", -1.0), ("outside", F32(-1.0) - e), ("inside", F32(-1.0) + e)):
        add((1.0, y, 0.0), "u", (PRED_ULIM, where), rounds=(where != "at"))
    for where, z in (("at", -1.0), ("outside", F32(-1.0) - e), ("inside", F32(-1.0) + e)):
        add((1.0, 0.0, z), "v", (PRED_VLIM, where), rounds=(where != "at"))
    for where, y in (("at", 2.0), ("outside", nxt(2.0, True)), ("inside", nxt(2.0, False))):
        add((1.875, y, 0.0), "u", (0.0, where))
    for where, z in (("at", 0.5), ("outside", nxt(0.5, True)), ("inside", nxt(0.5, False))):
        add((0.625, 0.0, z), "v", (0.0, where))
    inf, nan = np.inf, np.nan
    for r in ((4.0, -0.0, -0.0), (inf, inf, inf), (4.0, inf, 0.0), (4.0, -1.0, -inf), (-inf, 0.0, 0.0), (nan, nan, nan), (4.0, nan, 0.0),
              (4.0, -1.0, nan), (nan, -1.0, 0.0)):
        add(r, "special", "nonfinite-or-negzero")
    add(base, "special", "base")
    out = {"limits": (PRED_LIM, np.array(rows, dtype=F32), tags)}
    rows, tags = [], []
    add(base, "special", "base")
    for r in ((0.0, 1.0, 0.0), (0.0, -1.0, -0.5), (-0.0, -1.0, -0.5), (0.0, 0.0, 0.0)):
        add(r, "depth", "zero")
    for r in ((-4.0, 1.0, 0.0), (-1.0, 0.25, 0.5), (-8.0, 2.0, 0.0)):                  # u = 79 / 79 / 79, v = 48 / 78 / 48: inside
        add(r, "depth", "negative")
    add((-4.0, -1.0, 0.0), "depth", "negative-outside")                                # u = 49 ... still inside; v = 48
    add(base, "special", "base")
    out["depth"] = (PRED_LIM_DEPTH, np.array(rows, dtype=F32), tags)
    return out


def frame_crt(b):
    """Per-frame matrices of the batch cases: u_b = u + b (a0 = (64 + b) x - 60 y), small integers."""
    c = CRT_DYADIC.copy()
    c[:, 0] += F32(b) * c[:, 2]
    return c


# Family B sizes: around one compaction tile (1024 rows), and around 256 tiles (the single-block scan's carry loop: 256 block sums
# per trip) and one tile more
COMPACT_SIZES = (1, 2, 1023, 1024, 1025, 2048, 262143, 262144, 262145, 263169)
BATCH_FRAMES = ((1025, "hash_half"), (0, "none"), (1, "all"), (1023, "tile_last"), (2048, "alternating"), (1024, "none"),
                (3000, "tile_first"), (2, "last"))


# Family C clouds on the dyadic grid (points are multiples of 1/32 m).
def voxel_clouds():
    """-> {name: (pts [n,3] fp32, lim)}."""
    rng = np.random.default_rng(11)
    out = {}
    out["integer"] = (np.array([(1.0, 0.5, -1.0), (2.25, -3.75, 0.125), (15.25, 3.25, 1.125), (0.25, -3.75, -2.375), (7.0, 0.0, 0.0)], dtype=F32), VOX_LIM)
    out["half"] = (np.array([(1.125, 0.625, -0.9375), (9.875, -2.125, 0.6875), (15.375, 3.375, 1.1875), (0.125, -3.875, -2.4375)], dtype=F32), VOX_LIM)
    k = rng.integers(0, 32, size=(500, 3))                     # 500 points of the cell (xl, yl, zl) = (20, 18, 12), duplicates included
    one = np.stack([5.0 + (k[:, 0] % 8) / 32.0, 0.5 + (k[:, 1] % 8) / 32.0, -1.0 + (k[:, 2] % 4) / 32.0], 1)
    out["one_cell"] = (np.ascontiguousarray(one[rng.permutation(500)], dtype=F32), VOX_LIM)
    k = rng.integers(0, 192, size=(1300, 3))                   # a block of 6 x 6 x 6 cells, ~6 points per cell: shared voxels
    nb = np.stack([8.0 + (k[:, 0] % 48) / 32.0, -1.0 + (k[:, 1] % 48) / 32.0, 0.0 + (k[:, 2] % 24) / 32.0], 1)
    out["neighbours"] = (np.ascontiguousarray(nb, dtype=F32), VOX_LIM)
    # the last cell of each axis under limits without margin: yl = 31 wraps into the next row, xl = 63 into the next plane, and
    # in the last plane (zl = 31, or zl = 30 with xl = 63) the upper corners leave the grid
    last = [(15.78125, 0.5, 0.0), (5.0, 3.78125, 0.0), (5.0, 0.5, 1.40625), (15.78125, 3.78125, 0.0), (15.78125, 0.5, 1.40625),
            (5.0, 3.78125, 1.40625), (15.78125, 3.78125, 1.40625), (15.96875, 3.96875, 1.46875), (15.96875, 3.96875, 1.34375),
            (15.75, 3.75, 1.375), (15.78125, 3.78125, 1.28125), (0.03125, -3.96875, -2.46875)]
    k = rng.integers(0, 8, size=(60, 3))
    more = np.stack([15.75 + k[:, 0] / 32.0, 3.75 + k[:, 1] / 32.0, 1.25 + (k[:, 2] % 8) / 32.0], 1)
    out["last_cells"] = (np.ascontiguousarray(np.concatenate([np.array(last), more]), dtype=F32), VOX_LIM_TIGHT)
    return out


def tiny_grid_cloud(lim):
    """The tiny golden grid (32 x 64 x 32, aff 4,0,4,16,10,24, z < 0.6f): the last two floats below the z limit give fz == 30.0
    (the chain rounds up), and with xl == 63 the corners (zl + 1, xl + 1, .) lie past the last voxel."""
    z1 = nxt(lim[5], False)
    z2 = nxt(z1, False)
    rows = [(15.75, 0.5, z1), (15.78125, 3.78125, z1), (15.78125, 3.75, z2), (15.75, 3.78125, z2), (15.78125, 0.53125, z2),
            (15.5, 3.78125, z1), (15.78125, 3.78125, 0.5), (2.0, 0.5, z1), (15.78125, 3.78125, z1)]
    return np.array(rows, dtype=F32)


REFUSED_GRIDS = {                                              # hand-made: the LOWER corner leaves the grid
    "x_below": (np.array([-0.5, 15.5, -4.0, 3.5, -2.5, 1.25], dtype=F32), VOX_AFF, VOX_DIMS),         # fx > -2: xl = -1 at z = y = 0
    "z_above": (np.array([0.0, 15.5, -4.0, 3.5, -2.5, 1.625], dtype=F32), VOX_AFF, VOX_DIMS),         # fz < 33: zl = 32
}

"""CPU only: the statements of tests/_geometry_ref.py on their own -- the conditions under which the edge inputs test anything,
the statements against the C oracle on the same inputs, and the arithmetic of the voxeliser's host-side grid check."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import _geometry_ref as R
from _util import golden_cfg, load_golden
from oracle import geometry_ref

F32 = np.float32
MODE_NAME = {R.COMPAT: "compat", R.ACCUM: "accum", R.OCCUPANCY: "occupancy"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the helper
def test_fl32_is_round_to_nearest_even():
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-30, 30, 2000), [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24,
                           1 + 2.0 ** -24 + 2.0 ** -40, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -127 + 2.0 ** -150, 0.0, -0.1]])
    for v in vals:
        assert R.fl32(Fraction(float(v))) == Fraction(float(F32(v))), v      # numpy's float64 -> float32 is one correct rounding
    assert R.is_f32(Fraction(3, 512)) and not R.is_f32(Fraction(1, 3)) and not R.is_f32(1 + Fraction(1, 2 ** 24))


# ---------------------------------------------------------------------------------------------------------------- family A
def test_predicate_rows_sit_on_their_boundaries_and_are_exact():
    cases = R.predicate_cases()
    for group, (lim, rows, tags) in cases.items():
        rng = R.in_range(rows, lim)
        for i, (what, where, rounds) in enumerate(tags):
            row = rows[i]
            if what in "xyz":
                ax, (side, pos) = "xyz".index(what), where
                l = lim[2 * ax + side]
                want = {"at": l, "outside": R.nxt(l, side == 1), "inside": R.nxt(l, side == 0)}[pos]
                assert row[ax] == want and bool(rng[i]) == (pos == "inside"), (group, i)
            if not (np.isfinite(row).all() and rng[i]):
                continue
            log = []
            keep0, u, v = R._keep_uv_row(row, R.CRT_DYADIC, R.PRED_ULIM, R.PRED_VLIM, 0, log)
            keep1, _, _ = R._keep_uv_row(row, R.CRT_DYADIC, R.PRED_ULIM, R.PRED_VLIM, 1)
            assert all(log) != rounds, "%s row %d %s: chain exact = %s, declared rounding = %s" % (group, i, row, all(log), rounds)
            if what in "uv":
                got, (bound, pos) = (u if what == "u" else v), where
                if pos == "at":
                    assert got == F32(bound) and not keep0
                elif bound == 0.0:                   # nearest attainable values on either side of zero, exactly
                    assert (got > 0) == (pos == "inside") and got != 0 and abs(float(got)) <= 2.0 ** -15 and keep0 == (pos == "inside")
                else:                                # the fp32 neighbours of the bound
                    assert got == R.nxt(bound, pos == "outside") and keep0 == (pos == "inside")
            if what == "depth":
                a2 = R.proj_chain(row, R.CRT_DYADIC)[2]
                if where == "zero":
                    assert a2 == 0 and not keep0 and not keep1
                else:
                    assert a2 < 0 and keep0 and not keep1 and 0 < u < R.PRED_ULIM and 0 < v < R.PRED_VLIM
            if what in "xyz" or where == "base":
                assert keep0 and keep1
    lim, rows, tags = cases["limits"]
    assert sum(1 for t in tags if t[0] in "xyz") == 18 and sum(1 for t in tags if t[0] in "uv") == 12
    assert np.isnan(rows).any() and np.isinf(rows).any() and (np.signbit(rows) & (rows == 0)).any()


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_pattern_rows_follow_their_pattern(pattern):
    for n in (1, 2, 1025, 3000):
        want = R.keep_pattern(pattern, n)
        rows = R.pattern_rows(want)
        assert np.array_equal(R.in_range(rows, R.PRED_LIM), want)
        for b in (0, 7):
            for mode in (0, 1):
                log = []
                keep, _ = R.project_keep(rows, R.PRED_LIM, R.frame_crt(b), R.PRED_ULIM, R.PRED_VLIM, mode, log)
                assert np.array_equal(keep, want) and all(log)
    n = 263169
    frac_kept = R.keep_pattern("hash_half", n).mean()
    assert 0.49 < frac_kept < 0.51
    assert R.keep_pattern("tile_first", n).sum() == 258 and R.keep_pattern("tile_last", n).sum() == 258


def test_predicates_agree_with_the_c_oracle():
    for group, (lim, rows, tags) in R.predicate_cases().items():
        pin, src, m = R.range_filter(rows, lim)
        o_in, o_src = geometry_ref.range_filter(rows, lim)
        assert m == o_src.shape[0] and np.array_equal(src, o_src) and np.array_equal(_bits(pin), _bits(o_in)), group
        for mode in (0, 1):
            uv, xyz, psrc, pm = R.project_filter(rows, lim, R.CRT_DYADIC, R.PRED_ULIM, R.PRED_VLIM, mode)
            o_uv, o_xyz, o_s = geometry_ref.project(o_in, R.CRT_DYADIC, R.PRED_ULIM, R.PRED_VLIM, "compat" if mode == 0 else "correct")
            assert pm == o_uv.shape[0] and np.array_equal(psrc, o_src[o_s]), (group, mode)
            assert np.array_equal(_bits(uv), _bits(o_uv)) and np.array_equal(_bits(xyz), _bits(o_xyz)), (group, mode)
    want = R.keep_pattern("hash_half", 5000)
    rows = R.pattern_rows(want)
    o_in, o_src = geometry_ref.range_filter(rows, R.PRED_LIM)
    uv, xyz, psrc, pm = R.project_filter(rows, R.PRED_LIM, R.frame_crt(3), R.PRED_ULIM, R.PRED_VLIM, 1)
    o_uv, o_xyz, o_s = geometry_ref.project(o_in, R.frame_crt(3), R.PRED_ULIM, R.PRED_VLIM, "correct")
    assert np.array_equal(psrc, o_src[o_s]) and np.array_equal(_bits(uv), _bits(o_uv)) and np.array_equal(_bits(xyz), _bits(o_xyz))


# ---------------------------------------------------------------------------------------------------------------- family C
def _tiny():
    g = geometry_ref.grid_constants(golden_cfg(load_golden("model_tiny.npz")))
    return g["lim"], g["aff"], g["dims"]


def test_voxel_clouds_are_exact_and_reach_their_edges():
    nvox = R.VOX_DIMS[0] * R.VOX_DIMS[1] * R.VOX_DIMS[2]
    clouds = R.voxel_clouds()
    for name, (pts, lim) in clouds.items():
        assert np.array_equal(pts * 32, np.rint(pts * 32)), name               # multiples of 1/32 m
        assert R.in_range(pts, lim).all(), name
        for mode in (R.COMPAT, R.ACCUM, R.OCCUPANCY):
            log = []
            R.dense_grid(R.voxelize(pts, lim, R.VOX_AFF, R.VOX_DIMS, mode, log), R.VOX_DIMS)       # (asserts fp32 values)
            assert all(log), (name, mode)
        for row in pts:
            for v, w in R.voxel_corners(row, R.VOX_AFF, R.VOX_DIMS):
                assert (w * 512).denominator == 1
    for row in clouds["integer"][0]:
        assert sorted(w for _, w in R.voxel_corners(row, R.VOX_AFF, R.VOX_DIMS)) == [0] * 7 + [1]
    for row in clouds["half"][0]:
        assert [w for _, w in R.voxel_corners(row, R.VOX_AFF, R.VOX_DIMS)] == [Fraction(1, 8)] * 8
    cells = {R.voxel_corners(r, R.VOX_AFF, R.VOX_DIMS)[0][0] for r in clouds["one_cell"][0]}
    assert len(cells) == 1 and clouds["one_cell"][0].shape[0] == 500
    cells = [R.voxel_corners(r, R.VOX_AFF, R.VOX_DIMS)[0][0] for r in clouds["neighbours"][0]]
    assert len(set(cells)) == 216 and len(cells) > 5 * 216
    # compat differs from accum exactly where several points share a voxel
    for name in ("one_cell", "neighbours"):
        pts, lim = clouds[name]
        assert R.voxelize(pts, lim, R.VOX_AFF, R.VOX_DIMS, R.COMPAT) != R.voxelize(pts, lim, R.VOX_AFF, R.VOX_DIMS, R.ACCUM)
    # the bf16 store rounds: sums over the eight passes that are no bf16 numbers (a sum of weights k/256 below 2 has up to nine
    # significant bits; f16's eleven hold every one of them) -- eight such voxels are asked for, enough to tell a truncating store
    g = R.dense_grid(R.voxelize(*clouds["one_cell"], R.VOX_AFF, R.VOX_DIMS, R.COMPAT), R.VOX_DIMS)
    g2 = R.dense_grid(R.voxelize(*clouds["neighbours"], R.VOX_AFF, R.VOX_DIMS, R.COMPAT), R.VOX_DIMS)
    for tdt in (torch.bfloat16, torch.float16):
        back = R.grid_nhwc(g, tdt).float().numpy().transpose(2, 0, 1)
        back2 = R.grid_nhwc(g2, tdt).float().numpy().transpose(2, 0, 1)
        assert (back2 != g2).sum() >= (8 if tdt == torch.bfloat16 else 0), tdt
    # the last cells: the documented flat wrap (kept) and the corners past the last voxel (dropped)
    pts, lim = clouds["last_cells"]
    Cz, L, W = R.VOX_DIMS
    wraps = outside = 0
    for row in pts:
        c8 = R.voxel_corners(row, R.VOX_AFF, R.VOX_DIMS)
        cell = c8[0][0]
        yl, xl = cell % W, (cell // W) % L
        assert 0 <= cell < nvox
        wraps += int(yl == W - 1 or xl == L - 1)
        outside += sum(1 for v, _ in c8 if v >= nvox)
    assert wraps >= 10 and outside >= 20
    assert max(v for row in pts for v, _ in R.voxel_corners(row, R.VOX_AFF, R.VOX_DIMS)) == nvox - 1 + (L + 1) * W + 1       # (zl+1, xl+1, yl+1) of the very last cell
    assert R.voxel_max_corner(lim, R.VOX_AFF, R.VOX_DIMS) - (nvox - 1) == (L + 1) * W + 1                   # the unfixed code's largest overshoot


def test_tiny_grid_cloud_reaches_past_the_grid():
    lim, aff, dims = _tiny()
    Cz, L, W = dims
    nvox = Cz * L * W
    pts = R.tiny_grid_cloud(lim)
    assert R.in_range(pts, lim).all()
    z1 = R.nxt(lim[5], False)
    for z in (z1, R.nxt(z1, False)):
        c8 = R.voxel_corners((F32(15.75), F32(0.5), z), aff, dims)
        assert c8[0][0] // (L * W) == 30 and c8[1][1] == 0                 # fz == 30.0: zl = 30, dz = 0
    assert R.voxel_corners((F32(15.75), F32(0.5), R.nxt(R.nxt(z1, False), False)), aff, dims)[0][0] // (L * W) == 29
    top = max(v for row in pts for v, _ in R.voxel_corners(row, aff, dims))
    assert top == nvox + W == 65568
    assert sum(1 for row in pts for v, _ in R.voxel_corners(row, aff, dims) if v >= nvox) >= 12


def test_voxeliser_agrees_with_the_c_oracle():
    cases = [(name, pts, lim, R.VOX_AFF, R.VOX_DIMS) for name, (pts, lim) in R.voxel_clouds().items()]
    lim, aff, dims = _tiny()
    cases.append(("tiny", R.tiny_grid_cloud(lim), lim, aff, dims))
    for name, pts, lim, aff, dims in cases:
        pin, _ = geometry_ref.range_filter(pts, lim)
        for mode in (R.COMPAT, R.ACCUM, R.OCCUPANCY):
            want = R.dense_grid(R.voxelize(pts, lim, aff, dims, mode), dims)
            got = geometry_ref.voxelize(pin, aff, dims, MODE_NAME[mode])
            assert np.array_equal(_bits(got), _bits(want)), (name, mode)


# ---------------------------------------------------------------------------------------------------------------- the grid check
def _grid(cfg_update=None, name="geometry_carla.npz"):
    cfg = golden_cfg(load_golden(name))
    cfg.update(cfg_update or {})
    g = geometry_ref.grid_constants(cfg)
    return g["lim"], g["aff"], g["dims"]


def test_grid_check_arithmetic():
    kitti = dict(voxel_length=704, voxel_width=800, lidar_x_max=70.4, lidar_y_min=-40.0, lidar_y_max=40.0)
    for what, (lim, aff, dims), top in (("carla", _grid(), 3137008), ("kitti", _grid(kitti), 18021598), ("tiny", _tiny(), 65568)):
        nvox = dims[0] * dims[1] * dims[2]
        lo, hi, ok = R.voxel_cell_range(lim, aff, dims)
        assert ok and 0 <= lo <= hi < nvox, what
        assert R.voxel_max_corner(lim, aff, dims) == top, what
        assert (top >= nvox) == (what == "tiny")
    lo, hi, ok = R.voxel_cell_range(R.VOX_LIM, R.VOX_AFF, R.VOX_DIMS)
    assert ok and hi + (R.VOX_DIMS[1] + 1) * R.VOX_DIMS[2] + 1 < 65536
    lo, hi, ok = R.voxel_cell_range(R.VOX_LIM_TIGHT, R.VOX_AFF, R.VOX_DIMS)
    assert ok and (lo, hi) == (0, 65535)
    lo, hi, ok = R.voxel_cell_range(*R.REFUSED_GRIDS["x_below"])
    assert not ok and lo == -32 and hi < 65536
    lo, hi, ok = R.voxel_cell_range(*R.REFUSED_GRIDS["z_above"])
    assert not ok and lo == 0 and hi == (33 * 64 + 61) * 32 + 30         # (the last floats below 1.625 and 3.5 round up to fz = 33.0, fy = 30.0)
    bad = R.VOX_LIM.copy(); bad[3] = np.inf
    assert R.voxel_cell_range(bad, R.VOX_AFF, R.VOX_DIMS)[2] is False
    bad = R.VOX_AFF.copy(); bad[4] = np.nan
    assert R.voxel_cell_range(R.VOX_LIM, bad, R.VOX_DIMS)[2] is False
    neg = np.array([-4.0, 64.0, 4.0, 16.0, 8.0, 20.0], dtype=F32)           # a negative scale: both ends are taken
    assert R.voxel_cell_range(R.VOX_LIM, neg, R.VOX_DIMS)[:2] == ((0 * 64 + 2) * 32 + 0, (30 * 64 + 64) * 32 + 30)     # (fx = 64 - 4 x rounds to 64.0 at the first float above x = 0)


# ---------------------------------------------------------------------------------------------------------------- family D
def test_lattice_cloud_tie_census():
    xyz = R.lattice_cloud()
    assert xyz.shape == (1517, 3) and len({tuple(r[:2]) for r in xyz.tolist()}) == 1517
    for s in R.KNN_STRIDES:
        h, w = R.knn_site(s)
        assert int(R.knn_d2(xyz, h, w, s).max()) < 2 ** 14                  # exact in fp32 whatever the order of the two squares
        census = R.knn_tie_census(xyz, h, w, s)
        assert sum(1 for f in census if f > 0.5) >= 5, (s, census)
    assert [R.knn_site(s) for s in R.KNN_STRIDES] == [(52, 44), (26, 22), (13, 11), (6, 5)]


def test_knn_clouds_reach_their_edges():
    sp = R.sparse_cloud()
    h, w = R.knn_site(2)
    d2 = np.sort(R.knn_d2(sp, h, w, 2), axis=1)
    assert float((d2[:, 0] > 6 * 6).mean()) > 0.5                          # most pixels: nothing within 3/4 m (three stride-2 pixels) ...
    assert float((d2[:, 0] == d2[:, 1]).mean()) > 0.02 and float((d2[:, 1] == d2[:, 2]).mean()) > 0.02   # ... and ties decide
    bc = R.border_cloud()
    x, y = bc[:, 0], bc[:, 1]
    assert (x < 0).sum() >= 6 and (x > 13).sum() >= 6 and (y < -8).sum() >= 6 and (y > 3).sum() >= 6
    assert x.min() == -0.375 and x.max() == 13.375 and y.min() == -8.375 and y.max() == 3.375
    assert ((x == 0) | (x == 13) | (y == -8) | (y == 3)).sum() >= 20
    rc = R.radius_cloud()
    pix = (12 * 44 + 24)                                                   # stride 2: centre ((2*12+1)/8, (2*24+1-64)/8) = (3.125, -1.875)
    row = np.sort(R.knn_d2(rc, h, w, 2)[pix])
    assert row.tolist() == [0, 16, 16, 25, 25, 25, 26, 26]
    assert R.knn_rmax2_units(0.625) == 25 and R.knn_rmax2_units(0.5) == 16 and R.knn_rmax2_units(0.0) == 0
    got = R.knn_bev(rc, 8, h, w, 2, rmax=0.625).reshape(8, -1)[:, pix]
    assert (got >= 0).sum() == 6 and got[6] == -1                           # the three at 25/64 are kept, the two at 26/64 are not
    assert (R.knn_bev(rc, 8, h, w, 2, rmax=0.0).reshape(8, -1)[:, pix] >= 0).sum() == 1


@pytest.mark.parametrize("stride", R.KNN_STRIDES)
def test_knn_statement_agrees_with_the_c_oracle(stride):
    h, w = R.knn_site(stride)
    aff = R.KNN_AFF
    lat = R.lattice_cloud()
    for K in (1, 3, 8):
        assert np.array_equal(R.knn_bev(lat, K, h, w, stride), geometry_ref.knn_bev(lat, K, h, w, stride, aff)), K
    both = np.concatenate([R.radius_cloud(), lat])
    for name, xyz in (("sparse", R.sparse_cloud()), ("border", R.border_cloud()), ("radius", both)):
        for rmax in (None, 0.0, 0.5, 0.625):
            assert np.array_equal(R.knn_bev(xyz, 5, h, w, stride, rmax), geometry_ref.knn_bev(xyz, 5, h, w, stride, aff, rmax=rmax)), (name, rmax)
    for n in (0, 1, 4):
        assert np.array_equal(R.knn_bev(lat[:n], 5, h, w, stride), geometry_ref.knn_bev(lat[:n], 5, h, w, stride, aff)), n

"""GPU: the geometry kernels (csrc/geometry.hip, through the C ABI) at their edges against the integer / Fraction statements of
tests/_geometry_ref.py, bit for bit -- no tolerance anywhere.  Every output (grids, owner workspaces, uv / xyz / src, counts, index
maps) lives in a _conv_ref.guarded buffer: NaN-filled, with 64 KiB sentinel margins that are checked after each call.

A  predicates: rows on every range limit and image bound and on their fp32 neighbours, a2 == 0, a2 < 0, -0.0, +inf, NaN
B  compaction: sizes around one 1024-row tile and around the 256-tile carry of the single-block scan, prescribed keep patterns
C  voxeliser: a dyadic grid (weights are multiples of 1/512), collisions by construction, the end of the grid, the host-side refusal
D  BEV KNN: a dyadic site whose distances are integers / 64, ties between different points in different cells, blocks, rings and
   waves, d2 == rmax^2, points on and outside the border, sites that are no multiple of a tile and one smaller than a tile

The conditions under which these inputs test anything are asserted on the CPU in tests/test_geometry_ref_host.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _conv_ref as C
import _geometry_ref as R
from _util import golden_cfg, load_golden, pkg
from oracle import geometry_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN_BITS = 0x7fc00000                   # what guarded() leaves in an fp32 / int32 element nobody wrote


# ---------------------------------------------------------------------------------------------------------------- buffers
def _gf(shape, tdt=torch.float32):
    return C.guarded(tuple(shape), tdt)


def _gi(shape):
    view, chk = C.guarded(tuple(shape), torch.float32)
    return view.view(torch.int32), chk


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def _u32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _rows_equal(got, want, m, what, untouched=True):
    """The first m rows bit for bit; the rows behind them still hold the buffer's NaN fill."""
    g = _u32(got).reshape(got.shape[0], -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(m, g.shape[1])
    bad = np.flatnonzero((g[:m] != w).any(1))
    assert bad.size == 0, "%s: %d of %d rows differ, first row %d: got %s want %s" % (what, bad.size, m, bad[0], g[bad[0]], w[bad[0]])
    if untouched:
        assert (g[m:] == NAN_BITS).all(), "%s: rows past the count were written" % what


# ---------------------------------------------------------------------------------------------------------------- A / B entries
def _range_filter(pts, lim):
    H = pkg("_hip")
    n = pts.shape[0]
    out, c1 = _gf((max(n, 1), 3)); src, c2 = _gi((max(n, 1),)); cnt, c3 = _gi((1,))
    ws = torch.empty((H.lib().dcf_compact_workspace_bytes(n),), dtype=torch.uint8, device="cuda")
    H.call("dcf_range_filter", _dev(pts), n, H.host_f32(lim), out, src, cnt, ws, H.stream_ptr())
    torch.cuda.synchronize()
    for c in (c1, c2, c3):
        c("dcf_range_filter")
    return out, src, int(cnt.item())


def _project_filter(pts, lim, crt, mode):
    H = pkg("_hip")
    n = pts.shape[0]
    uv, c0 = _gf((max(n, 1), 2)); xyz, c1 = _gf((max(n, 1), 3)); src, c2 = _gi((max(n, 1),)); cnt, c3 = _gi((1,))
    ws = torch.empty((H.lib().dcf_compact_workspace_bytes(n),), dtype=torch.uint8, device="cuda")
    H.call("dcf_project_filter", _dev(pts), n, H.host_f32(lim), H.host_f32(crt).reshape(-1), float(R.PRED_ULIM), float(R.PRED_VLIM), mode,
           uv, xyz, src, cnt, ws, H.stream_ptr())
    torch.cuda.synchronize()
    for c in (c0, c1, c2, c3):
        c("dcf_project_filter")
    return uv, xyz, src, int(cnt.item())


def _project_filter_batch(frames, lim, crts, mode, rows=None):
    """-> (uv [B,rows,2], xyz [B,rows,3], counts list) in guarded buffers; raises what the entry raises (sentinels checked first)."""
    H = pkg("_hip")
    B = len(frames)
    ns = [int(p.shape[0]) for p in frames]
    rows = max(max(ns), 1) if rows is None else rows
    dev = [_dev(p) if p.shape[0] else None for p in frames]
    uv, c0 = _gf((B, rows, 2)); xyz, c1 = _gf((B, rows, 3)); cnt, c2 = _gi((B,))
    ptrs = (ctypes.c_void_p * B)(*[d.data_ptr() if d is not None else None for d in dev])
    cnts = (ctypes.c_int32 * B)(*ns)
    crt = np.ascontiguousarray(np.asarray(crts, dtype=F32).reshape(B, 12))
    ws = torch.empty((B * H.lib().dcf_compact_workspace_bytes(max(max(ns), 1)),), dtype=torch.uint8, device="cuda")
    err = None
    try:
        H.call("dcf_project_filter_batch", ctypes.addressof(ptrs), ctypes.addressof(cnts), B, H.host_f32(lim), crt, float(R.PRED_ULIM),
               float(R.PRED_VLIM), int(mode), uv, xyz, rows, cnt, ws, H.stream_ptr())
    except H.DcfError as e:
        err = e
    torch.cuda.synchronize()
    for c in (c0, c1, c2):
        c("dcf_project_filter_batch")
    if err is not None:
        assert (_u32(uv) == NAN_BITS).all() and (_u32(xyz) == NAN_BITS).all() and (_u32(cnt) == NAN_BITS).all(), "a refused call wrote its outputs"
        raise err
    return uv, xyz, [int(v) for v in cnt.cpu().tolist()]


def _check_range(pts, lim, what):
    want_pts, want_src, m = R.range_filter(pts, lim)
    out, src, cnt = _range_filter(pts, lim)
    assert cnt == m, "%s: count %d, statement %d" % (what, cnt, m)
    _rows_equal(out, want_pts, m, what + " points", untouched=False)
    assert np.array_equal(src.cpu().numpy()[:m], want_src), what + " src"


def _check_project(pts, lim, crt, mode, what):
    w_uv, w_xyz, w_src, m = R.project_filter(pts, lim, crt, R.PRED_ULIM, R.PRED_VLIM, mode)
    uv, xyz, src, cnt = _project_filter(pts, lim, crt, mode)
    assert cnt == m, "%s: count %d, statement %d" % (what, cnt, m)
    _rows_equal(uv, w_uv, m, what + " uv")
    _rows_equal(xyz, w_xyz, m, what + " xyz")
    _rows_equal(src.view(torch.float32), w_src, m, what + " src")


def _check_batch(frames, lim, crts, mode, what, rows=None):
    uv, xyz, cnt = _project_filter_batch(frames, lim, crts, mode, rows)
    for b, p in enumerate(frames):
        w_uv, w_xyz, _, m = R.project_filter(p, lim, crts[b], R.PRED_ULIM, R.PRED_VLIM, mode)
        assert cnt[b] == m, "%s frame %d: count %d, statement %d" % (what, b, cnt[b], m)
        _rows_equal(uv[b], w_uv, m, "%s frame %d uv" % (what, b))
        _rows_equal(xyz[b], w_xyz, m, "%s frame %d xyz" % (what, b))


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("group", ["limits", "depth"])
def test_predicates_on_their_boundaries(group):
    lim, rows, tags = R.predicate_cases()[group]
    _check_range(rows, lim, group)
    for mode in (0, 1):
        _check_project(rows, lim, R.CRT_DYADIC, mode, "%s mode %d" % (group, mode))
        # batch form: the rows as frame 1 of three, the other frames under their own matrices
        frames = [rows[::-1].copy(), rows, rows[:7]]
        _check_batch(frames, lim, [R.frame_crt(2), R.CRT_DYADIC, R.frame_crt(5)], mode, "%s batch mode %d" % (group, mode))
    if group == "depth":            # compat keeps a2 < 0 with (u, v) inside the image, correct drops it
        m0 = R.project_filter(rows, lim, R.CRT_DYADIC, R.PRED_ULIM, R.PRED_VLIM, 0)[3]
        m1 = R.project_filter(rows, lim, R.CRT_DYADIC, R.PRED_ULIM, R.PRED_VLIM, 1)[3]
        assert m0 == m1 + 4


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("n", R.COMPACT_SIZES)
def test_compaction_tile_edges(n):
    for k, pattern in enumerate(R.PATTERNS):
        rows = R.pattern_rows(R.keep_pattern(pattern, n))
        what = "n %d %s" % (n, pattern)
        _check_range(rows, R.PRED_LIM, what)
        for mode in ((0, 1) if n <= 2048 else (k & 1,)):
            _check_project(rows, R.PRED_LIM, R.frame_crt(1), mode, "%s mode %d" % (what, mode))
            other = R.pattern_rows(R.keep_pattern("hash_half", 1025))
            _check_batch([rows, other], R.PRED_LIM, [R.frame_crt(1), R.frame_crt(6)], mode, "%s batch mode %d" % (what, mode))


@pytest.mark.parametrize("mode", [0, 1])
def test_compaction_batch_of_eight_frames(mode):
    frames = [R.pattern_rows(R.keep_pattern(p, n)) for n, p in R.BATCH_FRAMES]
    crts = [R.frame_crt(b) for b in range(8)]
    assert len(frames) == 8 and any(f.shape[0] == 0 for f in frames)
    _check_batch(frames, R.PRED_LIM, crts, mode, "eight frames", rows=3000 + 37)
    H = pkg("_hip")
    with pytest.raises(H.DcfError):                                     # nine frames: refused, nothing written
        _project_filter_batch(frames + [frames[0]], R.PRED_LIM, crts + [crts[0]], mode)
    uv, xyz, cnt = _project_filter_batch([frames[1]], R.PRED_LIM, crts[:1], mode)      # only empty frames: counts zeroed, nothing else
    assert cnt == [0] and (_u32(uv) == NAN_BITS).all() and (_u32(xyz) == NAN_BITS).all()


def test_empty_inputs_write_a_zero_count_only():
    empty = np.zeros((0, 3), dtype=F32)
    out, src, cnt = _range_filter(empty, R.PRED_LIM)
    assert cnt == 0 and (_u32(out) == NAN_BITS).all()
    uv, xyz, src, cnt = _project_filter(empty, R.PRED_LIM, R.CRT_DYADIC, 1)
    assert cnt == 0 and (_u32(uv) == NAN_BITS).all() and (_u32(xyz) == NAN_BITS).all()


# ---------------------------------------------------------------------------------------------------------------- C
def _tiny():
    g = geometry_ref.grid_constants(golden_cfg(load_golden("model_tiny.npz")))
    return g["lim"], g["aff"], g["dims"]


@functools.lru_cache(maxsize=None)
def _vox_case(name):
    """-> (pts, lim, aff, dims, {mode: fp32 grid of the statement})."""
    if name == "tiny":
        lim, aff, dims = _tiny()
        pts = R.tiny_grid_cloud(lim)
    else:
        pts, lim = R.voxel_clouds()[name]
        aff, dims = R.VOX_AFF, R.VOX_DIMS
    want = {m: R.dense_grid(R.voxelize(pts, lim, aff, dims, m), dims) for m in (R.COMPAT, R.ACCUM, R.OCCUPANCY)}
    return pts, lim, aff, dims, want


def _owner(B, nvox):
    ow, chk = _gi((B, 2, nvox))
    ow.zero_()
    return ow, chk


def _voxelize(pts, lim, aff, dims, mode):
    H = pkg("_hip")
    Cz, L, W = dims
    grid, c0 = _gf(dims)
    ow, c1 = _owner(1, Cz * L * W)
    H.call("dcf_voxelize", _dev(pts), pts.shape[0], H.host_f32(lim), H.host_f32(aff), Cz, L, W, mode, grid,
           ow if mode in (R.COMPAT, R.COMPAT_ROUNDS) else None, H.stream_ptr())
    torch.cuda.synchronize()
    c0("dcf_voxelize grid, mode %d" % mode); c1("dcf_voxelize owner workspace, mode %d" % mode)
    assert int(ow.abs().max()) == 0, "the owner workspace did not come back zero (mode %d)" % mode
    return grid


def _voxelize_batch(frames, lim, aff, dims, dtype=None):
    """dcf_voxelize_batch (dtype None: fp32 [B,Cz,L,W]) or dcf_voxelize_batch_nhwc ([B,L,W,Cz] of the dtype code)."""
    H = pkg("_hip")
    Cz, L, W = dims
    B = len(frames)
    dev = [_dev(p) for p in frames]
    ptrs = (ctypes.c_void_p * B)(*[d.data_ptr() if d.shape[0] else None for d in dev])
    ns = (ctypes.c_int * B)(*[p.shape[0] for p in frames])
    ow, c1 = _owner(B, Cz * L * W)
    if dtype is None:
        out, c0 = _gf((B, Cz, L, W))
        H.call("dcf_voxelize_batch", ctypes.addressof(ptrs), ctypes.addressof(ns), B, H.host_f32(lim), H.host_f32(aff), Cz, L, W, out, ow, H.stream_ptr())
    else:
        out, c0 = _gf((B, L, W, Cz), {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}[dtype])
        H.call("dcf_voxelize_batch_nhwc", dtype, ctypes.addressof(ptrs), ctypes.addressof(ns), B, H.host_f32(lim), H.host_f32(aff), Cz, L, W, out, ow,
               H.stream_ptr())
    torch.cuda.synchronize()
    c0("voxelize batch output"); c1("voxelize batch owner workspace")
    assert int(ow.abs().max()) == 0, "the owner workspace did not come back zero"
    return out


def _grid_equal(got, want, what):
    g, w = _u32(got).reshape(-1), np.ascontiguousarray(want, dtype=F32).view(np.uint32).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d voxels differ, first flat index %d: got %#x want %#x" % (what, bad.size, bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("name", ["integer", "half", "one_cell", "neighbours", "last_cells", "tiny"])
def test_voxeliser_modes_bit_for_bit(name):
    pts, lim, aff, dims, want = _vox_case(name)
    _grid_equal(_voxelize(pts, lim, aff, dims, R.COMPAT), want[R.COMPAT], name + " compat")
    _grid_equal(_voxelize(pts, lim, aff, dims, R.COMPAT_ROUNDS), want[R.COMPAT], name + " compat, nine rounds")
    _grid_equal(_voxelize(pts, lim, aff, dims, R.ACCUM), want[R.ACCUM], name + " accum")
    _grid_equal(_voxelize(pts, lim, aff, dims, R.ACCUM), want[R.ACCUM], name + " accum, second run")
    _grid_equal(_voxelize(pts, lim, aff, dims, R.OCCUPANCY), want[R.OCCUPANCY], name + " occupancy")
    if name == "integer":           # one corner holds exactly 1, the seven others were written with +0.0
        assert sorted(want[R.ACCUM][want[R.ACCUM] != 0].tolist()) == [1.0] * pts.shape[0]


@pytest.mark.parametrize("name", ["neighbours", "last_cells", "tiny"])
def test_voxeliser_batch_forms_bit_for_bit(name):
    pts, lim, aff, dims, want = _vox_case(name)
    other = "one_cell" if name != "tiny" else "tiny"
    opts, _, _, _, owant = _vox_case(other)
    frames = [pts, np.zeros((0, 3), dtype=F32), opts[::-1].copy() if other == "tiny" else opts]
    wants = [want[R.COMPAT], np.zeros(dims, dtype=F32),
             R.dense_grid(R.voxelize(frames[2], lim, aff, dims, R.COMPAT), dims) if other == "tiny" else owant[R.COMPAT]]
    out = _voxelize_batch(frames, lim, aff, dims)
    for b in range(3):
        _grid_equal(out[b], wants[b], "%s batch frame %d" % (name, b))
    for code, tdt in ((0, torch.float32), (1, torch.bfloat16), (2, torch.float16)):
        out = _voxelize_batch(frames, lim, aff, dims, code)
        for b in range(3):
            w = R.grid_nhwc(wants[b], tdt)
            got = out[b].cpu()
            assert torch.equal(C.bits_of(got), C.bits_of(w)), "%s NHWC %s frame %d: %d elements differ" % (
                name, tdt, b, int((C.bits_of(got) != C.bits_of(w)).sum()))


def test_voxeliser_refuses_a_cell_outside_the_grid():
    """Limits under which the point's own cell can leave the grid, and non-finite lim / aff: DCF_EINVAL from every entry, nothing
    launched -- grid and owner workspace keep their NaN fill -- and the sentinels are intact."""
    H = pkg("_hip")
    pts = R.voxel_clouds()["integer"][0]
    Cz, L, W = R.VOX_DIMS
    cases = [(lim, aff) for lim, aff, _ in R.REFUSED_GRIDS.values()]
    bad = R.VOX_LIM.copy(); bad[1] = np.inf
    cases.append((bad, R.VOX_AFF))
    bad = R.VOX_AFF.copy(); bad[5] = np.nan
    cases.append((R.VOX_LIM, bad))
    d = _dev(pts)
    ptrs = (ctypes.c_void_p * 1)(d.data_ptr())
    ns = (ctypes.c_int * 1)(pts.shape[0])
    for lim, aff in cases:
        assert not R.voxel_cell_range(lim, aff, R.VOX_DIMS)[2]
        for entry in ("single0", "single1", "single2", "single3", "batch", "nhwc"):
            grid, c0 = _gf(R.VOX_DIMS)
            ow, c1 = _gi((1, 2, Cz * L * W))
            with pytest.raises(H.DcfError):
                if entry.startswith("single"):
                    H.call("dcf_voxelize", d, pts.shape[0], H.host_f32(lim), H.host_f32(aff), Cz, L, W, int(entry[-1]), grid, ow, H.stream_ptr())
                elif entry == "batch":
                    H.call("dcf_voxelize_batch", ctypes.addressof(ptrs), ctypes.addressof(ns), 1, H.host_f32(lim), H.host_f32(aff), Cz, L, W, grid, ow,
                           H.stream_ptr())
                else:
                    H.call("dcf_voxelize_batch_nhwc", 0, ctypes.addressof(ptrs), ctypes.addressof(ns), 1, H.host_f32(lim), H.host_f32(aff), Cz, L, W, grid, ow,
                           H.stream_ptr())
            torch.cuda.synchronize()
            c0("refused " + entry); c1("refused " + entry)
            assert (_u32(grid) == NAN_BITS).all() and (_u32(ow) == NAN_BITS).all(), "a refused call (%s) wrote something" % entry
    for lim, aff, dims in ((R.VOX_LIM, R.VOX_AFF, R.VOX_DIMS), (R.VOX_LIM_TIGHT, R.VOX_AFF, R.VOX_DIMS), _tiny()):      # accepted
        assert R.voxel_cell_range(lim, aff, dims)[2]
        _voxelize(pts, lim, aff, dims, R.COMPAT)


# ---------------------------------------------------------------------------------------------------------------- D
@functools.lru_cache(maxsize=None)
def _knn_cloud(name):
    if name == "lattice":
        return R.lattice_cloud()
    if name == "sparse":
        return R.sparse_cloud()
    if name == "border":
        return R.border_cloud()
    if name == "radius":
        return R.radius_cloud()
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _knn_want(name, count, stride, rmax):
    """The statement's K = 8 map of the first `count` rows (None: all); the map for a smaller K is its first K planes."""
    xyz = _knn_cloud(name)
    h, w = R.knn_site(stride)
    return R.knn_bev(xyz if count is None else xyz[:count], 8, h, w, stride, rmax)


def _pad(xyz, n_max):
    out = np.full((n_max, 3), np.nan, dtype=F32)
    out[:xyz.shape[0]] = xyz
    return out


def _knn(xyz, count, K, stride, rmax):
    H = pkg("_hip")
    h, w = R.knn_site(stride)
    n_max = xyz.shape[0]
    out, chk = _gi((K, h, w))
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    ws = torch.empty((H.lib().dcf_knn_workspace_bytes(n_max, h, w),), dtype=torch.uint8, device="cuda")
    r2 = -1.0 if rmax is None else float(F32(rmax) * F32(rmax))
    a = R.KNN_AFF
    H.call("dcf_knn_bev", _dev(xyz), cnt, n_max, K, h, w, stride, float(a[0]), float(a[1]), float(a[2]), float(a[3]), r2, out, ws, H.stream_ptr())
    torch.cuda.synchronize()
    chk("dcf_knn_bev")
    return out.cpu().numpy()


def _map_equal(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, "%s: %d entries differ, first (k, i, j) %s: got %s want %s" % (
        what, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


KERNELS = {"wave": ("wave", None), "tile1": ("tile", "1"), "tile2": ("tile", "2"), "tile4": ("tile", "4")}
RMAX = {"lattice": (None, 0.5), "sparse": (None, 0.625), "border": (None, 0.5), "radius": (None, 0.0, 0.5, 0.625)}


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("cloud", ["lattice", "sparse", "border", "radius"])
def test_knn_whole_site_against_the_integer_statement(cloud, kernel):
    H = pkg("_hip")
    xyz = _knn_cloud(cloud)
    try:
        H.set_option("KNN_KERNEL", KERNELS[kernel][0])
        H.set_option("KNN_TILE_WAVES", KERNELS[kernel][1])
        for stride in R.KNN_STRIDES:
            for rmax in RMAX[cloud]:
                want = _knn_want(cloud, None, stride, rmax)
                for K in range(1, 9):
                    _map_equal(_knn(xyz, xyz.shape[0], K, stride, rmax), want[:K], "%s %s stride %d K %d rmax %s" % (cloud, kernel, stride, K, rmax))
    finally:
        H.set_option("KNN_TILE_WAVES", None)
        H.set_option("KNN_KERNEL", None)
    if cloud == "radius":           # d2 == rmax^2 is kept: six neighbours at the pixel the cloud surrounds, not three
        assert (_knn_want(cloud, None, 2, 0.625)[:, 12, 24] >= 0).sum() == 6


@pytest.mark.parametrize("kernel", ["wave", "tile1", "tile4"])
def test_knn_count_edges(kernel):
    """count 0, 1 and K - 1 of a buffer whose rows past the count are NaN: -1 padding, the rows past the count are never read as points."""
    H = pkg("_hip")
    lat = _knn_cloud("lattice")
    try:
        H.set_option("KNN_KERNEL", KERNELS[kernel][0])
        H.set_option("KNN_TILE_WAVES", KERNELS[kernel][1])
        for stride in R.KNN_STRIDES:
            for K in (1, 2, 5, 8):
                for count in sorted({0, 1, K - 1}):
                    want = _knn_want("lattice", count, stride, None)[:K]
                    got = _knn(_pad(lat[:count], 40), count, K, stride, None)
                    _map_equal(got, want, "%s stride %d K %d count %d" % (kernel, stride, K, count))
                    assert (got[count:] == -1).all() and (count == 0 or (got[:count] >= 0).all())
    finally:
        H.set_option("KNN_TILE_WAVES", None)
        H.set_option("KNN_KERNEL", None)


def _batch_frames():
    """Three frames, one of them empty, rows past each count NaN -> (xyz [3,n_max,3], counts, names)."""
    lat, bc = _knn_cloud("lattice"), _knn_cloud("border")
    n_max = lat.shape[0] + 3
    return np.stack([_pad(lat, n_max), _pad(lat[:0], n_max), _pad(bc, n_max)]), [lat.shape[0], 0, bc.shape[0]], ["lattice", "lattice", "border"]


def _batch_want(names, counts, stride, rmax, K):
    return np.stack([_knn_want(nm, None if c == _knn_cloud(nm).shape[0] else c, stride, rmax)[:K] for nm, c in zip(names, counts)])


@pytest.mark.parametrize("fine_min", [None, "0"])
def test_knn_batch_and_coarse_sites_on_the_fine_cells(fine_min):
    """dcf_knn_bev_batch on the stride-2 site, then dcf_knn_bev_batch_shared for strides 4 / 8 / 16 on its cells -- with
    KNN_FINE_MIN at its default and at 0, where every pixel's window is served from the fine cells even on this small cloud."""
    H, ops = pkg("_hip"), pkg("ops")
    xyz, counts, names = _batch_frames()
    B, n_max = xyz.shape[0], xyz.shape[1]
    d = _dev(xyz)
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    fh, fw = R.knn_site(2)
    try:
        H.set_option("KNN_FINE_MIN", fine_min)
        for rmax in (None, 0.625):
            for K in (1, 3, 5, 8):
                ws_f = torch.empty((B, ops.knn_ws_stride(n_max, fh, fw)), dtype=torch.uint8, device="cuda")
                out, chk = _gi((B, K, fh, fw))
                ops.knn_bev_batch(d, cnt, K, fh, fw, 2, R.KNN_AFF, rmax, ws=ws_f, out=out)
                torch.cuda.synchronize()
                chk("dcf_knn_bev_batch")
                _map_equal(out.cpu().numpy(), _batch_want(names, counts, 2, rmax, K), "batch stride 2 K %d rmax %s" % (K, rmax))
                for stride in (4, 8, 16):
                    h, w = R.knn_site(stride)
                    out, chk = _gi((B, K, h, w))
                    ops.knn_bev_batch_shared(d, cnt, K, h, w, stride, (fh, fw, 2), ws_f, R.KNN_AFF, rmax, out=out)
                    torch.cuda.synchronize()
                    chk("dcf_knn_bev_batch_shared")
                    _map_equal(out.cpu().numpy(), _batch_want(names, counts, stride, rmax, K), "shared stride %d K %d rmax %s fine_min %s" % (stride, K, rmax, fine_min))
    finally:
        H.set_option("KNN_FINE_MIN", None)


@pytest.mark.parametrize("merged", [None, "0"])
def test_knn_all_sites_in_one_call(merged):
    """dcf_knn_bev_sites: the four sites of the dyadic grid in one call (the coarse three on the stride-2 cells), the searches as one
    launch and, with KNN_MERGED_SEARCH=0, as one launch per site."""
    H, ops = pkg("_hip"), pkg("ops")
    xyz, counts, names = _batch_frames()
    B, n_max = xyz.shape[0], xyz.shape[1]
    d = _dev(xyz)
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    try:
        H.set_option("KNN_MERGED_SEARCH", merged)
        for rmax in (None, 0.5):
            for K in (1, 5, 8):
                sites, checks = [], []
                for i, s in enumerate(R.KNN_STRIDES):
                    h, w = R.knn_site(s)
                    out, chk = _gi((B, K, h, w))
                    checks.append(chk)
                    sites.append((h, w, s, -1 if i == 0 else 0, torch.empty((B, ops.knn_ws_stride(n_max, h, w)), dtype=torch.uint8, device="cuda"), out))
                ops.knn_bev_sites(d, cnt, K, sites, R.KNN_AFF, rmax)
                torch.cuda.synchronize()
                for i, s in enumerate(R.KNN_STRIDES):
                    checks[i]("dcf_knn_bev_sites site %d" % i)
                    _map_equal(sites[i][5].cpu().numpy(), _batch_want(names, counts, s, rmax, K), "sites stride %d K %d rmax %s merged %s" % (s, K, rmax, merged))
    finally:
        H.set_option("KNN_MERGED_SEARCH", None)

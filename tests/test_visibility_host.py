"""The camera visibility mask without a GPU (visibility.py, train.parse_camera_mask_config): the fp32 chain against
libm's fmaf, the field-of-view predicate against the C oracle, occluders and the hidden rule against a float64 restatement, the
candidates dropped over nearer labels, and the config block."""
import copy
import ctypes
import ctypes.util

import numpy as np
import pytest

from _paste_util import label_row, plan_of, tiny_crt
from _util import pkg
from _visibility_util import LIM_KITTI, LIM_TINY, bits as _bits, lim_of as _lim, pasted_world as _pasted_world


def _fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
    return m.fmaf


# ------------------------------------------------------------------------------------------------ 1. the chain
def test_fma32_is_libm_fmaf_on_random_triples_and_constructed_ties():
    V = pkg("visibility")
    fmaf = _fmaf()
    rng = np.random.RandomState(3)
    n = 60000
    # mantissas of every length and exponents that let the addend fall anywhere against the product, far below its last bit included
    a = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.randint(-60, 40, n)).astype(np.float32)
    # cancellations: c close to -a b
    c[:n // 4] = -(a[:n // 4].astype(np.float64) * b[:n // 4]).astype(np.float32)
    # ties: a b = 1 + 2^-11 + 2^-24 lies exactly between two fp32 numbers; an addend far below decides, which a float64 sum loses
    t = np.float32(1.0 + 2.0 ** -12)
    ties_a = np.full(8, t, dtype=np.float32)
    ties_c = np.array([2.0 ** -80, -2.0 ** -80, 2.0 ** -100, -2.0 ** -100, 0.0, 2.0 ** -126, -2.0 ** -126, 2.0 ** -40], dtype=np.float32)
    a, b, c = np.concatenate([a, ties_a]), np.concatenate([b, ties_a]), np.concatenate([c, ties_c])
    got = V._fma32(a, b, c)
    want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(_bits(plain[n:]), _bits(want[n:]))          # the ties are ties: the double rounding gets some wrong


@pytest.mark.parametrize("which", ["tiny", "kitti"])
def test_project_chain_is_the_fmaf_chain(which):
    V = pkg("visibility")
    fmaf = _fmaf()
    crt = np.asarray(tiny_crt() if which == "tiny" else pkg("calib").kitti_like_crt(), dtype=np.float32).reshape(4, 3)
    rng = np.random.RandomState(5)
    pts = (rng.rand(4000, 3) * np.array([80.0, 90.0, 5.0]) + np.array([-5.0, -45.0, -3.5])).astype(np.float32)
    pts[:4] = [[4.0, -1.0, 0.0], [0.0, 0.0, 0.0], [np.inf, 1.0, 1.0], [np.nan, 1.0, 1.0]]
    u, v, a2 = V.project_chain(pts, crt)
    want = np.empty((len(pts), 3), dtype=np.float32)
    for i, (x, y, z) in enumerate(pts.tolist()):
        for j in range(3):
            t = float(np.float32(np.float64(x) * np.float64(crt[0, j]))) if np.isfinite(x) else float(np.float32(x) * crt[0, j])
            t = fmaf(y, float(crt[1, j]), t)
            t = fmaf(z, float(crt[2, j]), t)
            want[i, j] = fmaf(1.0, float(crt[3, j]), t)
    with np.errstate(invalid="ignore", divide="ignore"):
        wu, wv = want[:, 0] / want[:, 2], want[:, 1] / want[:, 2]        # numpy's fp32 division is correctly rounded
    fin = np.isfinite(pts).all(1)
    assert np.array_equal(_bits(a2[fin]), _bits(want[fin, 2])) and np.array_equal(_bits(u[fin]), _bits(wu[fin])) and np.array_equal(_bits(v[fin]), _bits(wv[fin]))
    assert not np.isfinite(u[3]) and not np.isfinite(a2[3])
    if which == "tiny":
        assert u[0] == 79.0 and a2[0] == 4.0                              # the dyadic calibration of the edge tests


# ------------------------------------------------------------------------------------------------ 2. the field of view
@pytest.mark.parametrize("mode", ["compat", "correct"])
def test_fov_keep_is_the_oracles_projection_after_its_range_filter(mode):
    from oracle import geometry_ref
    V = pkg("visibility")
    crt = np.asarray(tiny_crt(), dtype=np.float32).reshape(4, 3)
    Hh, Ww = 96, 128
    ulim, vlim = (Hh, Ww) if mode == "compat" else (Ww, Hh)               # FrameGeometry.limits(): compat swaps them
    lim = _lim(LIM_KITTI)
    rng = np.random.RandomState(11)
    pts = (rng.rand(30000, 3) * np.array([90.0, 100.0, 6.0]) + np.array([-10.0, -50.0, -4.0])).astype(np.float32)
    # u = 64 - 60 y / x, v = 48 - 60 z / x: points exactly on u = 0, u = ulim (both modes' bounds), v = 0, v = vlim, and the range faces
    edge = [[15.0, 16.0, -1.0], [15.0, -16.0, -1.0], [15.0, -8.0, -1.0], [0.625, 0.0, 0.5], [0.625, 0.0, -0.5], [60.0, 0.0, -2.0],
            [20.0, 1.0, 0.5], [4.0, -1.0, 0.0],
            [lim[0], 0.0, -1.0], [lim[1], 0.0, -1.0], [20.0, lim[2], -1.0], [20.0, lim[3], -1.0], [20.0, 0.0, lim[4]], [20.0, 0.0, lim[5]],
            [np.nextafter(lim[0], np.float32(1)), 0.0, -1.0], [np.nextafter(lim[1], np.float32(0)), 0.0, -1.0],
            [np.inf, np.inf, np.inf], [np.nan, 0.0, 0.0], [-np.inf, 0.0, 0.0], [-5.0, 0.5, 0.2]]
    pts[:len(edge)] = np.array(edge, dtype=np.float32)
    u, v, _ = V.project_chain(pts, crt)
    assert u[0] == 0.0 and u[1] == 128.0 and u[2] == 96.0 and v[3] == 0.0 and v[4] == 96.0      # the constructed points sit ON the bounds
    keep = V.fov_keep(pts, crt, lim, ulim, vlim, 0 if mode == "compat" else 1)
    pin, src1 = geometry_ref.range_filter(pts, lim)
    _, _, src2 = geometry_ref.project(pin, crt, ulim, vlim, mode)
    assert np.array_equal(np.nonzero(keep)[0], src1[src2])
    # a row ON a bound fails the strict compare; the bound of the OTHER mode lies inside this one's image
    assert keep[:6].tolist() == ([False, False, False, False, True, True] if mode == "compat" else [False, False, True, False, False, True])
    assert 1000 < keep.sum() < len(pts)
    masked = V.mask_points(pts, crt, lim, ulim, vlim, 0 if mode == "compat" else 1, True, None)
    assert np.array_equal(_bits(masked[keep]), _bits(pts[keep])) and np.isposinf(masked[~keep]).all()


def test_mask_points_off_is_a_copy_and_keeps_nan_payloads():
    V = pkg("visibility")
    pts = np.random.RandomState(2).rand(50, 3).astype(np.float32) * 10
    pts.view(np.uint32)[3] = [0x7FC12345, 0x3F800000, 0xFFC00001]
    pts[4] = [-np.inf, np.inf, 0.0]
    out = V.mask_points(pts, tiny_crt(), _lim(LIM_TINY), 128, 96, 1, False, None)
    assert out is not pts and np.array_equal(_bits(out), _bits(pts))
    # an occluder that hides nothing the NaN row compares with: the payload survives, a row behind it goes
    occ = np.array([[0.0, 0.0, 128.0, 96.0, 5.0]], dtype=np.float32)
    pts[5], pts[6] = [6.0, 0.0, 0.0], [5.0, 0.0, 0.0]
    out = V.mask_points(pts, tiny_crt(), _lim(LIM_TINY), 128, 96, 1, False, occ)
    assert np.array_equal(_bits(out[3]), _bits(pts[3])) and np.isposinf(out[5]).all() and np.array_equal(out[6], pts[6])


# ------------------------------------------------------------------------------------------------ 3. occluders and the hidden rule
@pytest.mark.parametrize("which", ["tiny", "kitti"])
def test_occluders_and_hidden_against_a_float64_restatement(which):
    V, P = pkg("visibility"), pkg("paste")
    bank, plan, pasted, n, crt, lim6, hw = _pasted_world(which)
    occ = V.occluders(plan, bank, crt)
    assert occ.dtype == np.float32 and occ.shape == (len(plan["patches"]), 5)
    u, v, a2 = V.project_chain(pasted, np.asarray(crt, dtype=np.float32))
    got = V.hidden(u, v, a2, occ)
    # the restatement: float64 projection, the far corner of the box by a search over its corners written out here
    with np.errstate(invalid="ignore"):                                   # (the rows pasting removed are +inf rows)
        u64, v64, d64 = P.project_px(pasted, np.asarray(crt, dtype=np.float32))
    want, near_edge = np.zeros(len(pasted), dtype=bool), np.zeros(len(pasted), dtype=bool)
    c64 = np.asarray(crt, dtype=np.float64).reshape(4, 3)
    for j, (q, r) in enumerate(zip(plan["patches"], plan["patch_rows"])):
        x, y, z, l, w, h, yaw = (float(t) for t in bank["boxes"][r][:7])
        far = -np.inf
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    px = x + sx * l / 2 * np.cos(yaw) - sy * w / 2 * np.sin(yaw)
                    py = y + sx * l / 2 * np.sin(yaw) + sy * w / 2 * np.cos(yaw)
                    far = max(far, px * c64[0, 2] + py * c64[1, 2] + (z + sz * h / 2) * c64[2, 2] + c64[3, 2])
        D = far + 1.0 / 64
        assert abs(float(occ[j, 4]) - D) <= 1e-5 * D and tuple(occ[j, :4]) == (q[0], q[1], q[0] + q[2], q[1] + q[3])
        with np.errstate(invalid="ignore"):
            want |= (u64 >= q[0]) & (u64 < q[0] + q[2]) & (v64 >= q[1]) & (v64 < q[1] + q[3]) & (d64 > D)
            for t, e in ((u64, q[0]), (u64, q[0] + q[2]), (v64, q[1]), (v64, q[1] + q[3]), (d64, D)):
                near_edge |= np.abs(t - e) < 1e-3                        # fp32 against float64 may decide either way within this of an edge
    sure = ~near_edge & np.isfinite(pasted).all(1)
    assert np.array_equal(got[sure], want[sure]) and near_edge.sum() < 0.05 * len(pasted)
    # no appended point is hidden by its own record; some scene rows are hidden
    first, own_hidden, own_rows = n, 0, 0
    for k, r in enumerate(plan["rows"]):
        a = int(plan["append"][k, 1])
        j = plan["patch_rows"].index(r)
        own_hidden += int(V.hidden(u[first:first + a], v[first:first + a], a2[first:first + a], occ[j:j + 1]).sum())
        own_rows, first = own_rows + a, first + a
    scene = int(got[:n].sum())
    print("%s: %d of %d own points hidden, %d of %d scene rows hidden" % (which, own_hidden, own_rows, scene, n))
    assert own_hidden == 0 and own_rows >= 80 and scene >= 100
    # every row mask_points leaves and every record whose rectangle holds its pixel: not deeper than D
    left = V.mask_points(pasted, crt, _lim(lim6), hw[1], hw[0], 1, False, occ)
    lu, lv, la = V.project_chain(left, np.asarray(crt, dtype=np.float32))
    with np.errstate(invalid="ignore"):
        for q in occ:
            inside = (lu >= q[0]) & (lu < q[2]) & (lv >= q[1]) & (lv < q[3])
            assert (la[inside] <= q[4]).all()


def test_occluders_skip_a_record_behind_the_camera():
    V = pkg("visibility")
    bank = {"boxes": np.stack([label_row(8.0, 0.0, -1.0, 0.0), label_row(1.0, 0.0, -1.0, 0.0)], 0)}      # the second box straddles x = 0
    plan = plan_of(hw=(96, 128))
    plan["patches"] = np.array([[10, 10, 20, 10, 0, 0, 20, 10, 0], [30, 10, 20, 10, 0, 0, 20, 10, 600]], dtype=np.int64)
    plan["patch_rows"] = [0, 1]
    occ = V.occluders(plan, bank, tiny_crt())
    assert occ.shape == (1, 5) and tuple(occ[0, :4]) == (10.0, 10.0, 30.0, 20.0) and occ[0, 4] == np.float32(10.0 + 2.0 ** -6)
    assert V.occluders(plan_of(hw=(96, 128)), bank, tiny_crt()).shape == (0, 5)


# ------------------------------------------------------------------------------------------------ 4. candidates over nearer labels
def _plan_with(bank, rows, dests, hw=(96, 128)):
    """A plan of the bank's `rows` with the destination rectangles `dests` (x0, y0, w, h), patch records in the given order."""
    P = pkg("paste")
    plan = P.empty_plan(100, hw)
    plan["rows"] = list(rows)
    plan["labels"] = np.asarray(bank["boxes"], dtype=np.float32)[list(rows)]
    plan["records"] = np.stack([P.record(bank["boxes"][r], 0.1) for r in rows], 0)
    plan["append"] = np.array([[10 * r, 10] for r in rows], dtype=np.int64)
    plan["patches"] = np.array([[d[0], d[1], d[2], d[3], 0, 0, d[2], d[3], 100 * k] for k, d in enumerate(dests)], dtype=np.int64)
    plan["patch_rows"] = list(rows)
    return plan


def _same_plan(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_drop_covering():
    V, B = pkg("visibility"), pkg("objbank")
    crt, hw = tiny_crt(), (96, 128)
    bank = {"boxes": np.stack([label_row(12.0, 0.0, -1.0, 0.0), label_row(9.0, 3.5, -1.0, 0.0)], 0)}
    boxes = np.zeros((20, 9), dtype=np.float32)
    boxes[0] = label_row(6.0, 0.0, -1.0, 0.0)                             # nearer than bank row 0, on the same pixels
    boxes[1] = label_row(14.0, -3.0, -1.0, 0.0)                           # farther than both
    boxes[2] = label_row(-6.0, 0.0, -1.0, 0.0)                            # behind the camera: no rectangle
    R0, R1, R2 = (B.patch_rect(boxes[i], crt, hw) for i in range(3))
    assert R0[2] > 0 and R1[2] > 0 and R2 == (0, 0, 0, 0)
    far, side = B.patch_rect(bank["boxes"][0], crt, hw), B.patch_rect(bank["boxes"][1], crt, hw)
    # a nearer label under a far candidate: dropped; the candidate beside it stays, orders kept
    plan = _plan_with(bank, [1, 0], [side, far])
    before = copy.deepcopy(plan)
    out = V.drop_covering(plan, boxes, 3, crt, bank)
    _same_plan(plan, before)                                              # pure
    assert out["rows"] == [1] and out["patch_rows"] == [1] and np.array_equal(out["patches"], plan["patches"][:1])
    assert np.array_equal(out["labels"], plan["labels"][:1]) and np.array_equal(out["records"], plan["records"][:1]) and np.array_equal(out["append"], plan["append"][:1])
    assert out["n_points"] == plan["n_points"] and out["image_hw"] == plan["image_hw"] and V.covering(plan, boxes, 3, crt, bank) == [0]
    # only the first `num` rows are labels
    _same_plan(V.drop_covering(plan, boxes[1:], 2, crt, bank), plan)
    # the reverse: a candidate NEARER than the label whose rectangle it meets stays (the label is the one hidden, as a real object would be)
    boxes2 = np.zeros((20, 9), dtype=np.float32)
    boxes2[0] = label_row(14.0, 0.0, -1.0, 0.0)
    assert B.patch_rect(boxes2[0], crt, hw)[2] > 0
    _same_plan(V.drop_covering(plan, boxes2, 1, crt, bank), plan)
    # equal depths do not drop (d_i < e_k is strict)
    boxes2[0] = label_row(12.0, 0.0, -1.0, 0.0)
    _same_plan(V.drop_covering(plan, boxes2, 1, crt, bank), plan)
    # touching rectangles do not meet (half-open); one pixel of overlap does -- on either axis
    x0, y0, w, h = R0
    for dest, dropped in (((x0 + w, y0, 5, h), False), ((x0 + w - 1, y0, 5, h), True), ((x0 - 5, y0, 5, h), False), ((x0 - 5, y0, 6, h), True),
                          ((x0, y0 + h, w, 4), False), ((x0, y0 + h - 1, w, 4), True), ((x0, y0 - 4, w, 4), False), ((x0, y0 - 4, w, 5), True)):
        p = _plan_with(bank, [0], [dest])
        assert (V.drop_covering(p, boxes, 1, crt, bank)["rows"] == []) == dropped, dest
    # a label without a rectangle drops nothing; no labels, no patches: equal plans
    _same_plan(V.drop_covering(plan, boxes[2:], 1, crt, bank), plan)
    _same_plan(V.drop_covering(plan, boxes, 0, crt, bank), plan)
    empty = pkg("paste").empty_plan(7, hw)
    _same_plan(V.drop_covering(empty, boxes, 3, crt, bank), empty)
    nopatch = dict(plan, patches=np.zeros((0, 9), dtype=np.int64), patch_rows=[])
    _same_plan(V.drop_covering(nopatch, boxes, 3, crt, bank), nopatch)


# ------------------------------------------------------------------------------------------------ 5. the config block
def test_config_block():
    T, V = pkg("train"), pkg("visibility")
    paste_on = dict(enabled=True, bank="bank.npz", paste_image=True)
    assert T.parse_camera_mask_config({}) is None
    assert T.parse_camera_mask_config({"camera_mask": None}) is None
    assert T.parse_camera_mask_config({"camera_mask": {}}) is None
    assert T.parse_camera_mask_config({"camera_mask": {"fov_crop": False, "paste_occlusion": False}}) is None
    assert T.parse_camera_mask_config({"camera_mask": {"fov_crop": True}}) == {"fov_crop": True, "paste_occlusion": False}
    assert T.parse_camera_mask_config({"camera_mask": {"paste_occlusion": True}, "augment_paste": paste_on}) == {"fov_crop": False, "paste_occlusion": True}
    assert T.parse_camera_mask_config({"camera_mask": {"fov_crop": True, "paste_occlusion": True}, "augment_paste": paste_on}) == {"fov_crop": True, "paste_occlusion": True}
    assert V.KEYS == ("fov_crop", "paste_occlusion")
    bad = [{"camera_mask": 1}, {"camera_mask": [True]}, {"camera_mask": {"fov": True}}, {"camera_mask": {"fov_crop": 1}},
           {"camera_mask": {"fov_crop": "true"}}, {"camera_mask": {"paste_occlusion": 0}}, {"camera_mask": {"fov_crop": None}},
           {"camera_mask": {"fov_crop": True, "enabled": True}},
           # paste_occlusion needs an ENABLED augment_paste block with paste_image: true
           {"camera_mask": {"paste_occlusion": True}},
           {"camera_mask": {"paste_occlusion": True}, "augment_paste": dict(paste_on, enabled=False)},
           {"camera_mask": {"paste_occlusion": True}, "augment_paste": dict(paste_on, paste_image=False)},
           {"camera_mask": {"fov_crop": True, "paste_occlusion": True}, "augment_paste": dict(paste_on, paste_image=False)}]
    for cfg in bad:
        with pytest.raises(ValueError):
            T.parse_camera_mask_config(cfg)
    # the paste block's parser returns what it returned: its key set is pinned, the switch is no key of it
    cfg = {"augment_paste": dict(paste_on, seed=4, margin=0.25)}
    want = T.parse_paste_config(cfg)
    assert T.parse_paste_config(dict(cfg, camera_mask={"fov_crop": True, "paste_occlusion": True})) == want
    assert sorted(want) == ["bank", "margin", "max_candidates", "paste_image", "seed", "target_objects"]
    with pytest.raises(ValueError):
        T.parse_paste_config({"augment_paste": dict(paste_on, paste_occlusion=True)})


def test_yaml_documents_the_block_as_comments_only():
    import os
    import yaml
    from _util import PKG, ROOT
    path = os.path.join(ROOT, PKG, "config", "config_carla.yaml")
    text = open(path).read()
    assert "# camera_mask:" in text and "#   fov_crop: false" in text and "#   paste_occlusion: false" in text
    assert "camera_mask" not in yaml.safe_load(text)

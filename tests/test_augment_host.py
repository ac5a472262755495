"""Train-time BEV augmentation without a GPU (augment.py, train.parse_augment_config): the stateless draw,
the fp32 point statement, the projection matrix that keeps a point on its pixel, the labels, the config block."""
import copy
import math
import os
import re

import numpy as np
import pytest
import yaml

from _util import PKG, ROOT, mix64, pkg

FULL = {"rotation_deg": 45.0, "scale": (0.9, 1.1), "flip_prob": 0.5, "point_drop": (0.05, 0.3)}
NEUTRAL = {"rotation_deg": 0.0, "scale": (1.0, 1.0), "flip_prob": 0.0, "point_drop": (0.0, 0.0)}
BOX_CFG = {"lidar_x_min": 0.0, "lidar_x_max": 70.4, "lidar_y_min": -40.0, "lidar_y_max": 40.0, "max_num_bbox": 20}


def _same(p, q):
    return (p["theta"], p["scale"], p["flip"], p["p"], p["drop_key"]) == (q["theta"], q["scale"], q["flip"], q["p"], q["drop_key"]) \
        and np.array_equal(p["a"], q["a"])


# ------------------------------------------------------------------------------------------------ draw
def test_export_declared_bound_and_built():
    H = pkg("_hip")
    header = open(os.path.join(ROOT, "include", "dcf_hip.h")).read()
    assert re.search(r"\bdcf_augment_points_batch\s*\(", header)
    assert "dcf_augment_points_batch" in H.SIGNATURES
    assert getattr(H.lib(), "dcf_augment_points_batch") is not None
    assert H.lib().dcf_version() == 202                    # an addition: the ABI version does not move
    assert callable(pkg("ops").augment_points_batch)


def test_draw_is_a_pure_function_of_its_arguments():
    A = pkg("augment")
    base = A.draw(FULL, 3, 1, 7, 2)
    assert _same(base, A.draw(dict(FULL), 3, 1, 7, 2))
    for other in ((4, 1, 7, 2), (3, 0, 7, 2), (3, 1, 8, 2), (3, 1, 7, 3)):
        q = A.draw(FULL, *other)
        assert q["theta"] != base["theta"] and q["scale"] != base["scale"] and q["p"] != base["p"] and q["drop_key"] != base["drop_key"], other


def test_draw_stays_inside_the_configured_ranges():
    A = pkg("augment")
    th, sc, fl, pp = [], [], [], []
    for i in range(10000):
        q = A.draw(FULL, 11, i % 4, i // 8, i % 8)
        th.append(q["theta"]); sc.append(q["scale"]); fl.append(q["flip"]); pp.append(q["p"])
        assert 0 <= q["drop_key"] < 1 << 64 and q["a"].dtype == np.float32 and q["a"].shape == (5,)
    th, sc, pp = np.degrees(np.array(th)), np.array(sc), np.array(pp)
    assert th.min() >= -45.0 and th.max() <= 45.0 and sc.min() >= 0.9 and sc.max() <= 1.1 and pp.min() >= 0.05 and pp.max() <= 0.3
    # ... and fills them: 10 000 uniform draws leave a gap of more than 1 % of the range at an end with probability 2e-44
    assert th.min() < -44.1 and th.max() > 44.1 and sc.min() < 0.902 and sc.max() > 1.098 and pp.min() < 0.0525 and pp.max() > 0.2975
    assert 0.45 < np.mean(fl) < 0.55                      # 10 000 fair coins: 10 sigma
    assert not any(A.draw(dict(FULL, flip_prob=0.0), 11, 0, i, 0)["flip"] for i in range(2000))
    assert all(A.draw(dict(FULL, flip_prob=1.0), 11, 0, i, 0)["flip"] for i in range(2000))


def test_neutral_config_draws_the_identity():
    A = pkg("augment")
    for i in range(50):
        q = A.draw(NEUTRAL, 5, i % 3, i, i % 4)
        assert q["theta"] == 0.0 and q["scale"] == 1.0 and q["flip"] is False and q["p"] == 0.0
        assert q["a"].tobytes() == np.array([1, 0, 0, 1, 1], dtype=np.float32).tobytes()      # +0.0 off the diagonal too
        assert A.drop_threshold(q) == 0 and A.keep_mask(1000, q).all()


def test_matrix_entries_are_the_issue_formulas_rounded_once():
    A = pkg("augment")
    for theta, s, flip in ((0.3, 1.07, False), (-1.1, 0.93, True), (math.pi / 2, 1.0, True)):
        f = -1.0 if flip else 1.0
        want = np.array([s * math.cos(theta), -s * math.sin(theta) * f, s * math.sin(theta), s * math.cos(theta) * f, s]).astype(np.float32)
        assert np.array_equal(A.params_from(theta, s, flip)["a"], want)


# ------------------------------------------------------------------------------------------------ points
def _points(n, seed):
    det = pkg("detfill")
    return det.synthetic_points(n, (0.0, 70.4, -40.0, 40.0, -2.4, 0.8), seed)


def test_transform_points_identity_and_float64_restatement():
    A = pkg("augment")
    pts = _points(5000, 3)
    assert A.transform_points(pts, A.identity()).tobytes() == pts.tobytes()
    q = A.params_from(math.radians(17.0), 1.03, True)
    got = A.transform_points(pts, q)
    assert got.dtype == np.float32 and got.shape == pts.shape
    want = pts.astype(np.float64) @ A.matrix3(q).T
    # two rounded products and a rounded sum per coordinate: each within half an ulp of a value no larger than |a| |x| + |b| |y|
    mag = np.abs(pts.astype(np.float64)) @ np.abs(A.matrix3(q)).T
    assert (np.abs(got - want) <= 1.5 * 2.0 ** -23 * mag + 1e-30).all()
    assert np.abs(got - want).max() > 0                   # (it IS fp32 arithmetic, not a rounded float64 result)


def test_keep_mask_is_the_documented_hash():
    A = pkg("augment")
    q = A.params_from(0.0, 1.0, False, p=0.3, drop_key=0x1234567890ABCDEF)
    keep = A.keep_mask(4000, q)
    thr = int(math.floor(0.3 * 2 ** 32))
    assert A.drop_threshold(q) == thr
    for i in range(0, 4000, 37):
        assert keep[i] == (not ((mix64(0x1234567890ABCDEF ^ mix64(i)) >> 32) < thr))
    assert 0.27 < 1.0 - keep.mean() < 0.33                # 4000 draws at p = 0.3: 4 sigma
    assert A.keep_mask(4000, A.params_from(0.0, 1.0, False, p=0.0, drop_key=77)).all()
    assert not A.keep_mask(4000, A.params_from(0.0, 1.0, False, p=1.0, drop_key=77)).any()


# ------------------------------------------------------------------------------------------------ projection matrix
@pytest.mark.parametrize("theta_deg,s,flip", [(17.0, 1.03, True), (-31.0, 0.91, False), (0.0, 1.0, True), (0.0, 0.5, False)])
def test_compose_crt_keeps_every_point_on_its_pixel(theta_deg, s, flip):
    A, calib = pkg("augment"), pkg("calib")
    crt = calib.kitti_like_crt()
    q = A.params_from(math.radians(theta_deg), s, flip)
    crt2 = A.compose_crt(crt, q)
    assert crt2.dtype == np.float32 and crt2.shape == (4, 3) and np.array_equal(crt2[3], np.asarray(crt, np.float32).reshape(4, 3)[3])
    # both sides in float64 from the fp32 A: the composed matrix before ITS rounding
    a = A.matrix3(q)
    c64 = np.asarray(crt, dtype=np.float64).reshape(4, 3)
    exact = c64.copy()
    exact[:3] = np.linalg.inv(a).T @ c64[:3]
    pts = _points(3000, 9).astype(np.float64)
    h = np.concatenate([pts, np.ones((len(pts), 1))], 1)
    front = (h @ c64)[:, 2] > 1.0                          # in-frustum side: a positive camera depth
    assert front.sum() > 1000
    lhs = np.concatenate([pts @ a.T, np.ones((len(pts), 1))], 1)[front] @ exact
    rhs = h[front] @ c64
    scale = np.abs(h[front]) @ np.abs(c64)
    assert (np.abs(lhs - rhs) <= 1e-9 * scale).all()
    # ... and compose_crt is that matrix rounded to fp32, entry by entry
    assert (np.abs(crt2.astype(np.float64) - exact) <= 2.0 ** -24 * np.abs(exact) + 1e-45).all()
    if theta_deg == 0.0 and s == 1.0:                      # flip alone: row 1 negated, exactly
        want = np.asarray(crt, np.float32).reshape(4, 3).copy()
        want[1] = -want[1]
        assert np.array_equal(crt2, want)
    if theta_deg == 0.0 and s == 0.5:                      # a power of two: exact doubles
        want = np.asarray(crt, np.float32).reshape(4, 3).copy()
        want[:3] *= 2
        assert np.array_equal(crt2, want)


# ------------------------------------------------------------------------------------------------ labels
def _boxes(n=6, seed=0):
    det = pkg("detfill")
    u = det.uniform((n, 7), 9300 + seed, 0.0, 1.0).astype(np.float64)
    b = np.zeros((BOX_CFG["max_num_bbox"], 9), dtype=np.float32)
    b[:n, 0] = 20.0 + 20.0 * u[:, 0]
    b[:n, 1] = -8.0 + 16.0 * u[:, 1]
    b[:n, 2] = -1.0 - 0.5 * u[:, 2]
    b[:n, 3] = 3.5 + 1.3 * u[:, 3]
    b[:n, 4] = 1.6 + 0.5 * u[:, 4]
    b[:n, 5] = 1.4 + 0.4 * u[:, 5]
    b[:n, 6] = 0.05 + 3.0 * u[:, 6]
    b[:n, 7], b[:n, 8] = 6, 1
    return b, n


def _corner_dev(EG, row_new, row_old, a):
    """Largest distance from a corner of bev_rect(row_new) to the nearest image under A of a corner of bev_rect(row_old), and back."""
    new = np.array(EG.bev_rect(row_new[:2], row_new[3:5], row_new[6]), dtype=np.float64)
    old = np.array(EG.bev_rect(row_old[:2], row_old[3:5], row_old[6]), dtype=np.float64) @ a[:2, :2].T
    d = np.linalg.norm(new[:, None, :] - old[None, :, :], axis=2)
    return max(d.min(1).max(), d.min(0).max())


PI_GAP = math.pi - 3.141592           # what one wrap by the dataset's literal turns a rectangle by, beyond half a turn


@pytest.mark.parametrize("theta_deg,s,flip", [(23.0, 1.0, False), (0.0, 1.0, True), (-14.0, 1.0, True), (9.0, 1.06, False), (-20.0, 0.94, True)])
def test_boxes_footprint_is_the_image_of_the_old_footprint(theta_deg, s, flip):
    """The four evalgeom.bev_rect corners of the new row are A applied to the old row's corners, as sets, in float64 (the rows asked
    for in float64: `dtype`) -- to 1e-9 where the yaw needs no wrap.  The dataset's orientation_inner_bound wraps by the literal
    3.141592, not pi, so a row it wraps k times is a rectangle turned by k (pi - 3.141592) = k 6.5e-7 rad: k times that angle
    times the half diagonal is allowed on top (a flip alone always wraps once: -yaw < 0).  The fp32 rows the trainer stores are
    the float64 rows rounded: checked entry by entry."""
    A, EG = pkg("augment"), pkg("evalgeom")
    q = A.params_from(math.radians(theta_deg), s, flip)
    a = A.matrix3(q)
    boxes, n = _boxes()
    new64, n64 = A.transform_boxes(boxes, n, q, BOX_CFG, dtype=np.float64)
    new32, n32 = A.transform_boxes(boxes, n, q, BOX_CFG)
    assert n64 == n32 == n and new32.dtype == np.float32 and new64.dtype == np.float64
    assert np.array_equal(new32, new64.astype(np.float32))
    wraps = 0
    for i in range(n):
        raw = A.box_image(boxes[i], q)[6]
        k = abs(round((raw - new64[i, 6]) / 3.141592))
        wraps += k
        half_diag = 0.5 * math.hypot(new64[i, 3], new64[i, 4])
        assert _corner_dev(EG, new64[i], boxes[i].astype(np.float64), a) <= 1e-9 + k * PI_GAP * half_diag
        assert 0.0 <= new64[i, 6] <= 3.141592 and 0.0 <= new32[i, 6] <= np.float32(3.141592)
        assert np.array_equal(new64[i, 7:], boxes[i, 7:].astype(np.float64))
        sxy = math.hypot(a[0, 0], a[1, 0])
        assert np.allclose(new64[i, [2, 5]], boxes[i, [2, 5]].astype(np.float64) * a[2, 2], rtol=1e-15)
        assert np.allclose(new64[i, 3:5], boxes[i, 3:5].astype(np.float64) * sxy, rtol=1e-15) and abs(sxy / s - 1.0) < 2.0 ** -22
    if not flip and theta_deg > 0:
        assert wraps < n                                  # the plain 1e-9 bound was really exercised
    assert not new64[n:].any() and not new32[n:].any()


def test_boxes_leaving_the_grid_are_removed_in_order():
    A = pkg("augment")
    boxes, n = _boxes()
    boxes[1, :2] = (60.0, 30.0)                           # turned by +40 degrees: y = 60 sin 40 + 30 cos 40 = 61.5 > lidar_y_max
    boxes[4, :2] = (5.0, -35.0)                           # x = 5 cos 40 + 35 sin 40 > 0, y = 5 sin 40 - 35 cos 40 = -23.6: stays
    q = A.params_from(math.radians(40.0), 1.0, False)
    new, k = A.transform_boxes(boxes, n, q, BOX_CFG)
    alone = [A.transform_boxes(boxes[i:i + 1], 1, q, BOX_CFG) for i in range(n)]
    keep = [i for i in range(n) if alone[i][1] == 1]
    assert 1 not in keep and 4 in keep and k == len(keep) < n
    for row, i in zip(new[:k], keep):
        assert np.array_equal(row, alone[i][0][0])
    assert not new[k:].any() and new.shape == boxes.shape
    # the identity keeps every row as it is (fp32 in, float64 arithmetic, fp32 out)
    same, ks = A.transform_boxes(boxes, n, A.identity(), BOX_CFG)
    assert ks == n and np.array_equal(same, boxes)
    # rows beyond num are ignored even when they hold data
    boxes[n] = boxes[0]
    assert np.array_equal(A.transform_boxes(boxes, n, A.identity(), BOX_CFG)[0][n], np.zeros(9, np.float32))


# ------------------------------------------------------------------------------------------------ config
def test_parse_augment_config_off_by_default_and_in_the_shipped_yaml():
    parse = pkg("train").parse_augment_config
    assert parse({}) is None
    assert parse({"augment": None}) is None
    assert parse({"augment": {"enabled": False, "rotation_deg": 10.0}}) is None
    with open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")) as f:
        shipped = yaml.safe_load(f)
    assert parse(shipped) is None
    blk = copy.deepcopy(shipped.get("augment") or {})
    assert blk.get("enabled", False) is False              # the block is documented there, switched off
    got = parse({"augment": {"enabled": True, "seed": 4, "rotation_deg": 20, "scale": [0.95, 1.05], "flip_prob": 0.5, "point_drop": [0.0, 0.1]}})
    assert got == {"seed": 4, "rotation_deg": 20.0, "scale": (0.95, 1.05), "flip_prob": 0.5, "point_drop": (0.0, 0.1)}
    assert parse({"augment": {"enabled": True}}) == {"seed": 0, "rotation_deg": 0.0, "scale": (1.0, 1.0), "flip_prob": 0.0, "point_drop": (0.0, 0.0)}


@pytest.mark.parametrize("enabled", [True, False])
@pytest.mark.parametrize("bad", [{"scale": [1.1, 0.9]}, {"point_drop": [0.4, 0.2]}, {"flip_prob": 1.5}, {"flip_prob": -0.1}, {"point_drop": [0.0, 1.2]},
                                 {"point_drop": [-0.1, 0.2]}, {"scale": [0.0, 1.0]}, {"scale": [-1.0, 1.0]}, {"rotation_deg": float("nan")},
                                 {"rotation_deg": float("inf")}, {"scale": [1.0, float("inf")]}, {"flip_prob": float("nan")},
                                 {"point_drop": [0.0, float("nan")]}, {"rotation_deg": -5.0}, {"scale": 1.0}, {"scale": [1.0]},
                                 {"rotation_deg": "ten"}, {"enabled": "yes"}, {"seed": 1.5}, {"rotatoin_deg": 10.0}])
def test_parse_augment_config_rejects_bad_values(bad, enabled):
    parse = pkg("train").parse_augment_config
    blk = {"enabled": enabled}
    blk.update(bad)
    with pytest.raises(ValueError):
        parse({"augment": blk})


def test_parse_augment_config_rejects_a_non_mapping():
    with pytest.raises(ValueError):
        pkg("train").parse_augment_config({"augment": True})

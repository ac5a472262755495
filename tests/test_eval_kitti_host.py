"""CPU suite: the host statement of the KITTI-style protocol (`eval_protocol: kitti`; evalkitti.py) against
restatements by hand -- levels, the dataset's two extra tensors, the 3-D IoU, the projected flags, the three-outcome matching, AP
with ignored detections -- and its reduction to the plain ranked evaluation (evalrank.py) when nothing is ignored."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from _util import golden_cfg, load_golden, pkg

THR = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]


def EK():
    return pkg("evalkitti")


def ER():
    return pkg("evalrank")


def bits(mask, d):
    """The ten threshold bits of difficulty d."""
    return (int(mask) >> (10 * d)) & 0x3FF


# ------------------------------------------------------------------ levels
def test_difficulty_levels_with_closed_boundaries():
    L = EK().difficulty_level
    assert L("Car", 40.0, 0, 0.15) == 0                                  # all three bounds are closed
    assert L("Car", 39.999, 0, 0.0) == 1 and L("Car", 25.0, 0, 0.0) == 1
    assert L("Car", 24.999, 0, 0.0) == 3
    assert L("Car", 100.0, 0, 0.1500001) == 1 and L("Car", 100.0, 0, 0.30) == 1
    assert L("Car", 100.0, 0, 0.31) == 2 and L("Car", 100.0, 0, 0.50) == 2 and L("Car", 100.0, 0, 0.51) == 3
    assert [L("Car", 100.0, o, 0.0) for o in (0, 1, 2, 3)] == [0, 1, 2, 3]
    assert L("Car", 30.0, 2, 0.1) == 2 and L("Car", 30.0, 0, 0.4) == 2
    assert L("Van", 100.0, 0, 0.0) == 3
    s = EK().settings({"eval_min_height": [50, 30, 10], "eval_max_occlusion": [0, 0, 1], "eval_max_truncation": [0.1, 0.2, 0.9]})
    assert L("Car", 45.0, 0, 0.0, s) == 1 and L("Car", 12.0, 1, 0.8, s) == 2 and L("Car", 60.0, 1, 0.05, s) == 2


# ------------------------------------------------------------------ KittiDataset on a written tree
def tiny_cfg(**kw):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dataset_name="kitti"))
    cfg.update(kw)
    return cfg


# (type, truncation, occlusion, top, bottom) of the label lines inside the grid, in file order, and the level each must get
LINES = [("Car", 0.0, 0, 10.0, 50.0, 0), ("Van", 0.0, 0, 10.0, 90.0, 3), ("Car", 0.2, 1, 10.0, 35.0, 1), ("Car", 0.4, 2, 10.0, 36.0, 2),
         ("Car", 0.0, 3, 10.0, 80.0, 3), ("Car", 0.15, 0, 10.0, 49.0, 1)]
DONTCARE = [(5.0, 6.0, 30.5, 40.25), (100.0, 10.0, 120.0, 20.0)]


def write_tree(root, cfg, n_dontcare=None):
    det = pkg("detfill")
    d = os.path.join(root, "training")
    for sub in ("velodyne", "image_2", "calib", "label_2"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    from PIL import Image
    lim6 = (cfg["lidar_x_min"], cfg["lidar_x_max"], cfg["lidar_y_min"], cfg["lidar_y_max"], cfg["lidar_z_min"], cfg["lidar_z_max"])
    pts = det.synthetic_points(300, lim6, 11)
    np.concatenate([pts, np.full((pts.shape[0], 1), 0.5, np.float32)], 1).astype(np.float32).tofile(os.path.join(d, "velodyne", "000000.bin"))
    Image.fromarray(np.zeros((94, 126, 3), np.uint8)).save(os.path.join(d, "image_2", "000000.png"))
    P2 = np.array([[60.0, 0.0, 64.0, 4.5], [0.0, 60.0, 48.0, 0.2], [0.0, 0.0, 1.0, 0.003]])
    R0 = np.eye(3)
    Tr = np.concatenate([pkg("calib").R_LIDAR_TO_CAM, np.array([[0.1], [-0.2], [0.05]])], 1)
    with open(os.path.join(d, "calib", "000000.txt"), "w") as f:
        f.write("P2: " + " ".join("%.12e" % v for v in P2.reshape(-1)) + "\n")
        f.write("R0_rect: " + " ".join("%.12e" % v for v in R0.reshape(-1)) + "\n")
        f.write("Tr_velo_to_cam: " + " ".join("%.12e" % v for v in Tr.reshape(-1)) + "\n")
    T4 = np.eye(4)
    T4[:3, :4] = Tr
    dc = DONTCARE if n_dontcare is None else [(float(k), 1.0, float(k) + 2.0, 5.0) for k in range(n_dontcare)]
    with open(os.path.join(d, "label_2", "000000.txt"), "w") as f:
        f.write("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n" % dc[0])
        f.write("Pedestrian 0 0 0 1 2 3 4 1.7 0.5 0.5 1 1 10 0\n")
        for k, (typ, trunc, occ, top, bottom, _) in enumerate(LINES):
            x = lim6[0] + (0.15 + 0.1 * k) * (lim6[1] - lim6[0])
            c = T4 @ np.array([x, 0.2 * lim6[3], -1.0, 1.0])
            f.write("%s %.7f %d 0.0 20.0 %.3f 60.0 %.3f 1.5 1.8 4.0 %.9f %.9f %.9f -1.7\n" % (typ, trunc, occ, top, bottom, c[0], c[1] + 0.75, c[2]))
            if k == 2:                                                  # a car outside the grid between the rows: no row, no level
                f.write("Car 0.0 0 0.0 0 0 10 100 1.5 1.8 4.0 0.0 1.0 %.3f 0.0\n" % (lim6[1] + 50.0))
        for rc in dc[1:]:
            f.write("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n" % rc)


def test_kitti_dataset_carries_levels_and_dontcare_only_under_the_protocol(tmp_path):
    K = pkg("data_import_kitti")
    cfg = tiny_cfg()
    write_tree(str(tmp_path), cfg)
    plain = K.KittiDataset(cfg, root=str(tmp_path), raw=True)[0]
    assert set(plain) == {"image", "bboxes", "num_bboxes", "lidar_points", "crt"}
    s = K.KittiDataset(tiny_cfg(eval_metric="ranked", eval_protocol="kitti"), root=str(tmp_path), raw=True)[0]
    assert set(s) == set(plain) | {"bbox_level", "dontcare"}
    assert torch.equal(s["bboxes"], plain["bboxes"]) and s["num_bboxes"] == plain["num_bboxes"] == len(LINES)
    mx = int(cfg["max_num_bbox"])
    assert s["bbox_level"].dtype == torch.int32 and tuple(s["bbox_level"].shape) == (mx,)
    assert s["bbox_level"].tolist() == [row[5] for row in LINES] + [3] * (mx - len(LINES))
    assert s["dontcare"].dtype == torch.float32 and tuple(s["dontcare"].shape) == (64, 4)
    assert s["dontcare"][:2].tolist() == [list(rc) for rc in DONTCARE] and not s["dontcare"][2:].any()
    # the loader carries both as stacked host tensors, next to bboxes
    FL = pkg("frame_loader")
    ds = K.KittiDataset(tiny_cfg(eval_metric="ranked", eval_protocol="kitti", eval_max_dontcare=3), root=str(tmp_path), raw=True)
    batch = next(iter(FL.FrameLoader(ds, 1, device=None)))
    assert tuple(batch["bbox_level"].shape) == (1, mx) and tuple(batch["dontcare"].shape) == (1, 3, 4) and tuple(batch["bboxes"].shape) == (1, mx, 9)
    assert "bbox_level" not in next(iter(FL.FrameLoader(K.KittiDataset(cfg, root=str(tmp_path), raw=True), 1, device=None)))


def test_kitti_dataset_raises_on_too_many_dontcare_lines(tmp_path):
    K = pkg("data_import_kitti")
    cfg = tiny_cfg(eval_metric="ranked", eval_protocol="kitti")
    write_tree(str(tmp_path), cfg, n_dontcare=65)
    with pytest.raises(ValueError, match="eval_max_dontcare"):
        K.KittiDataset(cfg, root=str(tmp_path), raw=True)[0]
    assert tuple(K.KittiDataset(dict(cfg, eval_max_dontcare=65), root=str(tmp_path), raw=True)[0]["dontcare"].shape) == (65, 4)
    with pytest.raises(ValueError, match="eval_metric"):
        K.KittiDataset(tiny_cfg(eval_protocol="kitti"), root=str(tmp_path), raw=True)


# ------------------------------------------------------------------ IoU
def test_iou_pair_against_exact_rationals():
    iou = EK().iou_pair
    a = [0.0, 0.0, 0.0, 4.0, 2.0, 2.0, 0.0]
    # shifted by (1, 0.5, 0.5): overlap 3 x 1.5 x 1.5 = 6.75 of 16 + 16 - 6.75
    bev, i3d = iou(a, [1.0, 0.5, 0.5, 4.0, 2.0, 2.0, 0.0])
    assert abs(bev - float(Fraction(9, 2) / (16 - Fraction(9, 2)))) <= 1e-15 and abs(i3d - float(Fraction(27, 4) / (32 - Fraction(27, 4)))) <= 1e-15
    # equal footprints, half the z extent shared: bev 1, 3-D 1/3
    bev, i3d = iou(a, [0.0, 0.0, 1.0, 4.0, 2.0, 2.0, 0.0])
    assert bev == 1.0 and abs(i3d - 1.0 / 3.0) <= 1e-15
    # different heights: 8 x 1 shared of 8 x 2 + 8 x 1
    assert abs(iou(a, [0.0, 0.0, 0.5, 4.0, 2.0, 1.0, 0.0])[1] - 0.5) <= 1e-15
    # disjoint in z (and touching): 0, the bird's-eye value unchanged
    assert iou(a, [0.0, 0.0, 2.5, 4.0, 2.0, 2.0, 0.0]) == (1.0, 0.0) and iou(a, [0.0, 0.0, 2.0, 4.0, 2.0, 2.0, 0.0]) == (1.0, 0.0)
    # zero volume on both sides: NaN, which compares false everywhere
    z = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert all(math.isnan(v) for v in iou(z, z))


def test_bev_value_is_bit_equal_to_evalrank():
    det = pkg("detfill")
    u = det.uniform((40, 7), 9100, 0.0, 1.0)
    b = np.stack([u[:, 0] * 6, u[:, 1] * 6, -1 + 0.5 * u[:, 2], 3.5 + 1.3 * u[:, 3], 1.6 + 0.5 * u[:, 4], 1.4 + 0.4 * u[:, 5], 3.14159 * u[:, 6]], 1).astype(np.float32)
    pos = 0
    for i in range(20):
        for j in range(20, 40):
            want = ER().bev_iou(b[i].astype(np.float64), b[j].astype(np.float64))
            got = EK().iou_pair(b[i], b[j])
            assert np.float64(got[0]).tobytes() == np.float64(want).tobytes()
            assert 0.0 <= got[1] <= got[0] + 1e-15
            pos += got[1] > 0
    assert pos > 20


# ------------------------------------------------------------------ det_flags
F, CX, CY, IH, IW = 100.0, 320.0, 240.0, 480, 640
PINHOLE = np.array([[CX, CY, 1.0], [-F, 0.0, 0.0], [0.0, -F, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)      # depth = x, u = cx - f y / x, v = cy - f z / x


def test_det_flags_projection_clamping_and_dontcare():
    E = EK()
    # a box whose nearest face is at depth D projects to height f h / D
    for D, h in ((10.0, 1.5), (7.3, 1.7), (31.0, 1.45)):
        p = E.project_box([D + 2.0, 0.3, -0.2, 4.0, 1.8, h, 0.0], PINHOLE, IH, IW)
        assert abs(p[4] - F * h / D) <= 1e-9 and p[5] > 0
    s = E.settings({})
    flags = E.det_flags([[2.5 + 2.0, 0.0, 0.0, 4.0, 1.8, 1.5, 0.0],          # 60 px: no bit
                         [3.0 + 2.0, 0.0, 0.0, 4.0, 1.8, 1.05, 0.0],         # 35 px: below easy only
                         [8.0 + 2.0, 0.0, 0.0, 4.0, 1.8, 1.6, 0.0]], PINHOLE, IH, IW, None, s)
    assert flags.tolist() == [0, 1, 7]
    # four corners behind the camera: only the face at depth 2 takes part
    p = E.project_box([0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0], PINHOLE, IH, IW)
    assert p == (CX - 50.0, CY - 37.5, CX + 50.0, CY + 37.5, 75.0, 7500.0)
    # all corners behind: height and area 0 -- every height bit, and no DontCare bit even under a rectangle over the whole image
    everything = np.array([[0.0, 0.0, IW, IH]], np.float32)
    assert E.project_box([-10.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0], PINHOLE, IH, IW)[4:] == (0.0, 0.0)
    assert E.det_flags([[-10.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0]], PINHOLE, IH, IW, everything, s).tolist() == [7]
    # clamping at the image border: a box 0.5 m in front fills the image
    p = E.project_box([2.5, 0.0, 0.0, 4.0, 8.0, 6.0, 0.0], PINHOLE, IH, IW)
    assert p == (0.0, 0.0, float(IW), float(IH), float(IH), float(IW * IH))
    # DontCare: a flat box at depth 10 projects to (310, 232.5, 330, 247.5), all exact; half of it is not "more than 0.5"
    box = [[10.0, 0.0, 0.0, 0.0, 2.0, 1.5, 0.0]]
    assert E.project_box(box[0], PINHOLE, IH, IW) == (310.0, 232.5, 330.0, 247.5, 15.0, 300.0)
    half = np.array([[0.0, 0.0, 1.0, 1.0], [300.0, 200.0, 320.0, 300.0]], np.float32)
    over = np.array([[0.0, 0.0, 1.0, 1.0], [300.0, 200.0, 320.01, 300.0]], np.float32)
    assert E.dontcare_ratio(E.project_box(box[0], PINHOLE, IH, IW), half[1]) == 0.5
    assert E.det_flags(box, PINHOLE, IH, IW, half, s).tolist() == [7] and E.det_flags(box, PINHOLE, IH, IW, over, s).tolist() == [15]
    assert E.det_flags(box, PINHOLE, IH, IW, everything, E.settings({"eval_dontcare_overlap": 1.0})).tolist() == [7]      # 1.0 is not > 1.0
    assert E.det_flags(box, PINHOLE, IH, IW, np.zeros((4, 4), np.float32), s).tolist() == [7]                       # unused rows overlap nothing


# ------------------------------------------------------------------ matching
def run_match(iou, levels, flags, valid=None, iou3=None):
    iou = np.asarray(iou, dtype=np.float64)
    n, R = iou.shape
    refs = np.zeros((R, 9), np.float32)
    refs[:, 8] = 1.0 if valid is None else valid
    return EK().match_levels(np.ones(n, np.int32), refs, levels, iou, iou if iou3 is None else np.asarray(iou3, np.float64), np.asarray(flags, np.uint32), THR)


def below(x):
    """The thresholds strictly below x, as a bit field."""
    return sum(1 << t for t, thr in enumerate(THR) if x > thr)


def test_matching_outcomes():
    # a detection on a level-3 row is ignored at every difficulty, at the thresholds its IoU exceeds; above them it is a false positive
    tp, ig = run_match([[0.72]], [3], [0])
    assert tp[0, 0] == 0 and [bits(ig[0, 0], d) for d in range(3)] == [below(0.72)] * 3 and below(0.72) == 0b11111
    # on a level-1 row: ignored at easy, a true positive at moderate and hard
    tp, ig = run_match([[0.72]], [1], [0])
    assert [bits(tp[0, 0], d) for d in range(3)] == [0, 0b11111, 0b11111] and [bits(ig[0, 0], d) for d in range(3)] == [0b11111, 0, 0]
    # a counted row with a lower IoU above t wins over an ignored row with a higher IoU; where only the ignored one exceeds t: ignored
    tp, ig = run_match([[0.62, 0.91]], [0, 3], [0])
    assert [bits(tp[0, 0], d) for d in range(3)] == [below(0.62)] * 3
    assert [bits(ig[0, 0], d) for d in range(3)] == [below(0.91) & ~below(0.62)] * 3
    # a second detection on a taken row is a false positive; ignored when flagged (DontCare bit, or the height bit of that difficulty)
    tp, ig = run_match([[0.97], [0.97], [0.97], [0.97]], [0], [0, 0, 8, 2])
    assert tp[0].tolist() == [0x3FFFFFFF, 0, 0, 0]
    assert ig[0].tolist() == [0, 0, 0x3FFFFFFF, 0x3FF << 10]
    # ignored rows are never taken: they absorb any number of detections
    tp, ig = run_match([[0.97], [0.97], [0.97]], [2], [0, 0, 0])
    assert [bits(x, 2) for x in tp[0]] == [0x3FF, 0, 0] and [bits(x, 1) for x in ig[0]] == [0x3FF] * 3 and [bits(x, 1) for x in tp[0]] == [0] * 3
    # an unmatched detection of height 30 (bit 0 only): ignored at easy, a false positive at moderate and hard
    f30 = int(EK().det_flags([[3.0 + 2.0, 0.0, 0.0, 4.0, 1.8, 0.9, 0.0]], PINHOLE, IH, IW)[0])
    assert f30 == 1
    tp, ig = run_match([[0.1]], [0], [f30])
    assert tp[0, 0] == 0 and [bits(ig[0, 0], d) for d in range(3)] == [0x3FF, 0, 0]
    # rows with ref[:, 8] != 1 do not exist; NaN never wins and never ignores; the two metrics are independent
    tp, ig = run_match([[0.97, float("nan")]], [0, 3], [0], valid=[0.0, 1.0])
    assert tp[0, 0] == 0 and ig[0, 0] == 0
    tp, ig = run_match([[0.97]], [0], [0], iou3=[[0.52]])
    assert tp[0, 0] == 0x3FFFFFFF and [bits(tp[1, 0], d) for d in range(3)] == [1, 1, 1] and ig.sum() == 0


# ------------------------------------------------------------------ AP with ignored detections
def random_marks(N, seed):
    det = pkg("detfill")
    scores = (np.round(det.uniform((N,), seed, 0.5, 1.0) * 32.0) / 32.0).astype(np.float32)        # heavily tied
    u = det.uniform((4, N, 30), seed + 1, 0.0, 1.0)
    tp = np.zeros((2, N), np.uint32)
    ig = np.zeros((2, N), np.uint32)
    for m in range(2):
        for k in range(30):
            tp[m] |= (u[m, :, k] < 0.7 - 0.015 * k).astype(np.uint32) << np.uint32(k)
            ig[m] |= (u[2 + m, :, k] < 0.1 + 0.01 * k).astype(np.uint32) << np.uint32(k)
    return scores, tp, ig


def test_average_precision_deletes_the_ignored_detections():
    N = 300
    scores, tp, ig = random_marks(N, 9200)
    n_gt = [7, 150, 0]
    ap, c, nig = EK().average_precision_levels(scores, tp, ig, n_gt, 10)
    for m in range(2):
        for d in range(3):
            for t in range(10):
                k = 10 * d + t
                stay = ((ig[m] >> k) & 1) == 0
                a, cc = ER().average_precision(scores[stay], ((tp[m] >> k) & 1)[stay].astype(np.uint32), n_gt[d], 1)
                assert np.float64(ap[m, d, t]).tobytes() == np.float64(a[0]).tobytes() and c[m, d, t] == cc[0] and nig[m, d, t] == N - stay.sum()
    assert np.isnan(ap[:, 2]).all() and not np.isnan(ap[:, :2]).any() and (nig > 0).all()
    # by hand: scores 0.9 .. 0.6, the second detection ignored at (bev, easy, 0.5) only, true positives first and last, n_gt = 2
    #   easy: the list (1, 0, 1): p = 1, 1/2, 2/3 at levels 20, 20, 40 -> AP = (20 + 20 x 2/3) / 40 = 5/6
    #   moderate: the list (1, 1, 0, 1) (the second is a true positive there), n_gt = 3: p = 1, 1, 2/3, 3/4 at levels 13, 26, 26, 40
    #             -> AP = (26 + 14 x 3/4) / 40
    scores = np.array([0.9, 0.8, 0.7, 0.6], np.float32)
    tp = np.zeros((2, 4), np.uint32)
    ig = np.zeros((2, 4), np.uint32)
    tp[0] = [1 | 1 << 10, 1 << 10, 0, 1 | 1 << 10]
    ig[0, 1] = 1
    s = EK().summarize(scores, tp, ig, [2, 3, 3], THR, truncated=2)
    assert abs(s["bev"]["easy"]["ap"][0.5] - float(Fraction(5, 6))) <= 1e-15
    assert abs(s["bev"]["moderate"]["ap"][0.5] - float((26 + 14 * Fraction(3, 4)) / 40)) <= 1e-15
    e, mo = s["bev"]["easy"], s["bev"]["moderate"]
    assert (e["tp"][0.5], e["num_ignored"][0.5], e["precision"][0.5], e["recall"][0.5], e["num_T"]) == (2, 1, 2 / 3, 1.0, 2)
    assert (mo["tp"][0.5], mo["num_ignored"][0.5], mo["precision"][0.5], mo["recall"][0.5], mo["num_T"]) == (3, 0, 0.75, 1.0, 3)
    assert e["ap"][0.55] == 0.0 and e["num_ignored"][0.55] == 0 and abs(e["map"] - float(Fraction(5, 6)) / 10) <= 1e-15
    assert (s["protocol"], s["num_P"], s["truncated_candidates"]) == ("kitti", 4, 2)
    assert set(s) == {"protocol", "bev", "3d", "num_P", "truncated_candidates"} and set(s["3d"]) == {"easy", "moderate", "hard"}
    assert set(e) == {"ap", "map", "tp", "precision", "recall", "num_T", "num_ignored"}
    line = EK().report_line(s, 0.5)
    assert "3-D 0.0000 / 0.0000 / 0.0000" in line and "bird's-eye 0.8333 / 0.9125 / " in line


# ------------------------------------------------------------------ reduction to the plain ranked evaluation
def test_protocol_reduces_to_the_plain_ranked_evaluation():
    det = pkg("detfill")
    n, G = 240, 24

    def mapped(u, span):
        return np.stack([u[:, 0] * span, u[:, 1] * span, -1.0 + 0.2 * u[:, 2], 3.5 + 1.3 * u[:, 3], 1.6 + 0.5 * u[:, 4], 1.4 + 0.4 * u[:, 5],
                         3.14159 * u[:, 6]], 1).astype(np.float32)
    u = det.uniform((n, 8), 9300, 0.0, 1.0)
    span = 3.0 * np.sqrt(n)
    boxes = mapped(u, span)
    labels = mapped(det.uniform((G, 7), 9301, 0.0, 1.0), span)
    for i in range(4 * G):
        s = 0.02 * (1 + i // G) ** 2
        boxes[i] = (labels[i % G].astype(np.float64) + (u[i, :7].astype(np.float64) - 0.5) * np.array([4 * s, 4 * s, 0.1, s, s, 0.1, 0.5 * s])).astype(np.float32)
    scores = (np.round(u[:, 7] * 64.0) / 64.0).astype(np.float32)
    order = np.argsort(ER().rank_keys(scores, np.arange(n)))[::-1]
    boxes, scores = np.ascontiguousarray(boxes[order]), scores[order]
    refs = np.zeros((G + 2, 9), np.float32)
    refs[1:G + 1, :7], refs[1:G + 1, 8] = labels, 1.0
    keep = ER().nms(boxes, 0.1)
    assert keep.sum() > 100
    want = ER().match(boxes, keep, refs, THR)
    assert (want & 1).sum() >= 10
    settings = EK().settings({"eval_min_height": [0, 0, 0]})
    C = np.array([[64.0, 48.0, 1.0], [-60.0, 0.0, 0.0], [0.0, -60.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    flags = EK().det_flags(boxes, C, 96, 128, None, settings)
    assert not flags.any()
    bev, i3d = EK().iou_matrices(boxes, keep, refs)
    assert np.array_equal(np.isnan(bev), np.isnan(ER().iou_matrix(boxes, keep, refs))) and np.array_equal(bev[~np.isnan(bev)], ER().iou_matrix(boxes, keep, refs)[~np.isnan(bev)])
    tp, ig = EK().match_levels(keep, refs, None, bev, i3d, flags, THR)
    assert not ig.any()
    assert tp[0].tolist() == (want | (want << np.uint32(10)) | (want << np.uint32(20))).tolist()
    assert 0 < (tp[1] & 1).sum() <= (tp[0] & 1).sum()                   # (the 3-D matching is its own one-to-one assignment)
    sel = keep != 0
    got = EK().summarize(scores[sel], tp[:, sel], ig[:, sel], EK().count_rows(refs), THR, truncated=1)
    plain = ER().summarize(scores[sel], want[sel], G, THR, truncated=1)
    for name in ("easy", "moderate", "hard"):
        lvl = got["bev"][name]
        for key in ("ap", "tp", "precision", "recall"):
            assert {t: np.float64(v).tobytes() for t, v in lvl[key].items()} == {t: np.float64(v).tobytes() for t, v in plain[key].items()}, (name, key)
        assert np.float64(lvl["map"]).tobytes() == np.float64(plain["map"]).tobytes() and lvl["num_T"] == plain["num_T"] == G
        assert set(lvl["num_ignored"].values()) == {0}
    assert got["num_P"] == plain["num_P"] and got["truncated_candidates"] == plain["truncated_candidates"] == 1


# ------------------------------------------------------------------ construction and the CPU path of RankedTest
def test_construction_raises_on_bad_values():
    Tm, TR = pkg("test"), pkg("train")
    net = torch.nn.Identity()
    base = {"score_threshold": 0.5, "eval_metric": "ranked", "eval_protocol": "kitti"}
    for bad in ({"eval_min_height": [40, 25]}, {"eval_max_occlusion": [0, 1, 2, 3]}, {"eval_max_truncation": 0.5}, {"eval_min_height": [40, -1, 25]},
                {"eval_dontcare_overlap": 0.0}, {"eval_dontcare_overlap": 1.5}, {"eval_report_iou": 0.72}, {"eval_protocol": "official"}):
        with pytest.raises(ValueError):
            Tm.RankedTest(net, dict(base, **bad))
        with pytest.raises(ValueError):
            TR.make_tester(net, dict(base, **bad))
    for metric in ({"eval_metric": "compat"}, {"eval_metric": None}):
        with pytest.raises(ValueError, match="eval_metric"):
            TR.make_tester(net, dict(base, **metric))
        with pytest.raises(ValueError, match="eval_metric"):
            Tm.RankedTest(net, dict(base, **metric))
    s = EK().settings(dict(base, eval_report_iou=0.5, eval_dontcare_overlap=1.0), THR)
    assert s["report_iou"] == 0.5 and s["min_height"] == (40.0, 25.0, 25.0) and s["max_occlusion"] == (0, 1, 2) and s["max_dontcare"] == 64


def harness(**cfg):
    Tm = pkg("test")
    T = Tm.RankedTest.__new__(Tm.RankedTest)
    torch.nn.Module.__init__(T)
    T.config = dict({"score_threshold": 0.5, "image_height": IH, "image_width": IW}, **cfg)
    T.initialize_ap()
    return T


def test_ranked_test_on_cpu_tensors_runs_the_host_statement():
    """Three detections on three labelled cars of levels 0 / 2 / 3 and one on nothing, through RankedTest.accumulate on CPU tensors."""
    pred = np.zeros((1, 32, 2, 4), np.float32)
    cars = [[10.0, 0.0, 0.0, 4.0, 1.8, 1.5, 0.0], [20.0, 4.0, 0.0, 4.0, 1.8, 1.5, 0.0], [30.0, -6.0, 0.0, 4.0, 1.8, 1.5, 0.0]]
    dets = cars + [[15.0, 12.0, 0.0, 4.0, 1.8, 1.5, 0.0]]
    for px, (box, score) in enumerate(zip(dets, (0.9, 0.8, 0.7, 0.6))):
        pred[0, 1, 0, px] = score
        pred[0, 18:25, 0, px] = box
    refs = np.zeros((1, 5, 9), np.float32)
    refs[0, :3, :7], refs[0, :3, 8] = cars, 1.0
    levels = torch.tensor([[0, 2, 3, 3, 3]], dtype=torch.int32)
    T = harness(eval_metric="ranked", eval_protocol="kitti")
    T.accumulate(torch.from_numpy(pred), torch.from_numpy(refs), levels=levels, dontcare=torch.zeros(1, 0, 4), crt=[torch.from_numpy(PINHOLE)])
    s = T.summary()
    assert s["num_P"] == 4 and [s["bev"][k]["num_T"] for k in ("easy", "moderate", "hard")] == [1, 1, 2]
    assert [s["3d"][k]["tp"][0.7] for k in ("easy", "moderate", "hard")] == [1, 1, 2]
    # heights: 100 x 1.5 / 8 = 18.75 px (below every minimum), 8.3 px, 5.4 px, 11.5 px: the unmatched detections are all ignored
    assert [s["bev"][k]["num_ignored"][0.7] for k in ("easy", "moderate", "hard")] == [3, 3, 2]
    assert [s["bev"][k]["ap"][0.7] for k in ("easy", "moderate", "hard")] == [1.0, 1.0, 1.0]
    assert (T.get_num_P(), T.get_num_T(), T.get_num_TP_set()[0.7]) == (4, 1, 1)
    # without levels every row is level 0; without the key the evaluator is the plain one and takes no extra input
    T.initialize_ap()
    T.accumulate(torch.from_numpy(pred), torch.from_numpy(refs))
    assert [T.summary()["bev"][k]["num_T"] for k in ("easy", "moderate", "hard")] == [3, 3, 3] and T.summary()["bev"]["easy"]["tp"][0.7] == 3
    P = harness(eval_metric="ranked")
    P.accumulate(torch.from_numpy(pred), torch.from_numpy(refs))
    assert "protocol" not in P.summary() and P.summary()["tp"][0.7] == 3 and P.summary()["num_T"] == 3


def test_evaluate_hands_the_protocol_inputs_to_the_tester_and_none_to_a_plain_one():
    import types
    TR, FL = pkg("train"), pkg("frame_loader")
    own, default = torch.full((4, 3), 2.0), np.full((4, 3), 7.0, np.float32)
    batch = FL.Batch(points=["p0", "p1"], image="img", bboxes="bb", num_bboxes="nb", crt=[own, None], bbox_level="lv", dontcare="dc")
    training = types.SimpleNamespace(recipe=None, geometry_async=lambda g, pts, crts=None, wait_event=None: ("x", "geom"))
    dataset = types.SimpleNamespace(geometry=types.SimpleNamespace(crt=default))
    for cfg, keys in (({"eval_protocol": "kitti"}, {"geom", "levels", "dontcare", "crt"}), ({}, {"geom"})):
        T = harness(eval_metric="ranked", **cfg)
        seen = []
        T.get_eval_value_onestep = lambda *a, **kw: (seen.append((a, kw)), (1.5, None))[1]
        mean, cum, num_p, num_t, tp = TR.evaluate(training, T, dataset, [batch])
        (a, kw), = seen
        assert a == ("x", "img", "bb", "nb") and set(kw) == keys and (mean, num_p, num_t) == (1.5, 0, 0) and set(tp) == set(THR)
        if cfg:
            assert (kw["levels"], kw["dontcare"]) == ("lv", "dc") and kw["crt"][0] is own and kw["crt"][1] is default

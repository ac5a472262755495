"""CPU suite: the host statement of the ranked evaluation (evalrank.py; `eval_metric: ranked`) against
restatements written here -- ranking, bird's-eye IoU, suppression order, one-to-one matching, KITTI R40 average precision -- and
the RankedTest switch, summary and accumulator overflow on CPU tensors."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from _util import pkg

THR = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]


def ER():
    return pkg("evalrank")


def make_pred(B, h, w, seed, nan_every=0):
    """pred [B,32,h,w] with scores quantised to 1/64 in [-0.5, 1] (ties within and across anchors)."""
    det = pkg("detfill")
    pred = det.uniform((B, 32, h, w), seed, -1.0, 1.0)
    for a in range(2):
        s = np.round(det.uniform((B, h, w), seed + 1 + a, -0.5, 1.0) * 64.0) / 64.0 + 0.0       # + 0.0: no -0.0
        if nan_every:
            s.reshape(-1)[a::nan_every] = np.nan
        pred[:, 2 * a + 1] = s.astype(np.float32)
    return pred


def restated_order(pred, b, thr):
    hw = pred.shape[2] * pred.shape[3]
    p = pred.reshape(pred.shape[0], 32, hw)
    cand = [(float(p[b, 2 * a + 1, px]), a * hw + px) for a in range(2) for px in range(hw) if p[b, 2 * a + 1, px] > np.float32(thr)]
    return sorted(cand, key=lambda c: (-c[0], c[1]))


@pytest.mark.parametrize("thr", [-0.25, 0.5])
def test_ranking_equals_sorted_restatement(thr):
    pred = make_pred(2, 6, 7, 9100, nan_every=5)
    hw = 42
    p = pred.reshape(2, 32, hw)
    full = [restated_order(pred, b, thr) for b in range(2)]
    assert all(len(set(s for s, _ in o)) < len(o) for o in full), "the scores must tie"
    for cap in (4096, 7, 1):
        boxes, scores, count, total = ER().rank_filter(pred, thr, cap)
        for b in range(2):
            want = full[b][:cap]
            assert total[b] == len(full[b]) and count[b] == len(want)
            assert scores[b, :count[b]].tolist() == [s for s, _ in want]
            exp = np.array([[p[b, 18 + 7 * (i // hw) + k, i % hw] for k in range(7)] for _, i in want], dtype=np.float32).reshape(-1, 7)
            assert np.array_equal(boxes[b, :count[b]], exp)
            assert not boxes[b, count[b]:].any() and not scores[b, count[b]:].any()
    assert not np.isnan(ER().rank_filter(pred, thr, 4096)[1]).any(), "a NaN score is never kept"


def test_orderable_key_is_a_total_order():
    s = np.array([-np.inf, -2.5, -1e-30, -0.0, 0.0, 1e-30, 0.5, 0.5000001, 3.0, np.inf], dtype=np.float32)
    u = ER().orderable_u32(s)
    assert all(int(u[i]) < int(u[i + 1]) for i in range(len(u) - 1))
    k = ER().rank_keys(np.array([0.5, 0.5], dtype=np.float32), np.array([3, 4]))
    assert int(k[0]) > int(k[1]), "ties go to the lower index"


def box(x, y, l=4.0, w=2.0, yaw=0.0):
    return np.array([x, y, -1.0, l, w, 1.5, yaw], dtype=np.float64)


def test_bev_iou_hand_values():
    iou = ER().bev_iou
    assert abs(iou(box(1.3, 2.7, 3.9, 1.7, 0.4), box(1.3, 2.7, 3.9, 1.7, 0.4)) - 1.0) < 1e-12
    assert iou(box(0, 0), box(10, 0)) == 0.0
    assert abs(iou(box(0, 0), box(2, 0)) - 1.0 / 3.0) < 1e-12
    # 4 x 2 against 6 x 2 turned by 90 degrees about the same centre: the overlap is the 2 x 2 square, the union 8 + 12 - 4
    assert abs(iou(box(0, 0), box(0, 0, 6.0, 2.0, math.pi / 2)) - 0.25) < 1e-12
    # the plane is (x, y): a shift along z changes nothing
    hi = box(2, 0)
    hi[2] = 50.0
    assert abs(iou(box(0, 0), hi) - 1.0 / 3.0) < 1e-12
    # 45 degrees: a 2 x 2 square against itself turned -- the regular octagon, area 8 (sqrt 2 - 1)
    oct_area = 8.0 * (math.sqrt(2.0) - 1.0)
    assert abs(iou(box(0, 0, 2, 2), box(0, 0, 2, 2, math.pi / 4)) - oct_area / (8.0 - oct_area)) < 1e-12


def test_bev_iou_against_shapely():
    geom = pytest.importorskip("shapely.geometry")
    EG, det = pkg("evalgeom"), pkg("detfill")
    u = det.uniform((40, 7), 9200, 0.0, 1.0).astype(np.float64)
    b = np.stack([u[:, 0] * 8, u[:, 1] * 8, u[:, 2], 3.5 + u[:, 3], 1.6 + u[:, 4], 1.5 + u[:, 5], 3.14159 * u[:, 6]], 1)
    for i in range(0, 40, 2):
        pa = geom.Polygon(EG.bev_rect(b[i, :2], b[i, 3:5], b[i, 6]))
        pb = geom.Polygon(EG.bev_rect(b[i + 1, :2], b[i + 1, 3:5], b[i + 1, 6]))
        want = pa.intersection(pb).area / pa.union(pb).area
        assert abs(ER().bev_iou(b[i], b[i + 1]) - want) < 1e-9


def test_zero_area_box_neither_suppresses_nor_matches():
    z = box(0, 0, 0.0, 2.0)
    assert math.isnan(ER().bev_iou(z, z))
    assert not ER().bev_iou(z, box(0, 0)) > 0.0 and not ER().bev_iou(box(0, 0), z) > 0.0
    boxes = np.stack([z, z, box(0, 0)])
    assert ER().nms(boxes, 0.1).tolist() == [1, 1, 1]
    refs = np.zeros((2, 9))
    refs[0, :7], refs[0, 8] = z, 1
    refs[1, :7], refs[1, 8] = box(0, 0), 1
    tp = ER().match(boxes, np.ones(3, np.int32), refs, THR)
    assert tp.tolist() == [0, 0, (1 << 10) - 1]


def harness(cls="Test", **cfg):
    Tm = pkg("test")
    T = getattr(Tm, cls).__new__(getattr(Tm, cls))
    torch.nn.Module.__init__(T)
    T.config = dict({"score_threshold": 0.5}, **cfg)
    T.initialize_ap()
    return T


def test_nms_runs_in_score_order_not_raster_order():
    """A low-score box that precedes an overlapping high-score one in raster order: it wins under Test.NMS_SAT, it loses here."""
    pred = np.zeros((1, 32, 2, 3), dtype=np.float32)
    lo, hi = box(10.0, 5.0), box(10.5, 5.0)
    pred[0, 18:25, 0, 0], pred[0, 1, 0, 0] = lo, 0.6                       # raster position 0
    pred[0, 18:25, 1, 1], pred[0, 1, 1, 1] = hi, 0.9                       # raster position 4
    T = harness()
    cls, _, bb = torch.split(torch.from_numpy(pred), [4, 14, 14], dim=1)
    raster = T.get_bboxes(cls, bb)
    compat = T.NMS_SAT(raster)[0]
    assert len(compat) == 1 and np.allclose(compat[0].numpy(), lo)
    boxes, scores, count, total = ER().rank_filter(pred, 0.5, 4096)
    assert count[0] == 2 and scores[0, :2].tolist() == [np.float32(0.9), np.float32(0.6)]
    keep = ER().nms(boxes[0, :2], 0.1)
    assert keep.tolist() == [1, 0] and np.allclose(boxes[0, 0], hi)


def test_matching_is_one_to_one():
    """Five survivors on one label: one true positive at 0.5 here, five under the compat counter."""
    dets = np.stack([box(20.0 + 0.05 * i, 3.0) for i in range(5)])
    keep = ER().nms(dets, 0.99)
    assert keep.tolist() == [1] * 5
    refs = np.zeros((1, 3, 9))
    refs[0, 0, :7], refs[0, 0, 8] = box(20.0, 3.0), 1
    refs[0, 1, :7], refs[0, 1, 8] = box(20.0, 3.0), 0                      # an unlabelled row is never taken
    tp = ER().match(dets, keep, refs[0], THR)
    assert [int(((tp >> 0) & 1).sum()), int(((tp >> 9) & 1).sum())] == [1, 1] and tp[0] == (1 << 10) - 1 and not tp[1:].any()
    T = harness()
    T.precision_recall_singleshot([[torch.from_numpy(d).float() for d in dets]], torch.from_numpy(refs).float())
    assert T.get_num_TP_set()[0.5] == 5 and T.get_num_P() == 5 and T.get_num_T() == 1


def test_matching_takes_the_best_unmatched_row_and_ties_go_to_the_lower_row():
    # rows: A at x = 0, B at x = 1; survivors at x = 0.4, then x = 0.3 (4 x 2 boxes: IoU = (4 - d) / (4 + d) at distance d).
    #   survivor 1: A 0.818, B 0.739      survivor 2: A 0.860, B 0.702
    # t <= 0.7:      1 takes A; 2 prefers A, which is taken, and gets B (0.702 > t): both true positives
    # t = 0.75, 0.8: 1 takes A; 2 is left with B, 0.702: a false positive (with many-to-one matching it would count on A)
    # t = 0.85:      1 fails on A (0.818) and takes nothing, so A is still free for 2 (0.860): a true positive
    # t >= 0.9:      nothing
    refs = np.zeros((3, 9))
    refs[0, :7], refs[0, 8] = box(0.0, 0.0), 1
    refs[1, :7], refs[1, 8] = box(1.0, 0.0), 1
    dets = np.stack([box(0.4, 0.0), box(0.3, 0.0)])
    iou = ER().iou_matrix(dets, np.ones(2, np.int32), refs)
    assert np.allclose(iou[:, :2], [[3.6 / 4.4, 3.4 / 4.6], [3.7 / 4.3, 3.3 / 4.7]], atol=1e-12) and np.isnan(iou[:, 2]).all()
    tp = ER().match(dets, np.ones(2, np.int32), refs, THR)
    assert tp.tolist() == [0b0001111111, 0b0010011111]
    # tie: a detection midway between rows A (x = 0) and B (x = 2), IoU 0.6 with both, takes the LOWER row; the next one, close
    # to A (0.905) and far from B (0.29), is therefore a false positive at 0.5 and 0.55 -- had the first taken B it would count
    refs2 = np.zeros((2, 9))
    refs2[0, :7], refs2[1, :7], refs2[:, 8] = box(0.0, 0.0), box(2.0, 0.0), 1
    dets2 = np.stack([box(1.0, 0.0), box(-0.2, 0.0)])
    iou2 = ER().iou_matrix(dets2, np.ones(2, np.int32), refs2)
    assert iou2[0, 0] == iou2[0, 1] and abs(iou2[0, 0] - 0.6) < 1e-12 and abs(iou2[1, 0] - 3.8 / 4.2) < 1e-12
    assert ER().match(dets2, np.ones(2, np.int32), refs2, THR).tolist() == [0b0000000011, 0b0111111100]
    assert ER().match(dets2, np.ones(2, np.int32), refs2[::-1].copy(), THR).tolist() == [0b0000000011, 0b0111111111]


def ap_restated(scores, tpmask, n_gt, t):
    """KITTI R40 with exact rationals."""
    N = len(scores)
    order = sorted(range(N), key=lambda i: (-float(scores[i]), i))
    c, pts = 0, []
    for k, i in enumerate(order, 1):
        c += int(tpmask[i] >> t) & 1
        pts.append((c, Fraction(c, k)))
    if n_gt == 0:
        return None, c
    total = 0.0
    for j in range(1, 41):
        reach = [p for ck, p in pts if 40 * ck >= j * n_gt]
        total = total + (float(max(reach)) if reach else 0.0)
    return total / 40.0, c


@pytest.mark.parametrize("N,n_gt,seed", [(1, 1, 1), (37, 20, 2), (300, 90, 3), (300, 1000, 4), (64, 7, 5)])
def test_average_precision_equals_rational_restatement(N, n_gt, seed):
    det = pkg("detfill")
    scores = (np.round(det.uniform((N,), 9300 + seed, 0.5, 1.0) * 16.0) / 16.0).astype(np.float32)      # heavily tied
    u = det.uniform((N, 10), 9400 + seed, 0.0, 1.0)
    tpmask = np.zeros(N, dtype=np.uint32)
    for t in range(10):
        tpmask |= ((u[:, t] < 0.8 - 0.06 * t).astype(np.uint32) << np.uint32(t))
    ap, tp = ER().average_precision(scores, tpmask, n_gt, 10)
    for t in range(10):
        want, c = ap_restated(scores, tpmask, n_gt, t)
        assert tp[t] == c
        assert abs(ap[t] - want) <= 1e-15, (t, ap[t], want)          # float(Fraction(c, k)) is the correctly rounded c / k too


def test_average_precision_fixed_cases():
    f = ER().average_precision
    s = np.linspace(0.9, 0.6, 8).astype(np.float32)
    ap, tp = f(s, np.full(8, 1023, np.uint32), 8, 10)
    assert ap.tolist() == [1.0] * 10 and tp.tolist() == [8] * 10
    ap, tp = f(s, np.zeros(8, np.uint32), 8, 10)
    assert ap.tolist() == [0.0] * 10 and tp.tolist() == [0] * 10
    ap, tp = f(s, np.full(8, 1023, np.uint32), 0, 10)
    assert np.isnan(ap).all() and tp.tolist() == [8] * 10
    ap, tp = f(np.zeros(0, np.float32), np.zeros(0, np.uint32), 5, 10)
    assert ap.tolist() == [0.0] * 10 and tp.tolist() == [0] * 10
    out = ER().summarize(np.zeros(0, np.float32), np.zeros(0, np.uint32), 5, THR)
    assert out["precision"][0.5] == 0.0 and out["recall"][0.5] == 0.0 and out["map"] == 0.0 and out["num_P"] == 0
    # one TP ranked first of two, two labels: recall 1/2 -> P_1..P_20 = 1, the rest 0
    ap, _ = f(np.array([0.9, 0.8], np.float32), np.array([1, 0], np.uint32), 2, 1)
    assert ap[0] == 0.5


def scene_pred(seed, n_lab=3):
    """A 4 x 5 map, two samples: jittered copies of the labels with tied scores above the threshold."""
    det = pkg("detfill")
    pred = np.zeros((2, 32, 4, 5), dtype=np.float32)
    refs = np.zeros((2, 4, 9), dtype=np.float32)
    u = det.uniform((2, 2, 20, 8), seed, 0.0, 1.0)
    for b in range(2):
        for g in range(n_lab):
            refs[b, g, :7], refs[b, g, 8] = box(6.0 * g, 3.0 * b), 1
        for a in range(2):
            for px in range(20):
                c = box(6.0 * (px % n_lab) + (u[b, a, px, 0] - 0.5), 3.0 * b + 0.5 * (u[b, a, px, 1] - 0.5), yaw=0.2 * (u[b, a, px, 2] - 0.5))
                pred[b, 18 + 7 * a:25 + 7 * a, px // 5, px % 5] = c
                pred[b, 2 * a + 1, px // 5, px % 5] = np.round(u[b, a, px, 7] * 8.0) / 8.0
    return pred, refs


def test_switch_builds_the_compat_evaluator_by_default():
    import os
    import yaml
    from _util import PKG, ROOT
    Tr, Tm = pkg("train"), pkg("test")
    net = torch.nn.Conv2d(1, 1, 1)
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")))
    assert "eval_metric" not in cfg
    assert type(Tr.make_tester(net, dict(cfg))) is Tm.Test
    assert type(Tr.make_tester(net, dict(cfg, eval_metric="compat"))) is Tm.Test
    assert type(Tr.make_tester(net, dict(cfg, eval_metric="ranked"))) is Tm.RankedTest
    with pytest.raises(ValueError):
        Tr.make_tester(net, dict(cfg, eval_metric="coco"))
    assert issubclass(Tm.RankedTest, Tm.Test)


def test_ranked_summary_on_cpu_tensors_agrees_with_the_pieces():
    T = harness("RankedTest", eval_score_threshold=0.3, eval_nms_iou=0.7)
    sc, tpm, n_gt = [], [], 0
    for step in range(2):
        pred, refs = scene_pred(9500 + step)
        T.accumulate(torch.from_numpy(pred), torch.from_numpy(refs))
        boxes, scores, count, total = ER().rank_filter(pred, 0.3, 4096)
        for b in range(2):
            n = int(count[b])
            keep = ER().nms(boxes[b, :n], 0.7)
            tp = ER().match(boxes[b, :n], keep, refs[b], T.IOU_threshold)
            sc += scores[b, :n][keep != 0].tolist()
            tpm += tp[keep != 0].tolist()
            n_gt += 3
        d = T.detections()
        assert len(d) == 2 and d[1][0].shape[0] == int(keep.sum()) and d[1][1].tolist() == scores[1, :n][keep != 0].tolist()
    want = ER().summarize(np.array(sc, np.float32), np.array(tpm, np.uint32), n_gt, T.IOU_threshold)
    got = T.summary()
    assert got["num_P"] == len(sc) > 12 and got["num_T"] == 12 and got["truncated_candidates"] == 0
    assert got["tp"] == want["tp"] and 0 < got["tp"][0.5] <= 12
    for t in T.IOU_threshold:
        assert got["ap"][t] == want["ap"][t] and got["precision"][t] == want["precision"][t] and got["recall"][t] == want["recall"][t]
    assert got["map"] == want["map"] and 0.0 < got["map"] <= 1.0
    assert (T.get_num_P(), T.get_num_T(), T.get_num_TP_set()) == (got["num_P"], 12, got["tp"])
    T.initialize_ap()
    assert T.summary()["num_P"] == 0 and T.summary()["num_T"] == 0
    # eval_max_candidates below the number kept: the highest-ranked stay, the sample is reported
    T2 = harness("RankedTest", eval_score_threshold=0.3, eval_max_candidates=4)
    pred, refs = scene_pred(9500)
    T2.accumulate(torch.from_numpy(pred), torch.from_numpy(refs))
    assert T2.summary()["truncated_candidates"] == 2 and T2.summary()["num_P"] <= 8


def test_accumulator_overflow_raises():
    T = harness("RankedTest", eval_score_threshold=0.3, eval_nms_iou=0.99, eval_max_detections=16)
    pred, refs = scene_pred(9500)
    T.accumulate(torch.from_numpy(pred), torch.from_numpy(refs))
    with pytest.raises(RuntimeError, match="eval_max_detections"):
        T.summary()

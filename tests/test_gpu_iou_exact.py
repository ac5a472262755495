"""GPU suite: the device's rotated-box IoU (ev_clip of csrc/ev_geom.h, through csrc/evalpost.hip and csrc/loss.hip) against the EXACT
rational clip of tests/_iou_exact.py -- not against the host statement, which is the same algorithm -- on the families of pairs whose
edges share a line up to rounding: the two IoU matrices of the KITTI-style protocol, the ranked path's suppression and matching, and the
anchor assignment.

The exact values start from the host's fp64 corners (evalgeom.bev_rect / box_corners).  The device's cos / sin may differ from libm in
the last bit, which moves a corner by about 1e-14; the bound of tests/test_iou_exact_host.py, 1e-9, covers that as it covers the
clip's own rounding (about 1e-12 at these magnitudes).  Decisions compare exactly: before any device call each test asserts, from the
reference alone, that every exact IoU that enters a decision is at least 1e-6 from the threshold it is compared with -- a condition on
the inputs -- and that every family is present.  Each test prints the worst difference it met (recorded in DESIGN.md section 13)."""
import numpy as np
import pytest
import torch

import _iou_exact as X
from _util import pkg

pytestmark = pytest.mark.gpu

BOUND = 1e-9
MARGIN = 1e-6
THR = [0.45, 0.7]               # the matching's IoU thresholds, and the two suppression thresholds.  Not 0.5: the second explicit pair
                                # (a box against its half) has the exact IoU 0.5; 0.25, 0.3, 0.6, 0.9 and (1 - f) / (1 + f) are taken too
POS_IOU, NEG_IOU = 0.7, 0.45    # the assignment's (its default pos_iou, 0.6, is the IoU of a box scaled by 0.6)
HELPER = 0.8                    # anchor 1 of a cell: the label scaled by this in length and width, IoU 0.64
_CASE = {}


def case():
    """The spaced pairs, and per sample the interleaved rows (first, second, first, ...) with their exact matrices, computed once."""
    if not _CASE:
        first, second, family, samples = X.spaced_case()
        _CASE.update(first=first, second=second, family=family, samples=[])
        for idx in samples:
            rows = np.empty((2 * len(idx), 7), np.float32)
            rows[0::2], rows[1::2] = first[idx], second[idx]
            bev, i3d = X.exact_matrices(rows, rows)
            _CASE["samples"].append(dict(idx=idx, rows=rows, bev=bev, i3d=i3d))
    return _CASE


def conditions(c):
    """No family dropped, the two batch shapes present, the pairs of a sample isolated, the explicit pairs what they claim."""
    fams = np.concatenate([c["family"][s["idx"]] for s in c["samples"]])
    assert (np.bincount(fams + 1, minlength=13) == [2] + [64] * 12).all()
    assert len(c["samples"][0]["idx"]) == 13 and sorted(c["family"][c["samples"][0]["idx"]].tolist()) == list(range(-1, 12))
    assert any(len(s["rows"]) == 300 for s in c["samples"])
    for s in c["samples"]:
        n = len(s["rows"])
        other = np.ones((n, n), bool)
        for i in range(0, n, 2):
            other[i:i + 2, i:i + 2] = False
        assert not s["bev"][other].any() and np.isfinite(s["bev"]).all() and np.isfinite(s["i3d"]).all()
        for p, fam in zip(s["idx"], c["family"][s["idx"]]):
            if fam == -1:
                i = 2 * int(np.flatnonzero(s["idx"] == p)[0])
                assert abs(s["bev"][i, i + 1] - X.EXPLICIT[p - 12 * 64][2]) <= 1e-7


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def int1(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def label_rows(boxes, total):
    """[total, 9] label rows: `boxes` valid (last column 1), then copies of them that are not (0, 2, 0, ...)."""
    refs = np.zeros((total, 9), np.float32)
    refs[:len(boxes), :7], refs[:len(boxes), 8] = boxes, 1.0
    for r in range(len(boxes), total):
        refs[r, :7], refs[r, 8] = boxes[(r - len(boxes)) % len(boxes)], 2.0 * ((r - len(boxes)) % 2)
    return refs


# ------------------------------------------------------------------ the two IoU matrices
def test_iou_levels_equal_exact():
    """Every row against every row as a label (a box with itself included), a zero-area row against a zero-area label (the NaN pair),
    at least 70 label rows of which the last ones are not valid, rows past the count."""
    c, ops = case(), pkg("ops")
    conditions(c)
    worst = 0.0
    for s in c["samples"]:
        n = len(s["rows"])
        zero = np.array([[400.0, 400.0, -1.0, 0.0, 0.0, 1.5, 0.3]], np.float32)
        rows = np.concatenate([s["rows"], zero])
        want_bev, want_3d = np.zeros((n + 1, n + 1)), np.zeros((n + 1, n + 1))
        want_bev[:n, :n], want_3d[:n, :n] = s["bev"], s["i3d"]
        want_bev[n, n], want_3d[n, n] = X.exact_matrices(zero, zero)[0][0, 0], X.exact_matrices(zero, zero)[1][0, 0]
        assert np.isnan(want_bev[n, n]) and np.isnan(want_3d[n, n]) and np.isnan(want_bev).sum() == 1
        R = max(n + 6, 70)
        refs = label_rows(rows, R)
        pad = 5
        boxes = dev(np.concatenate([rows, rows[:pad]]))
        keep = torch.ones(n + 1 + pad, dtype=torch.int32, device="cuda")
        keep[3] = 0                                                     # not a survivor: NaN along its row
        bev, i3d = ops.eval_iou_levels(boxes, keep, int1(n + 1), dev(refs))
        for got, want in ((bev, want_bev), (i3d, want_3d)):
            got = got.cpu().numpy()[:n + 1]
            assert np.isnan(got[:, n + 1:]).all() and np.isnan(got[3]).all()
            got, want = np.delete(got[:, :n + 1], 3, 0), np.delete(want, 3, 0)
            assert np.array_equal(np.isfinite(got), np.isfinite(want)), "finite exactly where the exact value is"
            err = float(np.nanmax(np.abs(got - want)))
            worst = max(worst, err)
            assert err <= BOUND, err
    print("eval_iou_levels: worst |device - exact| %.3g" % worst)


# ------------------------------------------------------------------ the ranked path
def test_match_ranked_equals_flags_of_exact_iou():
    """The first boxes are the survivors, the second boxes the labelled rows (at least 70 rows, the last ones not valid)."""
    c, ops, ER = case(), pkg("ops"), pkg("evalrank")
    conditions(c)
    hits = np.zeros(len(THR), np.int64)
    for s in c["samples"]:
        n, m = len(s["rows"]), len(s["idx"])
        R = max(m + 6, 70)
        refs = label_rows(s["rows"][1::2], R)
        keep = np.zeros(n, np.int32)
        keep[0::2] = 1
        exact = np.full((n, R), np.nan)
        exact[0::2, :m] = s["bev"][0::2, 1::2]
        assert X.away_from(exact, THR, MARGIN) and ((exact > 0).sum(1) <= 1).all()       # one candidate row per survivor: no choice to make
        want = ER.match(s["rows"], keep, refs, THR, iou=exact)
        assert want[1::2].sum() == 0 and [int(want[2 * k]) for k in range(m)] == [sum(1 << t for t, thr in enumerate(THR) if s["bev"][2 * k, 2 * k + 1] > thr) for k in range(m)]
        pad = 3
        got = ops.eval_match_ranked(dev(np.concatenate([s["rows"], s["rows"][:pad]])), dev(np.concatenate([keep, np.ones(pad, np.int32)])), int1(n), dev(refs),
                                    torch.tensor(THR, dtype=torch.float64, device="cuda"))
        got = got.cpu().numpy().view(np.uint32)
        assert got[:n].tolist() == want.tolist() and not got[n:].any()
        hits += [int(((want >> np.uint32(t)) & 1).sum()) for t in range(len(THR))]
    print("true positives per threshold", hits.tolist())
    assert (hits > 64).all() and hits[0] > hits[1]                      # both outcomes at both thresholds


def greedy(iou, thr):
    """Keep flags of the suppression in row order on a matrix iou[candidate, earlier row]."""
    keep, kept = np.zeros(len(iou), np.int32), []
    for i in range(len(iou)):
        if not any(iou[i, j] > thr for j in kept):
            keep[i] = 1
            kept.append(i)
    return keep


def nudged_3d(rows):
    """Exact 3-D IoU [i, j < i] of the suppression's IoU flavour (test.NMS_IOU): candidate i against row j with its centre moved by 1e-4,
    on evalgeom.box_corners of the rows laid into the (x, z) footprint plane."""
    EG = pkg("evalgeom")
    r64 = X.footprint_rows(rows).astype(np.float64)
    plain = [EG.box_corners(b[:3], b[3:6], b[6]) for b in r64]
    nudged = [EG.box_corners(b[:3] + 0.0001, b[3:6], b[6]) for b in r64]
    out = np.zeros((len(rows), len(rows)))
    for i in range(len(rows)):
        for j in range(i):
            if not X.apart(rows[i], rows[j]):
                out[i, j] = X.exact_rotated(plain[i], nudged[j])[0]
    return out


@pytest.mark.parametrize("mode", ["bev", "iou"])
def test_nms_equals_flags_of_exact_iou(mode):
    """Rows first, second, first, ...: a second box goes iff its exact IoU with its first box exceeds the threshold."""
    c, ops = case(), pkg("ops")
    conditions(c)
    gone = {t: 0 for t in THR}
    for s in c["samples"]:
        n = len(s["rows"])
        exact = np.tril(s["bev"], -1) if mode == "bev" else nudged_3d(s["rows"])
        assert X.away_from(exact, THR, MARGIN)
        pad = 3
        rows = s["rows"] if mode == "bev" else X.footprint_rows(s["rows"])
        boxes = dev(np.concatenate([rows, rows[:pad]]))
        for thr in THR:
            want = greedy(exact, thr)
            assert want[0::2].all()
            keep, nkeep = ops.eval_nms(boxes, mode, thr, count=int1(n))
            assert keep.cpu().numpy()[:n].tolist() == want.tolist() and not keep.cpu().numpy()[n:].any() and int(nkeep) == int(want.sum())
            gone[thr] += n - int(want.sum())
    print("suppressed per threshold", gone)
    assert gone[THR[0]] > gone[THR[1]] > 64 and gone[THR[0]] < 64 * 12   # duplicates go, neighbours stay


# ------------------------------------------------------------------ the anchor assignment
def test_anchor_assignment_equals_targets_of_exact_iou():
    """Anchor 0 of cell i lies on the first box of pair i, anchor 1 on its second box scaled by 0.8 (IoU 0.64 with the label: the anchor a
    label is forced to where its first box merely touches it); the labels are the second boxes, up to 50 per sample of the batch; cells
    beyond the pairs hold anchors far away."""
    c, ops, A = case(), pkg("ops"), pkg("assign")
    conditions(c)
    worst, kinds = 0.0, np.zeros(4, np.int64)
    for s in c["samples"]:
        m = len(s["idx"])
        W = min(m, 16)
        Hh = -(-m // W)
        HW = Hh * W
        cells = np.zeros((2, HW, 7), np.float32)
        cells[:, :, :] = np.array([900.0, 900.0, -1.0, 1.0, 1.0, 1.5, 0.0], np.float32)
        cells[:, :, 0] += 20.0 * np.arange(2 * HW, dtype=np.float32).reshape(2, HW)
        cells[0, :m], cells[1, :m] = s["rows"][0::2], s["rows"][1::2]
        cells[1, :m, 3:5] = (cells[1, :m, 3:5].astype(np.float64) * HELPER).astype(np.float32)
        anchors = np.ascontiguousarray(cells.transpose(0, 2, 1))          # [2, 7, HW]
        per = 50
        B = -(-m // per)
        boxes = np.zeros((B, 64, 9), np.float32)
        boxes[:, :, :7] = s["rows"][1]                                  # rows past nbox are not labels: a copy of one must change nothing
        nbox = np.zeros(B, np.int32)
        want = []
        for b in range(B):
            labels = s["rows"][1::2][b * per:(b + 1) * per]
            nbox[b] = len(labels)
            boxes[b, :len(labels), :7] = labels
            exact = X.exact_matrices(cells.reshape(2 * HW, 7), labels)[0]
            top2 = np.sort(exact, 0)[-2:]                                # per label: the runner-up and the best anchor
            row2 = np.sort(exact, 1)[:, -2:] if len(labels) > 1 else np.concatenate([np.zeros((2 * HW, 1)), exact], 1)
            assert X.away_from(exact, [POS_IOU, NEG_IOU], MARGIN)
            assert (top2[1] >= MARGIN).all() and (top2[1] - top2[0] >= MARGIN).all(), "forcing: a clear best anchor per label"
            assert ((row2[:, 1] - row2[:, 0] >= MARGIN) | (row2[:, 1] < POS_IOU)).all(), "a clear best label per anchor that takes it by its IoU"
            assert not A.void_labels(labels).any()
            want.append(A.targets_from_iou(exact, np.zeros(len(labels), bool), POS_IOU, NEG_IOU))
        ws, target, counts, best = ops.assign_anchors_workspace(B, Hh, W, 64, torch.device("cuda"), best=True)
        target.fill_(-77); counts.fill_(-77); best.fill_(-77.0)
        ops.assign_anchors_iou(dev(anchors), dev(boxes), dev(nbox), Hh, W, POS_IOU, NEG_IOU, target, counts, ws, best=best)
        for b in range(B):
            t, bst, cnt, forced = want[b]
            err = float(np.abs(best[b].reshape(-1).cpu().numpy() - bst).max())
            worst = max(worst, err)
            assert err <= BOUND, err
            assert np.array_equal(target[b].reshape(-1).cpu().numpy(), t) and np.array_equal(counts[b].cpu().numpy(), cnt), (b, counts[b].tolist(), cnt.tolist())
            kinds += (int((t[:HW] >= 0).sum()), int((t[HW:] >= 0).sum()), int((t == -2).sum()), int((t == -1).sum()))
    print("assign_anchors_iou: worst |best - exact| %.3g; positives on the first boxes %d, on the scaled labels %d, ignored %d, negative %d" % ((worst,) + tuple(kinds)))
    assert (kinds > 64).all()

"""Host statement of the IoU-based anchor assignment (`loss_sampling: anchor`) -- what the device entry
dcf_assign_anchors_iou (csrc/loss.hip, k_assign_*) is compared with in tests/test_gpu_loss_anchor.py.  numpy, float64 geometry on the
float32 inputs; the IoU is evalrank.bev_iou, the statement the evaluation's clip is pinned to.

Anchor index j = a * HW + i for anchor a in {0, 1} and cell i of anchors [2, 7, HW]; labels are rows (x, y, z, l, w, h, yaw, ...).
  I(j, k)    = evalrank.bev_iou(anchor j, label k): the anchor's rectangle clipped by the label's.  A VOID label (a non-finite x, y, l, w
               or yaw, or l <= 0 or w <= 0) has I = 0 everywhere.
  best(j)    = max_k I(j, k), arg(j) = the lowest k attaining it (0 and -1 without labels)
  forced(k)  = the j of highest I(j, k), ties to the lowest j, provided that value is > 0; else none
  target(j)  = the lowest k with forced(k) == j; else arg(j) if best(j) >= pos_iou; else -1 (negative) if best(j) < neg_iou; else -2
               (ignored)
  counts     = (anchors with target >= 0, ignored anchors, anchors positive through forcing only, void labels)
"""
import numpy as np

from . import evalrank

PRUNE = 1.002       # on the squared centre distance: 0.1 % of slack on the distance (csrc/loss.hip, AS_PRUNE)


def parse_assign_config(config):
    """(assign_pos_iou, assign_neg_iou), validated: finite numbers with 0 < neg <= pos <= 1.  The defaults (0.6, 0.45) are the car
    values of SECOND / PointPillars; this model has not been trained with them."""
    pos, neg = config.get("assign_pos_iou", 0.6), config.get("assign_neg_iou", 0.45)
    for key, v in (("assign_pos_iou", pos), ("assign_neg_iou", neg)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError("%s must be a finite number (got %r)" % (key, v))
    if not 0.0 < neg <= pos <= 1.0:
        raise ValueError("0 < assign_neg_iou <= assign_pos_iou <= 1 must hold (got %r, %r)" % (neg, pos))
    return float(pos), float(neg)


def _f32_rows(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def void_labels(boxes):
    """bool [n]: the label rows that take no part (a non-finite x, y, l, w or yaw, or l <= 0 or w <= 0)."""
    bx = _f32_rows(boxes)
    if bx.size == 0:
        return np.zeros(0, dtype=bool)
    used = bx[:, [0, 1, 3, 4, 6]]
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(used).all(1) & (bx[:, 3] > 0) & (bx[:, 4] > 0))


def anchor_iou(anchors, boxes, prune=True):
    """I [2 * HW, n] float64.  prune: a pair whose centres are further apart than the two half-diagonals together (times the slack)
    skips the clip -- the rectangles are disjoint, and the clip's own value there is exactly 0, so both settings agree bit for bit."""
    anc = _f32_rows(anchors)
    HW = anc.shape[2]
    rows = anc.transpose(0, 2, 1).reshape(2 * HW, 7)                   # row j = a * HW + i
    n = len(boxes)
    out = np.zeros((2 * HW, n), dtype=np.float64)
    if n == 0:
        return out
    bx = _f32_rows(boxes)[:, :7]
    void = void_labels(bx)
    a_half = 0.5 * np.sqrt(rows[:, 3] ** 2 + rows[:, 4] ** 2)
    for k in range(n):
        if void[k]:
            continue
        if prune:
            d2 = (rows[:, 0] - bx[k, 0]) ** 2 + (rows[:, 1] - bx[k, 1]) ** 2
            s = a_half + 0.5 * np.sqrt(bx[k, 3] ** 2 + bx[k, 4] ** 2)
            near = np.flatnonzero(~(d2 > s * s * PRUNE))
        else:
            near = range(2 * HW)
        for j in near:
            out[j, k] = evalrank.bev_iou(rows[j], bx[k])
    return out


def targets_from_iou(I, void, pos_iou, neg_iou):
    """Rules 2-5 on an IoU matrix [J, n] (void columns zero): (target int32 [J], best float64 [J], counts int32 [4], forced int64 [n])."""
    J, n = I.shape
    if n:
        best, arg = I.max(1), I.argmax(1)                              # argmax: the first, i.e. lowest, k of equal values
        top = I.argmax(0)                                              # ... and the lowest j
        forced = np.where(I[top, np.arange(n)] > 0, top, -1).astype(np.int64)
    else:
        best, arg, forced = np.zeros(J), np.full(J, -1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    target = np.where(best >= pos_iou, arg, np.where(best < neg_iou, -1, -2)).astype(np.int32)
    only = np.zeros(J, dtype=bool)
    for k in range(n - 1, -1, -1):                                     # descending: the lowest k that forces j is written last
        if forced[k] >= 0:
            target[forced[k]] = k
            only[forced[k]] = not best[forced[k]] >= pos_iou
    counts = np.array([(target >= 0).sum(), (target == -2).sum(), only.sum(), int(np.sum(void))], dtype=np.int32)
    return target, best, counts, forced


def anchor_targets(anchors, boxes, pos_iou, neg_iou, prune=True):
    """(target int32 [2 * HW], best float64 [2 * HW], counts int32 [4]) of one sample: anchors [2, 7, HW], boxes [n, >= 7] = the sample's
    label rows k < nbox."""
    I = anchor_iou(anchors, boxes, prune=prune)
    return targets_from_iou(I, void_labels(boxes), pos_iou, neg_iou)[:3]

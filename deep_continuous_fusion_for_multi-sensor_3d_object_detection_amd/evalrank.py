"""Host statement (numpy) of the ranked evaluation (`eval_metric: ranked`): score-ordered suppression,
one-to-one matching against the labels and KITTI R40 average precision.

Everything is decided on integer keys and fp64 geometry, so the device kernels of csrc/evalpost.hip (k_rank_* / k_ap_*) agree
with these functions on every integer output; RankedTest (test.py) runs them on CPU tensors, and the GPU tests check the device
against them.
  * candidate        = (sample b, anchor a, pixel px); score pred[b, 2a+1, px] (fp32), box pred[b, 18+7a .. 18+7a+6, px]; kept iff
                       score > threshold (a NaN score is never kept); index = a*h*w + px
  * rank in a sample = score descending, ties to the lower index: key (orderable_u32(score) << 32) | (0xFFFFFFFF - index),
                       larger first; keys are unique
  * bev_iou          = IoU of the two evalgeom.bev_rect rectangles in (x, y), clipped with evalgeom._clip_convex; no 1e-4 nudge;
                       NaN for a zero-area pair, which compares false everywhere
  * nms              = greedy in rank order: a box survives iff its bev_iou with every earlier survivor is not > the threshold
  * match            = per IoU threshold t, survivors in rank order each take the labelled row of highest bev_iou among the rows
                       not yet taken at t (ties: lower row); a pair iff that IoU > t, and only then is the row taken
  * average_precision= detections by (score descending, accumulation index ascending); P_j = max{c_k / k : 40 c_k >= j n_gt},
                       AP = (P_1 + ... + P_40) / 40
"""
import numpy as np

from . import evalgeom as EG

LEVELS = 40


def orderable_u32(scores):
    """Total-order map of fp32 bits to uint32: larger float <=> larger unsigned (-0.0 below +0.0)."""
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(bits >> np.uint32(31) != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def rank_keys(scores, index):
    """uint64 keys, larger first: (orderable_u32(score) << 32) | (0xFFFFFFFF - index)."""
    return (orderable_u32(scores).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(index, dtype=np.uint64))


def rank_filter(pred, threshold, cap):
    """pred [B,32,h,w] fp32 -> (boxes [B,cap,7] fp32, scores [B,cap] fp32, count [B], total [B]): per sample the candidates with
    score > threshold in rank order; total = how many passed, count = min(total, cap); rows >= count stay zero."""
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    B, C, h, w = pred.shape
    hw = h * w
    p = pred.reshape(B, C, hw)
    boxes = np.zeros((B, cap, 7), dtype=np.float32)
    scores = np.zeros((B, cap), dtype=np.float32)
    count = np.zeros((B,), dtype=np.int32)
    total = np.zeros((B,), dtype=np.int32)
    thr = np.float32(threshold)
    for b in range(B):
        s = np.concatenate([p[b, 1], p[b, 3]])                          # candidate index a*hw + px
        with np.errstate(invalid="ignore"):
            idx = np.nonzero(s > thr)[0]
        keys = rank_keys(s[idx], idx)
        idx = idx[np.argsort(keys)[::-1]]
        total[b] = len(idx)
        idx = idx[:cap]
        count[b] = len(idx)
        a, px = idx // hw, idx % hw
        for k in range(7):
            boxes[b, :len(idx), k] = p[b, 18 + 7 * a + k, px]
        scores[b, :len(idx)] = s[idx]
    return boxes, scores, count, total


def bev_iou(c1, c2):
    """Bird's-eye IoU of boxes c1, c2 (x, y, z, l, w, h, yaw): c1's rectangle clipped by c2's."""
    r1 = np.array(EG.bev_rect(c1[:2], c1[3:5], c1[6]), dtype=np.float64)
    r2 = np.array(EG.bev_rect(c2[:2], c2[3:5], c2[6]), dtype=np.float64)
    inter = EG._clip_convex(r1, r2)
    ia = EG._shoelace(np.array(inter, dtype=np.float64)) if len(inter) >= 3 else 0.0
    a1, a2 = EG._shoelace(r1), EG._shoelace(r2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(ia) / np.float64(a1 + a2 - ia))


def nms(boxes, iou_threshold):
    """Greedy suppression in row (= rank) order: keep flags int32 [n]."""
    boxes = np.asarray(boxes, dtype=np.float64)
    keep = np.zeros((len(boxes),), dtype=np.int32)
    kept = []
    for i, c in enumerate(boxes):
        if not any(bev_iou(c, k) > iou_threshold for k in kept):
            keep[i] = 1
            kept.append(c)
    return keep


def iou_matrix(boxes, keep, refs):
    """[n, R] fp64: bev_iou of every survivor with every labelled row (ref[:, 8] == 1); NaN elsewhere."""
    boxes = np.asarray(boxes, dtype=np.float64)
    refs = np.asarray(refs, dtype=np.float64).reshape(-1, 9)
    out = np.full((len(boxes), len(refs)), np.nan, dtype=np.float64)
    for i in np.nonzero(keep)[0]:
        for r in range(len(refs)):
            if refs[r, 8] == 1:
                out[i, r] = bev_iou(boxes[i], refs[r])
    return out


def match(boxes, keep, refs, thresholds, iou=None):
    """tpmask uint32 [n]: bit t set iff survivor i is a true positive at thresholds[t] (one-to-one, best unmatched row)."""
    iou = iou_matrix(boxes, keep, refs) if iou is None else iou
    n, R = iou.shape
    tpmask = np.zeros((n,), dtype=np.uint32)
    for t, thr in enumerate(thresholds):
        taken = np.zeros((R,), dtype=bool)
        for i in np.nonzero(keep)[0]:
            best, best_r = -np.inf, -1
            for r in range(R):
                if not taken[r] and iou[i, r] > best:                   # NaN never wins; ascending r keeps the lower row on a tie
                    best, best_r = iou[i, r], r
            if best_r >= 0 and best > thr:
                taken[best_r] = True
                tpmask[i] |= np.uint32(1 << t)
    return tpmask


def average_precision(scores, tpmask, n_gt, nthr):
    """(ap [nthr] fp64, tp [nthr] int64) of the accumulated detections (KITTI R40)."""
    scores = np.asarray(scores, dtype=np.float32)
    tpmask = np.asarray(tpmask, dtype=np.uint32)
    N = len(scores)
    order = np.argsort(rank_keys(scores, np.arange(N)))[::-1]
    tps = tpmask[order]
    ap = np.full((nthr,), np.nan, dtype=np.float64)
    tp = np.zeros((nthr,), dtype=np.int64)
    k = np.arange(1, N + 1, dtype=np.float64)
    for t in range(nthr):
        c = np.cumsum((tps >> np.uint32(t)) & np.uint32(1), dtype=np.int64)
        tp[t] = c[-1] if N else 0
        if n_gt <= 0:
            continue
        M = np.zeros((LEVELS + 1,), dtype=np.float64)
        if N:
            np.maximum.at(M, np.minimum(LEVELS, 40 * c // int(n_gt)), c.astype(np.float64) / k)
        total = np.float64(0.0)
        for j in range(1, LEVELS + 1):
            total = total + M[j:].max()
        ap[t] = total / np.float64(40.0)
    return ap, tp


def summarize(scores, tpmask, n_gt, thresholds, truncated=0):
    """The dictionary RankedTest.summary() returns, from the accumulated (score, tpmask) and the label count."""
    nthr = len(thresholds)
    ap, tp = average_precision(scores, tpmask, n_gt, nthr)
    return assemble(ap, tp, len(scores), int(n_gt), thresholds, truncated)


def assemble(ap, tp, N, n_gt, thresholds, truncated=0):
    nan = float("nan")
    m = 0.0
    for v in ap:
        m = m + float(v)
    return {"ap": {t: float(v) for t, v in zip(thresholds, ap)},
            "map": m / len(thresholds),
            "tp": {t: int(v) for t, v in zip(thresholds, tp)},
            "precision": {t: (int(v) / N if N else 0.0) for t, v in zip(thresholds, tp)},
            "recall": {t: (int(v) / n_gt if n_gt else nan) for t, v in zip(thresholds, tp)},
            "num_P": int(N), "num_T": int(n_gt), "truncated_candidates": int(truncated)}

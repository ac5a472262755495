"""Host statement (numpy) of the KITTI-style protocol on top of the ranked evaluation (`eval_protocol: kitti`).

KITTI-STYLE, not the official tool: the official tool matches in label order and re-matches at 41 score thresholds; this keeps
section 13's rank-order one-to-one matching (evalrank.py) and adds the third outcome -- ignored -- in COCO's manner.  The device
kernels of csrc/evalpost.hip (k_kitti_*) agree with these functions on every integer output; RankedTest (test.py) runs them on CPU
tensors, and the GPU tests check the device against them.
  * level of a row   = lowest d in (easy 0, moderate 1, hard 2) with h2d >= min_height[d], occlusion <= max_occlusion[d] and
                       truncation <= max_truncation[d]; 3 (never counted) when none qualifies and for a Van; rows without the
                       information are level 0.  At difficulty d a valid row (ref[:, 8] == 1) is COUNTED iff level <= d, else IGNORED
  * iou_pair         = (bird's-eye IoU, 3-D IoU) from one clip: ia, a1, a2 exactly evalrank.bev_iou's; zov = the overlap of the two
                       z extents [z - h/2, z + h/2]; iv = ia * zov; iou3d = iv / (a1 h1 + a2 h2 - iv), all fp64
  * det_flags        = the eight corners (evalgeom.bev_rect at z - h/2 and z + h/2) through the frame's [4,3] matrix C in fp64
                       (d = ((x C02 + y C12) + z C22) + C32, likewise u d and v d); corners with d > 0 only, u clamped to [0, W],
                       v to [0, H]; bit d: height < min_height[d]; bit 3: more than dontcare_overlap of the 2-D box's own area lies
                       in one DontCare rectangle
  * match_levels     = per metric m (bev, 3d), difficulty d and threshold t independently, survivors in rank order: (A) the counted
                       row of highest IoU among those not yet taken, a true positive iff that IoU > t (evalrank.match on the counted
                       rows); else (B) ignored iff an ignored row has IoU > t (ignored rows are never taken); else (C) ignored iff
                       flag bit d or 3 is set; else (D) a false positive.  Bit 10 d + t of tpmask[m] / igmask[m]
  * average_precision_levels = evalrank.average_precision per (m, d, t) over the detections not ignored there, with n_gt[d]
"""
import numpy as np

from . import evalgeom as EG
from . import evalrank as ER

LEVEL_NAMES = ("easy", "moderate", "hard")
METRICS = ("bev", "3d")
NEVER = 3                              # level of a row no difficulty counts
BITS = 10                              # bits per difficulty in a mask word: bit 10 d + t
DONTCARE_BIT = 3

DEFAULTS = {"eval_min_height": (40.0, 25.0, 25.0), "eval_max_occlusion": (0, 1, 2), "eval_max_truncation": (0.15, 0.30, 0.50),
            "eval_dontcare_overlap": 0.5, "eval_max_dontcare": 64, "eval_report_iou": 0.7}


def settings(config, thresholds=None):
    """The protocol's settings out of a config, validated (ValueError): three-entry lists, heights >= 0, overlap in (0, 1],
    eval_report_iou one of `thresholds`."""
    out = {}
    for key in ("eval_min_height", "eval_max_occlusion", "eval_max_truncation"):
        v = config.get(key)
        v = DEFAULTS[key] if v is None else v
        if not isinstance(v, (list, tuple)) or len(v) != 3:
            raise ValueError("%s must be a list of three values, easy / moderate / hard (got %r)" % (key, v))
        out[key[5:]] = tuple(int(x) for x in v) if key == "eval_max_occlusion" else tuple(float(x) for x in v)
    if any(not h >= 0 for h in out["min_height"]):
        raise ValueError("eval_min_height must not be negative (got %r)" % (out["min_height"],))
    ov = config.get("eval_dontcare_overlap")
    ov = float(DEFAULTS["eval_dontcare_overlap"] if ov is None else ov)
    if not 0.0 < ov <= 1.0:
        raise ValueError("eval_dontcare_overlap must be in (0, 1] (got %r)" % (ov,))
    out["dontcare_overlap"] = ov
    md = config.get("eval_max_dontcare")
    md = int(DEFAULTS["eval_max_dontcare"] if md is None else md)
    if md < 0:
        raise ValueError("eval_max_dontcare must not be negative (got %r)" % (md,))
    out["max_dontcare"] = md
    rep = config.get("eval_report_iou")
    rep = float(DEFAULTS["eval_report_iou"] if rep is None else rep)
    if thresholds is not None and rep not in [float(t) for t in thresholds]:
        raise ValueError("eval_report_iou must be one of %r (got %r)" % (list(thresholds), rep))
    out["report_iou"] = rep
    return out


def protocol(config):
    """'plain' or 'kitti' (ValueError otherwise; kitti needs eval_metric: ranked)."""
    p = config.get("eval_protocol") or "plain"
    if p not in ("plain", "kitti"):
        raise ValueError("eval_protocol must be plain or kitti (got %r)" % (p,))
    if p == "kitti" and (config.get("eval_metric") or "compat") != "ranked":
        raise ValueError("eval_protocol: kitti needs eval_metric: ranked (got %r)" % (config.get("eval_metric") or "compat",))
    return p


def difficulty_level(obj_type, h2d, occlusion, truncation, s=None):
    """Level of one KITTI label line: the lowest d all three closed bounds admit, else 3; a Van is always 3."""
    s = settings({}) if s is None else s
    if obj_type != "Car":
        return NEVER
    for d in range(3):
        if h2d >= s["min_height"][d] and int(occlusion) <= s["max_occlusion"][d] and truncation <= s["max_truncation"][d]:
            return d
    return NEVER


# ------------------------------------------------------------------ geometry
def iou_pair(c1, c2):
    """(bird's-eye IoU, 3-D IoU) of boxes c1, c2 (x, y, z, l, w, h, yaw; z at mid-height): c1's rectangle clipped by c2's, once."""
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    r1 = np.array(EG.bev_rect(c1[:2], c1[3:5], c1[6]), dtype=np.float64)
    r2 = np.array(EG.bev_rect(c2[:2], c2[3:5], c2[6]), dtype=np.float64)
    inter = EG._clip_convex(r1, r2)
    ia = EG._shoelace(np.array(inter, dtype=np.float64)) if len(inter) >= 3 else 0.0
    a1, a2 = EG._shoelace(r1), EG._shoelace(r2)
    z1, h1, z2, h2 = c1[2], c1[5], c2[2], c2[5]
    with np.errstate(invalid="ignore", divide="ignore"):
        bev = np.float64(ia) / np.float64(a1 + a2 - ia)
        zov = np.fmax(np.float64(0.0), np.fmin(z1 + h1 / 2, z2 + h2 / 2) - np.fmax(z1 - h1 / 2, z2 - h2 / 2))
        iv = np.float64(ia) * zov
        i3d = iv / (np.float64(a1) * h1 + np.float64(a2) * h2 - iv)
    return float(bev), float(i3d)


def iou_matrices(boxes, keep, refs):
    """(bev [n, R], 3d [n, R]) fp64: iou_pair of every survivor with every valid row (ref[:, 8] == 1); NaN elsewhere."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    refs = np.asarray(refs, dtype=np.float64).reshape(-1, 9)
    bev = np.full((len(boxes), len(refs)), np.nan, dtype=np.float64)
    i3d = np.full((len(boxes), len(refs)), np.nan, dtype=np.float64)
    for i in np.nonzero(keep)[0]:
        for r in range(len(refs)):
            if refs[r, 8] == 1:
                bev[i, r], i3d[i, r] = iou_pair(boxes[i], refs[r, :7])
    return bev, i3d


def project_box(box, C, H, W):
    """(umin, vmin, umax, vmax, height, area) of the image box of `box` under the [4,3] matrix C (fp32 entries, fp64 arithmetic);
    height = area = 0 with no corner in front of the camera."""
    box = np.asarray(box, dtype=np.float64)
    C = np.asarray(C, dtype=np.float32).reshape(4, 3).astype(np.float64)
    rect = EG.bev_rect(box[:2], box[3:5], box[6])
    umin = vmin = np.float64(np.inf)
    umax = vmax = np.float64(-np.inf)
    front = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for z in (box[2] - box[5] / 2, box[2] + box[5] / 2):
            for x, y in rect:
                x, y = np.float64(x), np.float64(y)
                col = [((x * C[0, k] + y * C[1, k]) + z * C[2, k]) + C[3, k] for k in range(3)]
                d = col[2]
                if not d > 0:
                    continue
                front += 1
                u = np.fmin(np.fmax(col[0] / d, np.float64(0.0)), np.float64(W))
                v = np.fmin(np.fmax(col[1] / d, np.float64(0.0)), np.float64(H))
                umin, umax = np.fmin(umin, u), np.fmax(umax, u)
                vmin, vmax = np.fmin(vmin, v), np.fmax(vmax, v)
    if front == 0:
        return 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    height = vmax - vmin
    return float(umin), float(vmin), float(umax), float(vmax), float(height), float((umax - umin) * height)


def dontcare_ratio(box2d, rect):
    """Share of the 2-D box (umin, vmin, umax, vmax, height, area; area > 0) that lies in the rectangle (l, t, r, b); 0 without overlap."""
    umin, vmin, umax, vmax, _, area = box2d
    l, t, r, b = (float(x) for x in rect)
    iw = min(umax, r) - max(umin, l)
    ih = min(vmax, b) - max(vmin, t)
    if iw > 0 and ih > 0:
        return iw * ih / area
    return 0.0


def det_flags(boxes, C, H, W, dontcare=None, s=None):
    """uint32 [n]: bit d (0..2) iff the projected height < min_height[d]; bit 3 iff the 2-D box has area > 0 and more than
    dontcare_overlap of it lies in one of the DontCare rectangles [D,4] (l, t, r, b)."""
    s = settings({}) if s is None else s
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 7)
    dc = np.zeros((0, 4), np.float32) if dontcare is None else np.asarray(dontcare, dtype=np.float32).reshape(-1, 4)
    out = np.zeros((len(boxes),), dtype=np.uint32)
    for i, b in enumerate(boxes):
        p = project_box(b, C, H, W)
        f = 0
        for d in range(3):
            if p[4] < s["min_height"][d]:
                f |= 1 << d
        if p[5] > 0 and any(dontcare_ratio(p, rc) > s["dontcare_overlap"] for rc in dc):
            f |= 1 << DONTCARE_BIT
        out[i] = f
    return out


# ------------------------------------------------------------------ matching
def row_levels(refs, levels=None):
    """(valid bool [R], level int64 [R]); rows handed in without levels are level 0."""
    refs = np.asarray(refs).reshape(-1, 9)
    lv = np.zeros((len(refs),), dtype=np.int64) if levels is None else np.asarray(levels, dtype=np.int64).reshape(-1)
    if len(lv) != len(refs):
        raise ValueError("levels: %d entries for %d label rows" % (len(lv), len(refs)))
    return refs[:, 8] == 1, lv


def count_rows(refs, levels=None):
    """n_gt int64 [3]: the counted rows per difficulty."""
    valid, lv = row_levels(refs, levels)
    return np.array([int((valid & (lv <= d)).sum()) for d in range(3)], dtype=np.int64)


def match_levels(keep, refs, levels, iou_bev, iou_3d, flags, thresholds):
    """(tpmask, igmask) uint32 [2, n]: per metric, bit 10 d + t set iff the survivor is a true positive / ignored at difficulty d
    and thresholds[t].  Neither bit set: a false positive (or not a survivor)."""
    if len(thresholds) > BITS:
        raise ValueError("at most %d IoU thresholds" % BITS)
    valid, lv = row_levels(refs, levels)
    n = len(keep)
    R = len(valid)
    tpm = np.zeros((2, n), dtype=np.uint32)
    igm = np.zeros((2, n), dtype=np.uint32)
    surv = np.nonzero(keep)[0]
    for m, iou in enumerate((np.asarray(iou_bev, dtype=np.float64).reshape(n, R), np.asarray(iou_3d, dtype=np.float64).reshape(n, R))):
        for d in range(3):
            counted = valid & (lv <= d)
            ignored = valid & ~(lv <= d)
            for t, thr in enumerate(thresholds):
                bit = np.uint32(1 << (BITS * d + t))
                taken = np.zeros((R,), dtype=bool)
                for i in surv:
                    row = iou[i]
                    best, best_r = -np.inf, -1
                    for r in np.nonzero(counted & ~taken)[0]:
                        if row[r] > best:                               # NaN never wins; ascending r keeps the lower row on a tie
                            best, best_r = row[r], r
                    if best_r >= 0 and best > thr:                      # A
                        taken[best_r] = True
                        tpm[m, i] |= bit
                    elif np.any(row[ignored] > thr):                    # B (a NaN compares false)
                        igm[m, i] |= bit
                    elif int(flags[i]) & ((1 << d) | (1 << DONTCARE_BIT)):          # C
                        igm[m, i] |= bit
    return tpm, igm


# ------------------------------------------------------------------ average precision
def average_precision_levels(scores, tpmask, igmask, n_gt, nthr):
    """(ap fp64 [2,3,nthr], tp int64 [2,3,nthr], ignored int64 [2,3,nthr]): evalrank.average_precision of the detections that are
    not ignored at (m, d, t), against n_gt[d]."""
    scores = np.asarray(scores, dtype=np.float32)
    tpmask = np.asarray(tpmask, dtype=np.uint32).reshape(2, -1)
    igmask = np.asarray(igmask, dtype=np.uint32).reshape(2, -1)
    ap = np.full((2, 3, nthr), np.nan, dtype=np.float64)
    tp = np.zeros((2, 3, nthr), dtype=np.int64)
    ig = np.zeros((2, 3, nthr), dtype=np.int64)
    for m in range(2):
        for d in range(3):
            for t in range(nthr):
                sh = np.uint32(BITS * d + t)
                stay = ((igmask[m] >> sh) & np.uint32(1)) == 0
                a, c = ER.average_precision(scores[stay], (tpmask[m][stay] >> sh) & np.uint32(1), int(n_gt[d]), 1)
                ap[m, d, t], tp[m, d, t], ig[m, d, t] = a[0], c[0], int((~stay).sum())
    return ap, tp, ig


def assemble(ap, tp, ig, N, n_gt, thresholds, truncated=0):
    """The dictionary RankedTest.summary() returns under the protocol, from the (m, d, t) arrays."""
    nan = float("nan")
    out = {"protocol": "kitti", "num_P": int(N), "truncated_candidates": int(truncated)}
    for m, metric in enumerate(METRICS):
        out[metric] = {}
        for d, name in enumerate(LEVEL_NAMES):
            g = int(n_gt[d])
            total = 0.0
            for v in ap[m][d]:
                total = total + float(v)
            rest = [int(N) - int(x) for x in ig[m][d]]
            out[metric][name] = {"ap": {t: float(v) for t, v in zip(thresholds, ap[m][d])},
                                 "map": total / len(thresholds),
                                 "tp": {t: int(v) for t, v in zip(thresholds, tp[m][d])},
                                 "precision": {t: (int(v) / k if k else 0.0) for t, v, k in zip(thresholds, tp[m][d], rest)},
                                 "recall": {t: (int(v) / g if g else nan) for t, v in zip(thresholds, tp[m][d])},
                                 "num_T": g,
                                 "num_ignored": {t: int(v) for t, v in zip(thresholds, ig[m][d])}}
    return out


def summarize(scores, tpmask, igmask, n_gt, thresholds, truncated=0):
    """assemble() of average_precision_levels(): the accumulated (score, tpmask[2], igmask[2]) and the counted rows per difficulty."""
    ap, tp, ig = average_precision_levels(scores, tpmask, igmask, n_gt, len(thresholds))
    return assemble(ap, tp, ig, len(np.asarray(scores)), n_gt, thresholds, truncated)


def report_line(summary, iou):
    """One line: 3-D and bird's-eye AP at easy / moderate / hard, at the IoU threshold `iou`."""
    def three(metric):
        return " / ".join("%.4f" % summary[metric][name]["ap"][iou] for name in LEVEL_NAMES)
    return "AP (R40, KITTI-style) at IoU %.2f, easy / moderate / hard: 3-D %s, bird's-eye %s" % (iou, three("3d"), three("bev"))

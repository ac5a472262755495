"""Train-time object pasting ("GT sampling"): the sampler and the host statements of the two kernels.

Per frame and step a handful of labelled objects of an object bank (objbank.py) are pasted into the frame at their own position in
the sensor frame: the scene's points inside the pasted boxes are removed, the bank's points are appended, the labels are appended,
and -- because this model samples camera features at every LiDAR point's pixel -- each object's image patch is painted where its
points project.  The host draws and collision-tests the boxes (draw); the per-point and per-pixel work is csrc/paste.hip
(k_paste_points_b, k_paste_patches_b), whose statements are paste_points and paste_image here.

All numpy, no state: draw() is a pure function of its arguments built like augment.draw (same `base`, same mix64 construction) on
hash streams from 32 upwards -- augment owns 0..4, augment_image 16..25 -- so the three blocks share the trainer's one counter
`aug_calls`, a checkpoint needs no new field, and the other blocks draw what they drew before this module existed.

The inside test, the one expression shared by the bank builder (margin 0), the host statement and the kernel, in np.float32 with
every product and sum rounded and nothing contracted:

    record = (cx, cy, cz, c = cos yaw, s = sin yaw, hl = l/2 + margin, hw = w/2 + margin, hh = h/2 + margin)   float64 -> fp32, once
    dx = x - cx   dy = y - cy   lx = fl(fl(dx c) + fl(dy s))   ly = fl(fl(dy c) - fl(dx s))
    inside  iff  |lx| <= hl  and  |ly| <= hw  and  |z - cz| <= hh          (a NaN or infinite coordinate compares false)
"""
import math

import numpy as np

from . import cfgcheck as C
from .augment import M64, mix64

MAX_RECORDS = 16           # records per frame: the kernels' table holds 16
NREC = 8                   # cx cy cz c s hl hw hh
NPATCH = 9                 # x0 y0 w h sx sy pw ph start
_CAND0 = 33                # candidate j draws on hash stream 33 + j (32 is kept free)
_STREAMS = np.arange(_CAND0, _CAND0 + MAX_RECORDS, dtype=np.uint64)
KEYS = ("enabled", "seed", "bank", "target_objects", "max_candidates", "margin", "paste_image")


# ------------------------------------------------------------------------------------------------ the inside test
def record(row, margin=0.0):
    """The eight fp32 numbers of one label row (x, y, z, l, w, h, yaw, ...): computed in float64, rounded here, once."""
    r = np.asarray(row, dtype=np.float64)
    m = float(margin)
    return np.array([r[0], r[1], r[2], math.cos(r[6]), math.sin(r[6]), r[3] / 2 + m, r[4] / 2 + m, r[5] / 2 + m], dtype=np.float64).astype(np.float32)


def inside_mask(pts_f32, rec):
    """bool [n]: the inside test of the module docstring for the rows of pts [n,3] fp32 against one record."""
    p = np.asarray(pts_f32, dtype=np.float32).reshape(-1, 3)
    q = np.asarray(rec, dtype=np.float32).reshape(NREC)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = p[:, 0] - q[0]
        dy = p[:, 1] - q[1]
        lx = (dx * q[3]).astype(np.float32) + (dy * q[4]).astype(np.float32)
        ly = (dy * q[3]).astype(np.float32) - (dx * q[4]).astype(np.float32)
        return (np.abs(lx) <= q[5]) & (np.abs(ly) <= q[6]) & (np.abs(p[:, 2] - q[2]) <= q[7])


# ------------------------------------------------------------------------------------------------ geometry on the host
def footprint(row, margin=0.0):
    """evalgeom.bev_rect of a label row, its length and width grown by 2 * margin: float64 [4,2]."""
    from .evalgeom import bev_rect
    m = 2.0 * float(margin)
    return np.array(bev_rect((row[0], row[1]), (float(row[3]) + m, float(row[4]) + m), row[6]), dtype=np.float64)


def _normals(rect):
    """The four unit edge normals of evalgeom.rects_overlap for one polygon (four (x, y)), with its own arithmetic: Python floats and
    math.hypot (numpy's hypot differs from it in the last bit for about one input in two hundred, which could turn a tie)."""
    pts = rect.tolist() if isinstance(rect, np.ndarray) else rect
    out = []
    for i in range(4):
        p, q = pts[i], pts[(i + 1) % 4]
        ex, ey = q[0] - p[0], q[1] - p[1]
        nx, ny = ey, -ex
        norm = math.hypot(nx, ny)
        out.append((nx / norm, ny / norm))
    return out


def overlap_pairs(A, nA, B, nB):
    """evalgeom.rects_overlap(A[i], B[k]) for every pair at once: bool [n,K].  A [n,4,2], B [K,4,2] float64 polygons, nA / nB their
    unit edge normals (_normals) [n,4,2] / [K,4,2].  The closed separating-axis test on the four normals of either polygon; every
    projection is the same two products and one sum as in the scalar function, so touching and identical rectangles decide alike.
    Array operations only: no Python loop over pairs."""
    n, K = A.shape[0], B.shape[0]
    if n == 0 or K == 0:
        return np.zeros((n, K), dtype=bool)
    axes = np.concatenate([np.broadcast_to(nA[:, None], (n, K, 4, 2)), np.broadcast_to(nB[None], (n, K, 4, 2))], 2)      # [n,K,8,2]
    ax, ay = axes[..., 0:1], axes[..., 1:2]                                                                           # [n,K,8,1]
    pa = A[:, None, None, :, 0] * ax + A[:, None, None, :, 1] * ay                                                    # [n,K,8,4]
    pb = B[None, :, None, :, 0] * ax + B[None, :, None, :, 1] * ay
    # (the extrema over the four corners as element-wise maxima: numpy's reductions over a short last axis cost several times that)
    amax, amin = np.maximum(np.maximum(pa[..., 0], pa[..., 1]), np.maximum(pa[..., 2], pa[..., 3])), np.minimum(np.minimum(pa[..., 0], pa[..., 1]), np.minimum(pa[..., 2], pa[..., 3]))
    bmax, bmin = np.maximum(np.maximum(pb[..., 0], pb[..., 1]), np.maximum(pb[..., 2], pb[..., 3])), np.minimum(np.minimum(pb[..., 0], pb[..., 1]), np.minimum(pb[..., 2], pb[..., 3]))
    apart = (amax < bmin) | (bmax < amin)
    return ~apart.any(2)


def overlap_many(rect, rects, normals=None, rect_normals=None):
    """evalgeom.rects_overlap(rect, rects[k]) for every k at once: bool [K] (overlap_pairs with one polygon on the left).
    rect [4,2], rects [K,4,2] float64; normals [K,4,2] / rect_normals [4,2]: the unit normals when the caller has them."""
    rect = np.asarray(rect, dtype=np.float64).reshape(1, 4, 2)
    rects = np.asarray(rects, dtype=np.float64).reshape(-1, 4, 2)
    na = np.array(_normals(rect[0]) if rect_normals is None else rect_normals, dtype=np.float64).reshape(1, 4, 2)
    nb = np.array([_normals(r) for r in rects] if normals is None else normals, dtype=np.float64).reshape(-1, 4, 2)
    return overlap_pairs(rect, na, rects, nb)[0]


def _prepared(bank, margin):
    """What draw() needs of a bank at one margin, computed once and kept in the bank dict under "_prepared" (objbank.save does
    not write it): float64 rows, footprints and their normals, plain and grown by the margin, the fp32 records, point counts and
    float64 distances.  A bank is read-only once it has been drawn from."""
    cache = bank.setdefault("_prepared", {})
    prep = cache.get(margin)
    if prep is None:
        rows = np.asarray(bank["boxes"], dtype=np.float64)
        fp = [footprint(r) for r in rows]
        grown = [footprint(r, margin) for r in rows]
        starts = np.asarray(bank["point_start"], dtype=np.int64)
        prep = cache[margin] = {
            "rows": rows, "fp": np.stack(fp, 0), "nfp": np.array([_normals(f) for f in fp], dtype=np.float64),
            "grown": np.stack(grown, 0), "ngrown": np.array([_normals(f) for f in grown], dtype=np.float64),
            "records": np.stack([record(r, margin) for r in bank["boxes"]], 0), "labels": np.ascontiguousarray(np.asarray(bank["boxes"], dtype=np.float32)),
            "starts": starts, "counts": (starts[1:] - starts[:-1]).tolist(), "dist": [math.hypot(float(r[0]), float(r[1])) for r in rows]}
    return prep


def project_px(points, crt):
    """[p, 1] . crt = (a0, a1, a2) in float64 for the rows of points [n,3]: (u = a0 / a2 [n], v = a1 / a2 [n], a2 [n]) -- the
    convention augment_image.compose_crt_image documents (u along the width).  Rows with a2 <= 0 carry nan."""
    c = np.asarray(crt, dtype=np.float64).reshape(4, 3)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    a = p @ c[0:3] + c[3]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = a[:, 2] > 0
        u = np.where(ok, a[:, 0] / np.where(ok, a[:, 2], 1.0), np.nan)
        v = np.where(ok, a[:, 1] / np.where(ok, a[:, 2], 1.0), np.nan)
    return u, v, a[:, 2]


def centre_pixel(row, crt):
    """The box centre's projected pixel rounded to the nearest integers, or None when it lies behind the camera (a2 <= 0)."""
    u, v, a2 = project_px(np.asarray(row[:3], dtype=np.float64)[None], crt)
    if not (a2[0] > 0 and np.isfinite(u[0]) and np.isfinite(v[0])):
        return None
    lim = float(2 ** 30)
    return int(np.rint(min(max(u[0], -lim), lim))), int(np.rint(min(max(v[0], -lim), lim)))


def _centre_pixels(rows, crt):
    """centre_pixel for the rows [n, >=3] at once: a list of (u, v) integers or None."""
    u, v, a2 = project_px(rows[:, :3], crt)
    lim = float(2 ** 30)
    with np.errstate(invalid="ignore"):
        ok = (a2 > 0) & np.isfinite(u) & np.isfinite(v)
        ui, vi = np.rint(np.clip(u, -lim, lim)), np.rint(np.clip(v, -lim, lim))
    return [(int(ui[k]), int(vi[k])) if ok[k] else None for k in range(len(ok))]


def destination(rect, centre_px, row, crt, image_hw, here=False):
    """Destination rectangle of a patch in a frame with the calibration `crt`: the bank's rect (x0, y0, w, h) translated by the
    integer vector round(projection of the box centre under crt) - centre_px, clipped to the image [H, W]; the source offset
    inside the patch moves with the clipping.  Returns (x0, y0, w, h, sx, sy) or None (no patch, centre behind the camera, or
    nothing left after the clipping).  here: centre_pixel(row, crt) when the caller has it."""
    x0, y0, w, h = (int(v) for v in rect)
    if w <= 0 or h <= 0:
        return None
    if here is False:
        here = centre_pixel(row, crt)
    if here is None:
        return None
    H, W = int(image_hw[0]), int(image_hw[1])
    ax, ay = x0 + here[0] - int(centre_px[0]), y0 + here[1] - int(centre_px[1])
    bx, by = max(ax, 0), max(ay, 0)
    ex, ey = min(ax + w, W), min(ay + h, H)
    if ex <= bx or ey <= by:
        return None
    return bx, by, ex - bx, ey - by, bx - ax, by - ay


# ------------------------------------------------------------------------------------------------ the sampler
def check_config(cfg):
    """Range checks of the parsed block (parse_config's dict, or any dict with those keys): ValueError."""
    C.integer("augment_paste.target_objects", cfg.get("target_objects", 15), lo=0)
    C.integer("augment_paste.max_candidates", cfg.get("max_candidates", 16), lo=1, hi=MAX_RECORDS)
    C.number("augment_paste.margin", cfg.get("margin", 0.0), nonneg=True)


def parse_config(config):
    """The `augment_paste` block, validated like `augment`: None = off (no block, or enabled: false), else
    {"seed", "bank" (path of the .npz), "target_objects", "max_candidates" (1..16), "margin" (metres, >= 0), "paste_image"}.  Bad
    values raise ValueError whether the block is enabled or not; an enabled block needs a bank."""
    got = C.seeded_block(config, "augment_paste", KEYS)
    if got is None:
        return None
    blk, enabled, seed = got
    with_image = C.flag("augment_paste.paste_image", blk.get("paste_image", True))
    bank = blk.get("bank", None)
    if bank is not None and not isinstance(bank, str):
        raise ValueError("augment_paste.bank must be the path of an object bank (got %r)" % (bank,))
    out = {"seed": seed, "bank": bank, "target_objects": blk.get("target_objects", 15), "max_candidates": blk.get("max_candidates", 16),
           "margin": blk.get("margin", 0.0), "paste_image": with_image}
    check_config(out)
    out["margin"] = float(out["margin"])
    if not enabled:
        return None
    if not bank:
        raise ValueError("augment_paste.bank: an enabled block needs the path of an object bank (python -m <package>.objbank --out PATH)")
    return out


def check_bank(bank, image_hw=None):
    """A bank the sampler can draw from: M >= 1, consistent arrays and, given image_hw = (H, W), patches cut from such images."""
    need = ("points", "point_start", "boxes", "rect", "patch", "patch_start", "centre_px", "image_hw")
    missing = [k for k in need if k not in bank]
    if missing:
        raise ValueError("object bank: missing arrays %s" % missing)
    M = int(np.asarray(bank["boxes"]).shape[0])
    if M < 1:
        raise ValueError("object bank: no objects (M = 0)")
    if np.asarray(bank["point_start"]).shape != (M + 1,) or np.asarray(bank["patch_start"]).shape != (M + 1,) or np.asarray(bank["rect"]).shape != (M, 4):
        raise ValueError("object bank: inconsistent array shapes")
    if image_hw is not None and tuple(int(v) for v in bank["image_hw"]) != tuple(int(v) for v in image_hw):
        raise ValueError("object bank: patches of %s images for %s ones" % (tuple(int(v) for v in bank["image_hw"]), tuple(int(v) for v in image_hw)))


def empty_plan(n_points, image_hw):
    return {"rows": [], "labels": np.zeros((0, 9), dtype=np.float32), "records": np.zeros((0, NREC), dtype=np.float32),
            "append": np.zeros((0, 2), dtype=np.int64), "patches": np.zeros((0, NPATCH), dtype=np.int64), "patch_rows": [],
            "n_points": int(n_points), "image_hw": (int(image_hw[0]), int(image_hw[1]))}


def draw(cfg, seed, rank, call, b, bank, boxes, num, n_points, crt, config):
    """The plan of frame b of the call-th augmented step on `rank`.  cfg: the dict of parse_config; bank: objbank's
    dict; boxes [max_num_bbox, 9] with the first `num` rows valid, n_points and crt [4,3]: the frame's own labels, point count
    and calibration; config: the dataset config (ranges, max_num_bbox, max_num_pc).

    want = min(max(target_objects - num, 0), max_candidates, 16) candidates, candidate j = bank row floor(u(33 + j) M), accepted
    greedily in j order iff its centre passes CarlaDataset.valid_bbox, its footprint grown by `margin` overlaps (closed
    separating-axis test) neither a valid label nor an accepted candidate, a label row is free, the points fit max_num_pc and --
    with paste_image -- it has a patch whose shifted, clipped destination is not empty.

    Returns {"rows": accepted bank rows in acceptance order, "labels" fp32 [k,9], "records" fp32 [k,8] (margin included),
    "append" int64 [k,2] = (bank start, count), "patches" int64 [p,9] = (x0, y0, w, h, sx, sy, pw, ph, patch start) ordered far
    to near (descending float64 hypot(x, y), ties by acceptance order: the later record is painted on top), "patch_rows": the
    bank row of each patch record, "n_points", "image_hw"}."""
    check_config(cfg)
    check_bank(bank)
    image_hw = (int(bank["image_hw"][0]), int(bank["image_hw"][1]))
    num, n_points = int(num), int(n_points)
    plan = empty_plan(n_points, image_hw)
    M = int(bank["boxes"].shape[0])
    want = min(max(int(cfg.get("target_objects", 15)) - num, 0), int(cfg.get("max_candidates", 16)), MAX_RECORDS)
    if want == 0:
        return plan
    base = (int(seed) * 0x9E3779B1 + int(call) + int(rank) * 0x85EBCA77C2B2AE63) & M64      # augment.draw's formula
    with np.errstate(over="ignore"):
        hv = mix64(np.uint64(base) ^ mix64(np.uint64((int(b) << 8) & M64) | _STREAMS[:want]))
    uni = (hv >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    cand = np.minimum(np.floor(uni * M).astype(np.int64), M - 1)
    margin, with_image = float(cfg.get("margin", 0.0)), bool(cfg.get("paste_image", True))
    max_box, max_pc = int(config["max_num_bbox"]), int(config["max_num_pc"])
    xlo, xhi, ylo, yhi = config["lidar_x_min"], config["lidar_x_max"], config["lidar_y_min"], config["lidar_y_max"]
    prep = _prepared(bank, margin)
    crow = prep["rows"][cand]
    in_range = ((crow[:, 0] >= xlo) & (crow[:, 0] < xhi) & (crow[:, 1] >= ylo) & (crow[:, 1] < yhi)).tolist()      # CarlaDataset.valid_bbox
    # the collision tests of all candidates in ONE batched call: every grown candidate against the frame's valid labels and against
    # every candidate's own (ungrown) footprint -- the greedy pass below only looks the answers up
    others, nothers = prep["fp"][cand], prep["nfp"][cand]
    if num:
        src = np.asarray(boxes, dtype=np.float64)
        lab = [footprint(src[i]) for i in range(num)]
        others = np.concatenate([np.stack(lab, 0), others], 0)
        nothers = np.concatenate([np.array([_normals(f) for f in lab], dtype=np.float64), nothers], 0)
    table = overlap_pairs(prep["grown"][cand], prep["ngrown"][cand], others, nothers).tolist()
    hits_label = [any(t[:num]) for t in table]
    hits = [t[num:] for t in table]
    here = _centre_pixels(crow, crt) if with_image else None
    cand, counts, pstarts = cand.tolist(), prep["counts"], bank["patch_start"]
    picked, rows, dests, appended = [], [], [], 0
    for j in range(want):
        r = cand[j]
        if not in_range[j] or hits_label[j]:
            continue
        if num + len(rows) >= max_box:
            break
        if n_points + appended + counts[r] > max_pc:
            continue
        if any(hits[j][k] for k in picked):                 # (a bank row drawn twice meets its own footprint)
            continue
        dest = None
        if with_image:
            dest = destination(bank["rect"][r], bank["centre_px"][r], crow[j], crt, image_hw, here=here[j])
            if dest is None:
                continue
        picked.append(j)
        rows.append(r)
        dests.append(dest)
        appended += counts[r]
    if not rows:
        return plan
    sel = np.asarray(rows, dtype=np.int64)
    plan["rows"] = rows
    plan["labels"] = prep["labels"][sel]
    plan["records"] = prep["records"][sel]
    plan["append"] = np.stack([prep["starts"][sel], prep["starts"][sel + 1] - prep["starts"][sel]], 1)
    if with_image:
        order = sorted(range(len(rows)), key=lambda k: (-prep["dist"][rows[k]], k))
        pt = np.empty((len(rows), NPATCH), dtype=np.int64)
        for o, k in enumerate(order):
            r = rows[k]
            pt[o, 0:6] = dests[k]
            pt[o, 6], pt[o, 7], pt[o, 8] = int(bank["rect"][r][2]), int(bank["rect"][r][3]), int(pstarts[r])
        plan["patches"] = pt
        plan["patch_rows"] = [rows[k] for k in order]
    return plan


def append_labels(boxes, num, plan):
    """The frame's label tensor with the plan's rows after its own: (boxes' [max_num_bbox, 9] float32 copy, num')."""
    out = np.array(boxes, dtype=np.float32, copy=True)
    num, k = int(num), len(plan["rows"])
    if num + k > out.shape[0]:
        raise ValueError("paste: %d labels and %d pasted objects in %d rows" % (num, k, out.shape[0]))
    out[num:num + k] = plan["labels"]
    return out, num + k


# ------------------------------------------------------------------------------------------------ the host statements
def paste_points(pts, plan, bank):
    """fp32 [n,3] -> fp32 [n + a, 3], the statement of k_paste_points_b: row i < n is the source row bit for bit, or (+inf, +inf,
    +inf) when the point is inside any record; the rows behind are the bank's, object after object in record order, bit for bit."""
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
    gone = np.zeros(p.shape[0], dtype=bool)
    for q in plan["records"]:
        gone |= inside_mask(p, q)
    head = p.copy()
    head[gone] = np.inf
    bp = np.asarray(bank["points"], dtype=np.float32).reshape(-1, 3)
    return np.concatenate([head] + [bp[int(s):int(s) + int(c)] for s, c in plan["append"]], 0)


def paste_image(img, plan, bank):
    """uint8 [3,H,W] -> uint8 [3,H,W], the statement of k_paste_patches_b: every output byte (c, y, x) is the byte
    patch[start + (c ph + (y - y0 + sy)) pw + (x - x0 + sx)] of the LAST listed record whose destination rectangle contains (x, y),
    the input byte where none does.  A function of the destination pixel alone."""
    src = np.asarray(img)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[0] != 3:
        raise ValueError("image must be uint8 [3,H,W] (got %s %s)" % (src.dtype, src.shape))
    _, H, W = src.shape
    owner = np.full((H, W), -1, dtype=np.int64)
    for j, q in enumerate(plan["patches"]):
        owner[int(q[1]):int(q[1]) + int(q[3]), int(q[0]):int(q[0]) + int(q[2])] = j
    out = src.copy()
    patch = np.asarray(bank["patch"], dtype=np.uint8).reshape(-1)
    ys, xs = np.nonzero(owner >= 0)
    if len(ys):
        q = np.asarray(plan["patches"], dtype=np.int64)[owner[ys, xs]]
        py, px = ys - q[:, 1] + q[:, 5], xs - q[:, 0] + q[:, 4]
        for c in range(3):
            out[c, ys, xs] = patch[q[:, 8] + (c * q[:, 7] + py) * q[:, 6] + px]
    return out

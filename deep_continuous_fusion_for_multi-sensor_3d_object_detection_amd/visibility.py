"""The camera visibility mask: which LiDAR rows the camera sees, stated on the host.

Two rules turn a row into (+inf, +inf, +inf) -- the convention of the point drop and of object pasting: every range test of the
library rejects such a row, nothing is compacted and the point counts stay host-known:

    fov_crop          the row fails the projection kernel's own predicate (ProjPred of csrc/geometry.hip): outside the strict
                      range test, outside 0 < u < ulim, 0 < v < vlim, or -- mode `correct` -- a2 <= 0
    paste_occlusion   the row projects into the destination rectangle of a pasted patch and lies behind the pasted object:
                      u >= x0 && u < x1 && v >= y0 && v < y1 && a2 > D for an occluder (x0, y0, x1, y1, D)

Both decide on the projection kernel's fp32 chain (project_chain).  csrc/camera_mask.hip is the device side; mask_points is its
statement, bit for bit.  drop_covering is the other half of paste_occlusion: a candidate whose patch would be painted over a
nearer labelled object of the frame is not pasted at all.  All numpy, no state.
"""
import numpy as np

from . import cfgcheck as C
from . import paste

MAX_OCCLUDERS = 16         # occluders per frame: one per patch record (paste.MAX_RECORDS)
NOCC = 5                   # x0 y0 x1 y1 D
SLACK = 2.0 ** -6          # metres added to the far corner's depth: an object never hides its own points
KEYS = ("fov_crop", "paste_occlusion")
PROJ_COMPAT, PROJ_CORRECT = 0, 1


def parse_config(config):
    """The `camera_mask` block by itself: None = off (no block, or both switches false), else {"fov_crop", "paste_occlusion"}.
    Unknown keys and non-boolean values raise ValueError.  (train.parse_camera_mask_config adds the dependency on augment_paste.)"""
    blk = config.get("camera_mask", None)
    if blk is None:
        return None
    C.block("camera_mask", blk, KEYS)
    out = {key: C.flag("camera_mask." + key, blk.get(key, False)) for key in KEYS}
    return out if (out["fov_crop"] or out["paste_occlusion"]) else None


# ------------------------------------------------------------------------------------------------ the fp32 chain
def _fma32(a, b, c):
    """fl32(a b + c) with ONE rounding for fp32 arrays: the product is exact in float64 (48 bits), the float64 sum is rounded to
    odd (TwoSum tells whether it was exact and which way the error points), and 53 >= 2 * 24 + 2 bits make the final cast to fp32
    the correctly rounded result.  The plain float64 form rounds twice and is wrong for about one input in 2^29."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def project_chain(pts_f32, crt_f32):
    """(u, v, a2) fp32 [n] of the rows of pts [n,3] under the [4,3] matrix: ProjPred's chain of csrc/geometry.hip,
        a_j = fma(1, c[3][j], fma(z, c[2][j], fma(y, c[1][j], fl(x c[0][j]))))      u = fl(a0 / a2)      v = fl(a1 / a2)
    every fma a single rounding.  Non-finite rows give whatever IEEE arithmetic gives (NaN, inf): the callers only compare."""
    p = np.ascontiguousarray(np.asarray(pts_f32, dtype=np.float32).reshape(-1, 3))
    c = np.asarray(crt_f32, dtype=np.float32).reshape(4, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    one = np.ones_like(x)
    a = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(3):
            t = (x.astype(np.float64) * np.float64(c[0, j])).astype(np.float32)
            t = _fma32(y, np.full_like(x, c[1, j]), t)
            t = _fma32(z, np.full_like(x, c[2, j]), t)
            t = _fma32(one, np.full_like(x, c[3, j]), t)
            a.append(t)
        u = (a[0].astype(np.float64) / a[2].astype(np.float64)).astype(np.float32)
        v = (a[1].astype(np.float64) / a[2].astype(np.float64)).astype(np.float32)
    return u, v, a[2]


def _in_range(p, lim6):
    l = np.asarray(lim6, dtype=np.float32).reshape(6)
    with np.errstate(invalid="ignore"):
        return (p[:, 0] > l[0]) & (p[:, 0] < l[1]) & (p[:, 1] > l[2]) & (p[:, 1] < l[3]) & (p[:, 2] > l[4]) & (p[:, 2] < l[5])


def _keep(p, lim6, ulim, vlim, mode, u, v, a2):
    with np.errstate(invalid="ignore"):
        keep = _in_range(p, lim6) & (u > np.float32(0)) & (u < np.float32(ulim)) & (v > np.float32(0)) & (v < np.float32(vlim))
        if int(mode) == PROJ_CORRECT:
            keep &= a2 > np.float32(0)
    return keep


def fov_keep(pts, crt, lim6, ulim, vlim, mode):
    """bool [n]: exactly ProjPred -- the strict range test, 0 < u < ulim, 0 < v < vlim and, in mode `correct` (1), a2 > 0.  ulim /
    vlim are FrameGeometry.limits()'s, so compat's swapped bounds are inherited."""
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
    u, v, a2 = project_chain(p, crt)
    return _keep(p, lim6, ulim, vlim, mode, u, v, a2)


# ------------------------------------------------------------------------------------------------ pasted patches as occluders
def _box_corners(row):
    """The eight corners objbank.patch_rect projects: evalgeom.bev_rect's footprint at z -+ h/2."""
    fp = paste.footprint(row)
    z, hh = float(row[2]), float(row[5]) / 2
    return np.array([(x, y, zz) for zz in (z - hh, z + hh) for x, y in fp], dtype=np.float64)


def occluders(plan, bank, crt):
    """fp32 [p,5] = (x0, y0, x1, y1, D), one per patch record of the plan, in its order (far to near): the record's clipped
    destination rectangle, x1 = x0 + w, y1 = y0 + h, and D = fl32(max over the box's eight corners of a2 + 2^-6) under THIS frame's
    matrix, in float64.  a2 is affine in the point, so every point inside the box lies at or in front of the far corner; the slack
    is three orders of magnitude over the fp32 rounding of the inside test and the chain.  A record whose corner depths are not all
    finite and positive gives no occluder."""
    out = []
    for q, r in zip(np.asarray(plan["patches"], dtype=np.int64).reshape(-1, paste.NPATCH), plan["patch_rows"]):
        _, _, a2 = paste.project_px(_box_corners(np.asarray(bank["boxes"][int(r)], dtype=np.float64)), crt)
        if not (np.isfinite(a2).all() and (a2 > 0).all()):
            continue
        out.append((float(q[0]), float(q[1]), float(q[0] + q[2]), float(q[1] + q[3]), float(a2.max()) + SLACK))
    return np.asarray(out, dtype=np.float64).reshape(-1, NOCC).astype(np.float32)


def hidden(u, v, a2, occ):
    """bool [n]: exists j: u >= x0 && u < x1 && v >= y0 && v < y1 && a2 > D, fp32 compares; a NaN compares false."""
    u, v, a2 = (np.asarray(t, dtype=np.float32).reshape(-1) for t in (u, v, a2))
    out = np.zeros(u.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for q in np.asarray(occ, dtype=np.float32).reshape(-1, NOCC):
            out |= (u >= q[0]) & (u < q[2]) & (v >= q[1]) & (v < q[3]) & (a2 > q[4])
    return out


def gone_mask(pts, crt, lim6, ulim, vlim, mode, fov, occ):
    """bool [n]: (fov and not fov_keep) or hidden -- the rows mask_points overwrites."""
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
    u, v, a2 = project_chain(p, crt)
    gone = hidden(u, v, a2, np.zeros((0, NOCC), dtype=np.float32) if occ is None else occ)
    if fov:
        gone |= ~_keep(p, lim6, ulim, vlim, mode, u, v, a2)
    return gone


def mask_points(pts, crt, lim6, ulim, vlim, mode, fov, occ):
    """fp32 [n,3] -> fp32 [n,3], the statement of k_camera_mask_b: row i becomes (+inf, +inf, +inf) iff (fov and not fov_keep_i) or
    hidden_i; every other row is kept bit for bit (a NaN keeps its payload).  fov false and no occluders: a copy."""
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
    out = p.copy()
    out.view(np.uint32)[gone_mask(p, crt, lim6, ulim, vlim, mode, fov, occ)] = np.uint32(0x7F800000)
    return out


# ------------------------------------------------------------------------------------------------ candidates over nearer labels
def _meet(r, q):
    """Integer half-open rectangles (x0, y0, w, h) with a non-empty intersection."""
    return max(r[0], q[0]) < min(r[0] + r[2], q[0] + q[2]) and max(r[1], q[1]) < min(r[1] + r[3], q[1] + q[3])


def covering(plan, boxes, num, crt, bank):
    """The accepted bank rows of the plan that drop_covering removes, in acceptance order."""
    from . import objbank
    patches = np.asarray(plan["patches"], dtype=np.int64).reshape(-1, paste.NPATCH)
    if not len(patches) or int(num) <= 0:
        return []
    src = np.asarray(boxes, dtype=np.float64)
    labels = []
    for i in range(int(num)):
        rect = objbank.patch_rect(src[i], crt, plan["image_hw"])
        if rect[2] > 0 and rect[3] > 0:
            labels.append((rect, float(paste.project_px(src[i, :3][None], crt)[2][0])))
    gone = set()
    for q, r in zip(patches, plan["patch_rows"]):
        e = float(paste.project_px(np.asarray(bank["boxes"][int(r)], dtype=np.float64)[:3][None], crt)[2][0])
        dest = tuple(int(t) for t in q[0:4])
        if any(_meet(rect, dest) and d < e for rect, d in labels):
            gone.add(int(r))
    return [int(r) for r in plan["rows"] if int(r) in gone]


def drop_covering(plan, boxes, num, crt, bank):
    """The plan without the accepted objects whose patch would be painted over a NEARER labelled object of the frame.  For every
    valid label i < num: R_i = objbank.patch_rect(row_i, crt, image_hw), d_i = a2 of its centre (float64, paste.project_px); for
    every accepted object k with a patch record: its destination rectangle Q_k and e_k = a2 of its centre under this frame's
    matrix.  k is dropped iff some i has w_i > 0, R_i and Q_k meet (integer, half-open) and d_i < e_k.  The result is a new plan
    with `rows`, `labels`, `records`, `append`, `patches` and `patch_rows` filtered, orders kept; the argument is not written, and
    a plan with nothing dropped comes back equal."""
    gone = set(covering(plan, boxes, num, crt, bank))
    keep = [k for k, r in enumerate(plan["rows"]) if int(r) not in gone]
    pkeep = [k for k, r in enumerate(plan["patch_rows"]) if int(r) not in gone]
    out = dict(plan)
    out["rows"] = [plan["rows"][k] for k in keep]
    for key in ("labels", "records", "append"):
        out[key] = np.array(np.asarray(plan[key])[keep], copy=True)
    out["patches"] = np.array(np.asarray(plan["patches"])[pkeep], copy=True)
    out["patch_rows"] = [plan["patch_rows"][k] for k in pkeep]
    return out

"""CPU suite: every host statement of rotated-box IoU (evalrank.bev_iou, evalgeom.rotated_iou, evalkitti.iou_pair, assign.anchor_iou --
all through evalgeom._clip_convex) against the exact rational clip of tests/_iou_exact.py, on the families of pairs whose edges share a
line up to rounding.  The device is pinned to the same exact values in tests/test_gpu_iou_exact.py.

The bound is 1e-9: the corners are fp64 at magnitude <= 150, a few ulps of corner error (3e-14) times a perimeter <= 16 over areas >= 1 is
about 1e-12, which leaves three orders of margin; the failures it has to catch are >= 1e-2 or NaN.  With `t = cross(e, a - q) / cross(e,
p - q)` as the crossing parameter this file failed with the two explicit pairs NaN and errors of 0.6 and 0.9 in the concentric families;
with `t = sq / (sq - sp)` the worst difference over everything below is 1.8e-11 (printed by each test, recorded in DESIGN.md section 13)."""
import math

import numpy as np
import pytest

import _iou_exact as X
from _util import pkg

BOUND = 1e-9
PER_FAMILY = 128
_DATA = {}


def data():
    """Both layouts once: 128 pairs per family with centres in [0, 70] x [-40, 40] and the 64 per family of the GPU tests on their grid."""
    if not _DATA:
        a1, b1, f1 = X.family_pairs(PER_FAMILY, 9101)
        a2, b2, f2, _ = X.spaced_case()
        _DATA.update(first=np.concatenate([a1, a2]), second=np.concatenate([b1, b2]), family=np.concatenate([f1, f2]))
        _DATA["rect"] = [(X.rect_of(a), X.rect_of(b)) for a, b in zip(_DATA["first"], _DATA["second"])]
        _DATA["exact"] = np.array([X.exact_kitti(r1, a[2], a[5], r2, b[2], b[5]) for (r1, r2), a, b in zip(_DATA["rect"], _DATA["first"], _DATA["second"])])
    return _DATA


def compare(name, got, want, family):
    """Finite wherever the exact value is, and within the bound; the count per family is printed before anything is asserted."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(want).all()
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= BOUND)
    err = np.where(np.isfinite(got), np.abs(got - want), 0.0)
    for k in sorted(set(family.tolist())):
        sel = family == k
        print("%s, %s: %d of %d not finite, %d beyond %g, worst finite error %.3g" % (name, X.FAMILIES[k] if k >= 0 else "explicit", int((~np.isfinite(got[sel])).sum()),
              int(sel.sum()), int(bad[sel].sum()), BOUND, float(err[sel].max())))
    assert np.isfinite(got).all(), "%s: %d values are not finite where the exact IoU is" % (name, int((~np.isfinite(got)).sum()))
    assert not bad.any(), "%s: %d values differ from the exact IoU by more than %g, worst %.3g" % (name, int(bad.sum()), BOUND, float(err.max()))


# ------------------------------------------------------------------ the reference against closed forms
def square(cx, cy, half, turn=0.0):
    return [(cx + half * math.sqrt(2) * math.cos(turn + k * math.pi / 2 + math.pi / 4), cy + half * math.sqrt(2) * math.sin(turn + k * math.pi / 2 + math.pi / 4))
            for k in range(4)]


def box(x, y, l, w):
    return [(x - l / 2, y - w / 2), (x + l / 2, y - w / 2), (x + l / 2, y + w / 2), (x - l / 2, y + w / 2)]


def test_reference_equals_closed_forms():
    s = box(0.25, -3.0, 2.0, 2.0)
    assert X.exact_bev(s, s) == 1.0 and X.exact_bev(s, s[::-1]) == 1.0 and X.exact_bev(s[::-1], s) == 1.0          # either orientation
    ia, a1, a2 = X.exact_areas(square(0.0, 0.0, 1.0), square(0.0, 0.0, 1.0, math.pi / 4))                            # a regular octagon
    assert abs(float(ia) - 8.0 * (math.sqrt(2.0) - 1.0)) <= 1e-14 and abs(float(a1) - 4.0) <= 1e-14 and abs(float(a2) - 4.0) <= 1e-14
    for l, w in ((4.0, 2.0), (1.5, 0.75)):                                # dyadic sizes and shifts: every corner is exact
        for num in (1, 3, 5, 7):
            f = num / 8.0
            want = (1.0 - f) / (1.0 + f)
            assert X.exact_bev(box(8.0, -2.0, l, w), box(8.0 + f * l, -2.0, l, w)) == want
            assert X.exact_bev(box(8.0, -2.0, l, w)[::-1], box(8.0, -2.0 - f * w, l, w)) == want
    assert X.exact_bev(box(0.0, 0.0, 4.0, 2.0), box(4.5, 0.0, 4.0, 2.0)) == 0.0                                      # disjoint
    assert X.exact_bev(box(0.0, 0.0, 4.0, 2.0), box(4.0, 0.0, 4.0, 2.0)) == 0.0                                      # touching along an edge
    assert X.exact_bev(box(0.0, 0.0, 4.0, 2.0), box(4.0, 2.0, 4.0, 2.0)) == 0.0                                      # touching in a corner
    assert X.exact_bev(box(0.0, 0.0, 4.0, 2.0), box(0.5, 0.25, 2.0, 1.0)) == 0.25                                    # one inside the other
    assert math.isnan(X.exact_bev(box(1.0, 1.0, 0.0, 0.0), box(1.0, 1.0, 0.0, 0.0)))                                 # a zero-area pair
    assert X.exact_bev(box(1.0, 1.0, 0.0, 0.0), box(1.0, 1.0, 2.0, 2.0)) == 0.0
    # the 3-D values: exact area times the overlap of the extents over the volumes
    bev, i3d = X.exact_kitti(box(0.0, 0.0, 4.0, 2.0), 0.0, 2.0, box(1.0, 0.0, 4.0, 2.0), 0.5, 2.0)
    assert bev == 6.0 / 10.0 and i3d == (6.0 * 1.5) / (16.0 + 16.0 - 9.0)
    assert X.exact_kitti(box(0.0, 0.0, 4.0, 2.0), 0.0, 2.0, box(1.0, 0.0, 4.0, 2.0), 2.5, 2.0)[1] == 0.0
    EG = pkg("evalgeom")
    c1, c2 = EG.box_corners((0.0, 0.0, 0.0), (4.0, 2.0, 2.0), 0.0), EG.box_corners((1.0, 0.5, 0.0), (4.0, 2.0, 2.0), 0.0)
    assert X.exact_rotated(c1, c2) == ((6.0 * 1.5) / (16.0 + 16.0 - 9.0), 6.0 / 10.0)


def test_explicit_pairs_and_families_are_what_they_claim():
    d = data()
    for a, b, fam, (e_bev, _) in zip(d["first"], d["second"], d["family"], d["exact"]):
        if fam == -1:
            want = [w for row, length, w in X.EXPLICIT if float(b[3]) == length][0]
            assert abs(e_bev - want) <= 1e-7
    assert sorted(set(d["family"].tolist())) == list(range(-1, 12)) and (np.bincount(d["family"] + 1)[1:] == PER_FAMILY + 64).all()
    e = d["exact"][:, 0]
    for k, name in enumerate(X.FAMILIES):                                 # the closed forms of the families, to fp32 rounding of the parameters
        v = e[d["family"] == k]
        if name in ("length_scaled", "width_scaled", "axis_aligned_length_scaled"):
            assert all(min(abs(x - f) for f in X.FACTORS) <= 1e-6 for x in v)
        elif name in ("shifted_along", "shifted_across"):
            assert all(min(abs(x - (1 - f) / (1 + f)) for f in X.FACTORS) <= 1e-4 for x in v)
        elif name in ("end_to_end", "side_by_side"):
            assert (v <= 1e-4).all()
        elif name in ("one_ulp", "turned_half", "yaw_one_ulp"):
            assert (v >= 1.0 - 1e-4).all()
        elif name == "turned_quarter":
            assert (v > 0.0).all() and (v < 1.0).all()
        else:
            assert (v < 1.0).all() and (v > 0.0).sum() >= len(v) // 2


# ------------------------------------------------------------------ every host statement against the reference
def test_bev_iou_equals_exact():
    d = data()
    got = [pkg("evalrank").bev_iou(a.astype(np.float64), b.astype(np.float64)) for a, b in zip(d["first"], d["second"])]
    compare("evalrank.bev_iou", got, d["exact"][:, 0], d["family"])
    back = [pkg("evalrank").bev_iou(b.astype(np.float64), a.astype(np.float64)) for a, b in zip(d["first"], d["second"])]
    compare("evalrank.bev_iou, second clipped by first", back, d["exact"][:, 0], d["family"])


def test_iou_pair_equals_exact():
    d = data()
    got = np.array([pkg("evalkitti").iou_pair(a, b) for a, b in zip(d["first"], d["second"])])
    compare("evalkitti.iou_pair bev", got[:, 0], d["exact"][:, 0], d["family"])
    compare("evalkitti.iou_pair 3d", got[:, 1], d["exact"][:, 1], d["family"])


def test_rotated_iou_equals_exact():
    d, EG = data(), pkg("evalgeom")
    got, want = [], []
    for a, b in zip(X.footprint_rows(d["first"]).astype(np.float64), X.footprint_rows(d["second"]).astype(np.float64)):
        c1, c2 = EG.box_corners(a[:3], a[3:6], a[6]), EG.box_corners(b[:3], b[3:6], b[6])
        with np.errstate(invalid="ignore", divide="ignore"):
            got.append(EG.rotated_iou(c1, c2))
        want.append(X.exact_rotated(c1, c2))
    got, want = np.array(got, np.float64), np.array(want, np.float64)
    assert np.abs(want[:, 1] - d["exact"][:, 0]).max() <= 1e-12           # the same rectangles as in (x, y), up to the rounding of their corners
    compare("evalgeom.rotated_iou bev", got[:, 1], want[:, 1], d["family"])
    compare("evalgeom.rotated_iou 3d", got[:, 0], want[:, 0], d["family"])


def test_anchor_iou_equals_exact():
    """Anchor 0 of cell i is the first box of pair i, anchor 1 its second box; the labels are the second box and the first."""
    d, A = data(), pkg("assign")
    got, want = np.zeros((len(d["first"]), 4)), np.zeros((len(d["first"]), 4))
    for p, (a, b) in enumerate(zip(d["first"], d["second"])):
        anchors = np.stack([a, b]).reshape(2, 7, 1)
        got[p] = A.anchor_iou(anchors, np.stack([b, a])).reshape(-1)      # (a, b), (a, a), (b, b), (b, a)
        assert np.array_equal(got[p], A.anchor_iou(anchors, np.stack([b, a]), prune=False).reshape(-1), equal_nan=True)
        want[p] = (d["exact"][p, 0], 1.0, 1.0, d["exact"][p, 0])
    for col, name in enumerate(("anchor on first, label on second", "a box with itself (first)", "a box with itself (second)", "anchor on second, label on first")):
        compare("assign.anchor_iou, " + name, got[:, col], want[:, col], d["family"])
    assert np.abs(got[:, 1:3] - 1.0).max() <= 1e-11                       # a box with itself: the shoelace's own rounding only


def test_host_clip_stays_within_the_device_vertex_budget():
    """ev_clip (csrc/ev_geom.h) keeps 12 vertices per polygon buffer: over every family, in both roles, no pass of the host statement -- the
    same decisions -- holds more; after the last pass a convex intersection of two quadrilaterals has at most 8."""
    d, EG = data(), pkg("evalgeom")
    worst, worst_final = 0, 0
    for r1, r2 in d["rect"]:
        for s, c in ((r1, r2), (r2, r1)):
            counts = []
            out = EG._clip_convex(np.array(s), np.array(c), counts=counts)
            assert len(counts) <= 4 and (not counts or counts[-1] == len(out))
            worst, worst_final = max([worst] + counts), max(worst_final, len(out))
    print("most vertices in a pass %d, after the last pass %d" % (worst, worst_final))
    assert worst <= 12 and worst_final <= 8


def test_zero_area_pair_is_nan_and_zero_area_box_is_zero():
    ER, EK, EG, A = pkg("evalrank"), pkg("evalkitti"), pkg("evalgeom"), pkg("assign")
    z = np.array([3.0, -2.0, -1.0, 0.0, 0.0, 1.5, 0.7])
    line = np.array([3.0, -2.0, -1.0, 4.0, 0.0, 1.5, 0.7])
    full = np.array([3.0, -2.0, -1.0, 4.0, 2.0, 1.5, 0.7])
    for a, b in ((z, z), (line, line), (z, line)):
        assert math.isnan(ER.bev_iou(a, b)) and all(math.isnan(v) for v in EK.iou_pair(a, b))
        assert math.isnan(X.exact_bev(X.rect_of(a), X.rect_of(b)))
        assert all(math.isnan(v) for v in X.exact_rotated(EG.box_corners(a[:3], a[3:6], a[6]), EG.box_corners(b[:3], b[3:6], b[6])))
    for a in (z, line):
        assert ER.bev_iou(a, full) == 0.0 and ER.bev_iou(full, a) == 0.0 and EK.iou_pair(a, full) == (0.0, 0.0)
        assert X.exact_bev(X.rect_of(a), X.rect_of(full)) == 0.0
    assert ER.bev_iou(full, full) == 1.0 and EK.iou_pair(full, full) == (1.0, 1.0)
    assert A.anchor_iou(np.stack([full, z]).reshape(2, 7, 1).astype(np.float32), np.stack([z, full]).astype(np.float32)).tolist() == [[0.0, 1.0], [0.0, 0.0]]   # a void label is 0

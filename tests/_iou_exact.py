"""An exact statement of rotated-box IoU, independent of the project's clip, and the box pairs at which a floating-point clip goes wrong
(test infrastructure of tests/test_iou_exact_host.py and tests/test_gpu_iou_exact.py).

The reference is rational arithmetic (fractions.Fraction) on the fp64 corners it is handed: every double is a rational number, the
crossing point of two lines through rational points is rational, and so is a shoelace area, so nothing here rounds before the final
float().  It shares no code with evalgeom / evalrank / evalkitti / assign: closed half-planes instead of the strict ones, either
orientation of both quadrilaterals, crossing points from the two side values.

The families are the pairs of rectangles of which one edge lies on the line of an edge of the other up to rounding -- concentric boxes
of one heading, copies one ulp apart, boxes shifted along or across their heading -- plus the ones that merely look similar and a
generic family.  Parameters are fp32 (what the device reads); factors are 0.3 / 0.6 / 0.9, so that no IoU sits on 0.5 or 0.7.
"""
import math
from fractions import Fraction

import numpy as np

from _util import pkg

NAN = float("nan")


# ------------------------------------------------------------------ the exact reference
def _rational(poly):
    """Counter-clockwise list of exact (x, y) of a polygon given as floats in either orientation."""
    pts = [(Fraction(float(p[0])), Fraction(float(p[1]))) for p in poly]
    return pts if _twice_area(pts) >= 0 else pts[::-1]


def _twice_area(pts):
    """Signed: positive for a counter-clockwise polygon."""
    total = Fraction(0)
    for i, (x, y) in enumerate(pts):
        nx, ny = pts[(i + 1) % len(pts)]
        total += x * ny - nx * y
    return total


def _intersect(subject, clip):
    """subject cut by the closed half-planes left of each edge of the counter-clockwise convex polygon clip."""
    out = list(subject)
    for i in range(len(clip)):
        if not out:
            break
        (ax, ay), (bx, by) = clip[i], clip[(i + 1) % len(clip)]
        side = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for px, py in out]
        cut = []
        for j, p in enumerate(out):
            q, sq, sp = out[j - 1], side[j - 1], side[j]
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):                # a proper crossing: the point at which the side value is 0
                t = sq / (sq - sp)
                cut.append((q[0] + t * (p[0] - q[0]), q[1] + t * (p[1] - q[1])))
            if sp >= 0:
                cut.append(p)
        out = cut
    return out


def exact_areas(quad1, quad2):
    """(intersection area, area of quad1, area of quad2) as Fractions, of two convex polygons given by fp64 corners."""
    p1, p2 = _rational(quad1), _rational(quad2)
    inter = _intersect(p1, p2)
    ia = _twice_area(inter) / 2 if len(inter) >= 3 else Fraction(0)
    return ia, _twice_area(p1) / 2, _twice_area(p2) / 2


def _ratio(num, den):
    return float(num / den) if den != 0 else NAN


def exact_bev(quad1, quad2):
    """Bird's-eye IoU as a float; NaN when a1 + a2 - ia == 0 (a zero-area pair)."""
    ia, a1, a2 = exact_areas(quad1, quad2)
    return _ratio(ia, a1 + a2 - ia)


def exact_kitti(quad1, z1, h1, quad2, z2, h2):
    """(bird's-eye IoU, 3-D IoU) as evalkitti.iou_pair defines them: exact areas, the fp64 overlap of the z extents [z - h/2, z + h/2],
    volumes a h."""
    ia, a1, a2 = exact_areas(quad1, quad2)
    z1, h1, z2, h2 = float(z1), float(h1), float(z2), float(h2)
    zov = max(0.0, min(z1 + h1 / 2, z2 + h2 / 2) - max(z1 - h1 / 2, z2 - h2 / 2))
    iv = ia * Fraction(zov)
    return _ratio(ia, a1 + a2 - ia), _ratio(iv, a1 * Fraction(h1) + a2 * Fraction(h2) - iv)


def exact_rotated(corners1, corners2):
    """(3-D IoU, bird's-eye IoU) as evalgeom.rotated_iou defines them on two (8,3) corner arrays: footprints (x, z) of corners 0-3
    exactly, the fp64 overlap of the y extents (corner 0 above, corner 4 below), fp64 volumes from three edge lengths."""
    c1, c2 = np.asarray(corners1, np.float64), np.asarray(corners2, np.float64)
    ia, a1, a2 = exact_areas([(c1[i, 0], c1[i, 2]) for i in range(4)], [(c2[i, 0], c2[i, 2]) for i in range(4)])
    iv = ia * Fraction(max(0.0, min(float(c1[0, 1]), float(c2[0, 1])) - max(float(c1[4, 1]), float(c2[4, 1]))))

    def edge(c, i, j):
        return math.sqrt(sum((float(c[i, k]) - float(c[j, k])) ** 2 for k in range(3)))

    v1, v2 = (edge(c, 0, 1) * edge(c, 1, 2) * edge(c, 0, 4) for c in (c1, c2))
    return _ratio(iv, Fraction(v1) + Fraction(v2) - iv), _ratio(ia, a1 + a2 - ia)


def apart(b1, b2):
    """True when the two rectangles are certainly disjoint (centres further apart than the half-diagonals together, with 1e-3 to spare
    against 1e-14 of rounding) and not both of zero area: the exact IoU is then 0 and the rational clip can be skipped."""
    d = math.hypot(float(b1[0]) - float(b2[0]), float(b1[1]) - float(b2[1]))
    r = 0.5 * (math.hypot(float(b1[3]), float(b1[4])) + math.hypot(float(b2[3]), float(b2[4])))
    return d > r + 1e-3 and (float(b1[3]) * float(b1[4]) != 0.0 or float(b2[3]) * float(b2[4]) != 0.0)


def rect_of(box):
    """The host's fp64 rectangle of a box row (x, y, z, l, w, h, yaw): the corners every IoU here starts from."""
    b = np.asarray(box, np.float64)
    return pkg("evalgeom").bev_rect(b[:2], b[3:5], b[6])


def exact_matrices(rows1, rows2):
    """(bev [n, m], 3d [n, m]) float64 of exact_kitti for every row of rows1 against every row of rows2."""
    r1, r2 = [rect_of(b) for b in rows1], [rect_of(b) for b in rows2]
    bev, i3d = np.zeros((len(rows1), len(rows2))), np.zeros((len(rows1), len(rows2)))
    for i, a in enumerate(rows1):
        for j, b in enumerate(rows2):
            if not apart(a, b):
                bev[i, j], i3d[i, j] = exact_kitti(r1[i], a[2], a[5], r2[j], b[2], b[5])
    return bev, i3d


# ------------------------------------------------------------------ the families
FAMILIES = ("length_scaled", "width_scaled", "one_ulp", "axis_aligned_length_scaled", "shifted_along", "shifted_across", "end_to_end",
            "side_by_side", "turned_quarter", "turned_half", "yaw_one_ulp", "generic")
FACTORS = (0.3, 0.6, 0.9)
EXPLICIT = (([0.8470991253852844, -1.359326958656311, 0.0, 4.766824722290039, 1.5237280130386353, 1.5, 2.401460886001587], 1.1917061805725098, 0.25),
            ([20.711071014404297, -1.3733352422714233, 0.0, 4.767300128936768, 1.3119361400604248, 1.5, 0.5846763849258423], 2.383650064468384, 0.5))
SPACING = 20.0          # grid pitch of spaced_centres: a pair reaches at most l + half a diagonal = 7.92 from its first centre


def _pick(u, choices):
    return choices[min(int(float(u) * len(choices)), len(choices) - 1)]


def _ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def spaced_centres(count, seed):
    """fp32 [count, 2]: jittered points of a square grid of pitch SPACING about the origin, at odd multiples of SPACING / 2 so that none
    lies on the two explicit pairs (which keep their own centres, near (0.8, -1.4) and (20.7, -1.4))."""
    cols = max(1, int(math.ceil(math.sqrt(count))))
    jitter = pkg("detfill").uniform((count, 2), seed, 0.0, 1.0).astype(np.float64)
    i = np.arange(count)
    grid = np.stack([i % cols - cols // 2, i // cols - cols // 2], 1) * SPACING + SPACING / 2
    return (grid + jitter).astype(np.float32)


def family_pairs(per_family, seed, centres=None):
    """(first [P, 7], second [P, 7], family [P]) fp32 box rows (x, y, z, l, w, h, yaw) and the index into FAMILIES (-1: an explicit pair),
    P = 12 per_family + 2.  Pair p < 12 per_family belongs to family p % 12; the two explicit pairs come last.  Centres are uniform in
    [0, 70] x [-40, 40] unless fp32 `centres` [12 per_family, 2] are given; l in [1, 5], w in [1, 3], any yaw, z in [-1.2, -0.8], h in
    [1.4, 1.8].  The second box's z and h differ from the first's except in the two one-ulp families, whose pairs are duplicates in 3-D too."""
    n = 12 * per_family
    u = pkg("detfill").uniform((n, 16), seed, 0.0, 1.0).astype(np.float64)
    first, second = np.zeros((n + 2, 7), np.float32), np.zeros((n + 2, 7), np.float32)
    family = np.full((n + 2,), -1, np.int64)
    quarter = [np.float32(0.0), np.float32(math.pi / 2), np.float32(-math.pi / 2), np.float32(math.pi)]
    for p in range(n):
        name = FAMILIES[p % 12]
        family[p] = p % 12
        a = np.array([70.0 * u[p, 0], -40.0 + 80.0 * u[p, 1], -1.2 + 0.4 * u[p, 2], 1.0 + 4.0 * u[p, 3], 1.0 + 2.0 * u[p, 4], 1.4 + 0.4 * u[p, 5],
                      math.pi * (2.0 * u[p, 6] - 1.0)], np.float64).astype(np.float32)
        if centres is not None:
            a[:2] = centres[p]
        if name == "axis_aligned_length_scaled":
            a[6] = _pick(u[p, 7], quarter)
        f = _pick(u[p, 8], FACTORS)
        x, y, z, l, w, h, yaw = (float(v) for v in a)                    # fp64 arithmetic on the fp32 values, rounded to fp32 once
        b = a.astype(np.float64)
        b[2], b[5] = z + (0.6 * u[p, 9] - 0.3) * h, h * (0.7 + 0.3 * u[p, 10])
        if name in ("length_scaled", "axis_aligned_length_scaled"):
            b[3] = l * f
        elif name == "width_scaled":
            b[4] = w * f
        elif name in ("shifted_along", "end_to_end"):
            s = l * (f if name == "shifted_along" else 1.0)
            b[0], b[1] = x + s * math.cos(yaw), y + s * math.sin(yaw)
        elif name in ("shifted_across", "side_by_side"):
            s = w * (f if name == "shifted_across" else 1.0)
            b[0], b[1] = x - s * math.sin(yaw), y + s * math.cos(yaw)
        elif name in ("turned_quarter", "turned_half"):
            b[6] = yaw + (1.0 if u[p, 7] < 0.5 else -1.0) * (math.pi / 2 if name == "turned_quarter" else math.pi)
        elif name == "generic":
            b[0], b[1] = x + 4.0 * u[p, 11] - 2.0, y + 4.0 * u[p, 12] - 2.0
            b[3], b[4], b[6] = 1.0 + 4.0 * u[p, 13], 1.0 + 2.0 * u[p, 14], math.pi * (2.0 * u[p, 15] - 1.0)
        b = b.astype(np.float32)
        if name == "one_ulp":
            b = a.copy()
            k = _pick(u[p, 7], (0, 1, 3, 4))
            b[k] = _ulp(a[k], u[p, 11] < 0.5)
        elif name == "yaw_one_ulp":
            b = a.copy()
            b[6] = _ulp(a[6], u[p, 11] < 0.5)
        first[p], second[p] = a, b
    for e, (row, length, _) in enumerate(EXPLICIT):
        first[n + e] = np.array(row, np.float64).astype(np.float32)
        second[n + e] = first[n + e]
        second[n + e, 3] = np.float32(length)
        assert [float(v) for v in first[n + e]] == row and float(second[n + e, 3]) == length, "the explicit pairs are fp32 values"
    return first, second, family


def spaced_case(per_family=64, seed=9102):
    """(first, second, family, samples) for tests in which the pairs of a sample must not interact: family_pairs on one grid per sample.
    samples = index arrays; the first holds 13 pairs (one of each family and the first explicit pair), the others up to 150 (300 rows),
    the last one also the second explicit pair.  Corners stay below 150 in magnitude."""
    n = 12 * per_family
    samples = [list(range(12))] + [list(range(s, min(s + 150, n))) for s in range(12, n, 150)]
    centres = np.zeros((n, 2), np.float32)
    for k, idx in enumerate(samples):
        centres[idx] = spaced_centres(len(idx), seed + 1 + k)
    samples[0].append(n)
    samples[-1].append(n + 1)
    first, second, family = family_pairs(per_family, seed, centres)
    return first, second, family, [np.array(idx) for idx in samples]


def footprint_rows(rows):
    """The rows whose evalgeom.box_corners footprint in (x, z) is the rectangle `rows` have in (x, y): y and z exchanged, yaw negated
    (box_corners turns about the y axis, the other way round).  Exact in fp32."""
    out = np.array(rows, np.float32)[:, [0, 2, 1, 3, 4, 5, 6]]
    out[:, 6] = -out[:, 6]
    return np.ascontiguousarray(out)


def away_from(values, thresholds, margin=1e-6):
    """True when every finite value is at least `margin` from every threshold."""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    return all(float(np.abs(v - t).min()) >= margin for t in thresholds) if len(v) else True

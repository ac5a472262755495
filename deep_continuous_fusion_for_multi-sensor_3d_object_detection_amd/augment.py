"""Train-time BEV augmentation: the transform and its host statement.

Per frame  A = s * R(theta) * F:  F = diag(1, f, 1) (f = -1: the frame is flipped, y -> -y), R(theta) a rotation about z
through the sensor origin, s a scale of all three coordinates.  theta, s, cos and sin are float64 on the host; the five numbers
the device needs are rounded ONCE to fp32 and are the transform from then on:

    a00 = s cos(theta)   a01 = -s sin(theta) f   a10 = s sin(theta)   a11 = s cos(theta) f   a22 = s

Everything else -- the projection matrix that keeps an augmented point on the pixel of its original (compose_crt), the labels
(transform_boxes) -- is derived from those fp32 values, i.e. from what csrc/geometry.hip's k_augment_points_b really applies.
This block never touches the image: `uv` stays the un-augmented frame's, while the voxel grid, the KNN neighbourhoods, the fusion
MLP's offsets and the labels move together.  (The camera side has a block of its own, augment_image.py, which moves `uv` along
with the image instead; the two compose.)

All numpy, no state: draw() is a pure function of (config, seed, rank, call, frame), in the style of the loss sampler's hash
(loss.py: _mix64 / LossTotal._step_seed), so a resumed or a data-parallel run draws what an uninterrupted one draws, and ranks
draw different values.
"""
import math

import numpy as np

from . import cfgcheck as C

M64 = (1 << 64) - 1
KEYS = ("enabled", "seed", "rotation_deg", "scale", "flip_prob", "point_drop")


def parse_config(config):
    """The `augment` block (config_carla.yaml), validated: None = off (no block, or enabled: false), else {"seed", "rotation_deg",
    "scale": (lo, hi), "flip_prob", "point_drop": (lo, hi)}.  Bad values raise ValueError whether the block is enabled or not --
    augmentation is never switched off quietly."""
    got = C.seeded_block(config, "augment", KEYS)
    if got is None:
        return None
    blk, enabled, seed = got
    rot = C.number("augment.rotation_deg", blk.get("rotation_deg", 0.0))
    if rot < 0.0:
        raise ValueError("augment.rotation_deg: theta ~ U(-r, +r) needs r >= 0 (got %r)" % (rot,))
    scale = C.interval("augment.scale", blk.get("scale", (1.0, 1.0)))
    if scale[0] <= 0.0:
        raise ValueError("augment.scale must be positive (got %r)" % (blk.get("scale"),))
    flip = C.probability("augment.flip_prob", blk.get("flip_prob", 0.0))
    drop = C.interval("augment.point_drop", blk.get("point_drop", (0.0, 0.0)))
    for p in drop:
        C.probability("augment.point_drop", p)
    if not enabled:
        return None
    return {"seed": seed, "rotation_deg": rot, "scale": scale, "flip_prob": flip, "point_drop": drop}


def mix64(z):
    """dcf_mix64 of csrc/dcf_common.h on a Python int or a uint64 array (loss._mix64, the loss sampler's restatement)."""
    from .loss import _mix64
    with np.errstate(over="ignore"):
        if isinstance(z, np.ndarray):
            return _mix64(z)
        return int(_mix64(np.uint64(z & M64)))


def params_from(theta, scale, flip, p=0.0, drop_key=0):
    """The parameter set of one frame from its float64 angle (radians), scale, flip flag and drop probability: the fp32 matrix
    entries are rounded here, once."""
    theta, scale, f = float(theta), float(scale), (-1.0 if flip else 1.0)
    c, s = math.cos(theta), math.sin(theta)
    a = np.array([scale * c, 0.0 - scale * s * f, scale * s, scale * c * f, scale], dtype=np.float64).astype(np.float32)
    return {"theta": theta, "scale": scale, "flip": bool(flip), "p": float(p), "drop_key": int(drop_key) & M64, "a": a}


def identity():
    return params_from(0.0, 1.0, False)


# one hash stream per drawn value
_THETA, _SCALE, _FLIP, _DROP_P, _DROP_KEY = range(5)


def draw(cfg, seed, rank, call, b):
    """Parameters of frame b of the call-th augmented step on `rank`: theta ~ U(-rotation_deg, +rotation_deg), s ~ U(scale),
    flip with probability flip_prob, p ~ U(point_drop), and the 64-bit key of the point-drop hash.  cfg: the dict of
    parse_config (or any dict with those keys)."""
    base = (int(seed) * 0x9E3779B1 + int(call) + int(rank) * 0x85EBCA77C2B2AE63) & M64      # LossTotal._step_seed's formula

    def h(stream):
        return mix64(base ^ mix64((int(b) << 8) | stream))

    def u(stream):                                  # [0, 1): the top 53 bits
        return (h(stream) >> 11) * (1.0 / (1 << 53))

    r = float(cfg.get("rotation_deg", 0.0))
    slo, shi = (float(v) for v in cfg.get("scale", (1.0, 1.0)))
    plo, phi = (float(v) for v in cfg.get("point_drop", (0.0, 0.0)))
    theta = math.radians(-r + 2.0 * r * u(_THETA))
    scale = slo + (shi - slo) * u(_SCALE)
    flip = u(_FLIP) < float(cfg.get("flip_prob", 0.0))
    p = plo + (phi - plo) * u(_DROP_P)
    return params_from(theta, min(max(scale, slo), shi), flip, min(max(p, plo), phi), h(_DROP_KEY))


def matrix5(params):
    """{a00, a01, a10, a11, a22} as fp32 -- the `mat` row of dcf_augment_points_batch."""
    return np.asarray(params["a"], dtype=np.float32).reshape(5)


def matrix3(params):
    """A as a float64 3x3 matrix of the fp32 entries (column-vector convention: p' = A p)."""
    a = matrix5(params).astype(np.float64)
    return np.array([[a[0], a[1], 0.0], [a[2], a[3], 0.0], [0.0, 0.0, a[4]]], dtype=np.float64)


def drop_threshold(params):
    """floor(p * 2^32) as the uint32 the device compares with (p = 1 would need 2^32: capped at 2^32 - 1)."""
    return min(int(math.floor(float(params["p"]) * 4294967296.0)), 0xFFFFFFFF)


def transform_points(pts_f32, params):
    """[n,3] fp32 -> [n,3] fp32, in np.float32 arithmetic, every product and sum rounded, nothing contracted:
    x' = fl(fl(a00 x) + fl(a01 y)),  y' = fl(fl(a10 x) + fl(a11 y)),  z' = fl(a22 z)."""
    p = np.asarray(pts_f32, dtype=np.float32).reshape(-1, 3)
    a = matrix5(params)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    out[:, 0] = (a[0] * x).astype(np.float32) + (a[1] * y).astype(np.float32)
    out[:, 1] = (a[2] * x).astype(np.float32) + (a[3] * y).astype(np.float32)
    out[:, 2] = a[4] * z
    return out


def keep_mask(n, params):
    """bool [n]: point i is DROPPED iff (mix64(drop_key ^ mix64(i)) >> 32) < drop_threshold -- integers only, so the host and
    the device agree exactly.  p = 0 drops nothing."""
    i = np.arange(int(n), dtype=np.uint64)
    hv = mix64(np.uint64(int(params["drop_key"]) & M64) ^ mix64(i)) >> np.uint64(32)
    return ~(hv < np.uint64(drop_threshold(params)))


def compose_crt(crt_4x3, params):
    """The [4,3] matrix that projects an AUGMENTED point to the pixel of its ORIGINAL: [A p, 1] . crt' = [p, 1] . crt, so rows
    0..2 are A^-T . crt[0:3] with A^-1 taken in float64 from the fp32 entries (the inverse of what the device applies); row 3
    is unchanged.  Rounded to fp32.  A flip negates row 1 and a scale by a power of two scales rows 0..2 by its inverse, both
    exactly."""
    crt = np.asarray(crt_4x3, dtype=np.float64).reshape(4, 3)
    a = matrix5(params).astype(np.float64)
    det = a[0] * a[3] - a[1] * a[2]
    inv_t = np.array([[a[3] / det, -a[2] / det, 0.0], [-a[1] / det, a[0] / det, 0.0], [0.0, 0.0, 1.0 / a[4]]], dtype=np.float64)   # (A^-1)^T
    out = crt.copy()
    out[0:3] = inv_t @ crt[0:3]
    return np.ascontiguousarray(out.astype(np.float32))


def box_image(row, params):
    """One label row (x, y, z, l, w, h, yaw, ...) under A, in float64, the yaw NOT yet wrapped.  The fp32 entries are exactly a
    flip followed by a rotation through atan2(a10, a00) and an in-plane scale hypot(a00, a10) (|a00| = |a11| and |a01| = |a10|
    bit for bit), so the footprint rectangle of the result is the image under A of the row's: l and w take the in-plane scale,
    z and h take a22, and a heading (cos yaw, sin yaw) becomes (cos, sin)(theta' - yaw) on a flip, (theta' + yaw) without."""
    a = matrix5(params).astype(np.float64)
    r = np.asarray(row, dtype=np.float64).copy()
    x, y = r[0], r[1]
    r[0] = a[0] * x + a[1] * y
    r[1] = a[2] * x + a[3] * y
    sxy = math.hypot(a[0], a[2])
    r[2] *= a[4]
    r[3] *= sxy
    r[4] *= sxy
    r[5] *= a[4]
    flipped = a[0] * a[3] - a[1] * a[2] < 0.0             # det A = f (a00^2 + a10^2)
    r[6] = (-r[6] if flipped else r[6]) + math.atan2(a[2], a[0])
    return r


def transform_boxes(boxes, num, params, config, dtype=np.float32):
    """Labels of one frame under A: boxes [max_num_bbox, 9] rows (x, y, z, l, w, h, yaw, class, 1), the first `num` valid.
    Centre through A, sizes scaled, yaw mirrored on a flip, turned, and wrapped with the dataset's own orientation_inner_bound
    (box_image); float64 arithmetic, stored as `dtype`.  Rows whose new centre fails the dataset's valid_bbox range test are
    removed, the rest packed to the front in their old order, unused rows zero.  Returns (boxes', num')."""
    from types import SimpleNamespace
    from .data_import_carla import CarlaDataset
    ds = SimpleNamespace(config=config)
    src = np.asarray(boxes)
    out = np.zeros(src.shape, dtype=dtype)
    k = 0
    for i in range(int(num)):
        r = box_image(src[i], params)
        if not CarlaDataset.valid_bbox(ds, r):
            continue
        r[6] = CarlaDataset.orientation_inner_bound(float(r[6]))
        out[k] = r
        k += 1
    return out, k

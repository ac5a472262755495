"""Train-time camera image augmentation: the transform and its host statement.

Geometric part, per frame: an axis-aligned affine of the image plane that keeps the centre,

    u' = su u + tu     v' = sv v + tv        su = f s,  sv = s  (f = -1: horizontal flip)
    tu = W/2 - su W/2 + dx                   tv = H/2 - sv H/2 + dy

Photometric part, per channel c: t = g_c val + bias with g_c = kappa beta gamma_c (contrast, brightness, channel gain) and
bias = 255 * 0.5 * (1 - kappa) (the contrast pivots on mid-grey).  A dropped frame (drop_prob) has g_c = bias = 0: its image is
all zeros, the camera branch sees an uninformative input.

s, f, dx, dy, beta, kappa, gamma_c are float64 on the host; the EIGHT numbers the device needs are computed in float64 and rounded
ONCE to fp32 -- they are the transform from then on, as augment.params_from's five are for the BEV block:

    q = (ku, cu, kv, cv, g_0, g_1, g_2, bias)      ku = 1/su   cu = -tu/su   kv = 1/sv   cv = -tv/sv

i.e. the INVERSE map the gather kernel applies: the output pixel (h, w) reads the source at (kv (h + .5) + cv, ku (w + .5) + cu).
The projection matrix that moves a LiDAR point's pixel along with the image (compose_crt_image) is derived from those fp32 values,
i.e. from what csrc/image_aug.hip's k_augment_image_b really applies.  Labels do not move: they are 3-D boxes in the LiDAR frame.

All numpy, no state: draw() is a pure function of (config, seed, rank, call, frame) built like augment.draw (same `base`, same
mix64 construction) on hash streams 16..25 -- the BEV block owns 0..4 -- so both blocks share the trainer's one counter
`aug_calls`, a checkpoint needs no new field, and the BEV block draws what it drew before this module existed.
"""
import numpy as np

from . import cfgcheck as C
from .augment import M64, mix64

NQ = 8                     # ku cu kv cv g0 g1 g2 bias
# one hash stream per drawn value (augment.py holds 0..4)
_ZOOM, _DX, _DY, _FLIP, _BRIGHT, _CONTRAST, _GAIN0, _GAIN1, _GAIN2, _DROP = range(16, 26)
_STREAMS = np.arange(16, 26, dtype=np.uint64)
KEYS = ("enabled", "seed", "zoom", "shift", "flip_prob", "brightness", "contrast", "channel_gain", "drop_prob")


def _factor_interval(blk, key, least=None):
    """blk[key] (default [1, 1]) as an interval of positive factors, lo >= least where given."""
    lo, hi = C.interval("augment_image." + key, blk.get(key, (1.0, 1.0)))
    if lo <= 0.0 or (least is not None and lo < least):
        raise ValueError("augment_image.%s must be %s (got %r)" % (key, "positive" if least is None else ">= %g" % least, blk.get(key)))
    return lo, hi


def parse_config(config):
    """The `augment_image` block, validated like `augment`: None = off (no block, or enabled: false), else {"seed", "zoom": (lo, hi),
    "shift": (fx, fy), "flip_prob", "brightness": (lo, hi), "contrast": (lo, hi), "channel_gain": (lo, hi), "drop_prob"}.  Bad values
    raise ValueError whether the block is enabled or not.  zoom needs lo >= 0.5: the two-tap bilinear of the kernel covers every
    source pixel only up to a 2x minification (a bound derived from the filter's footprint, not a measured one)."""
    got = C.seeded_block(config, "augment_image", KEYS)
    if got is None:
        return None
    blk, enabled, seed = got
    zoom = _factor_interval(blk, "zoom", least=0.5)
    shift = C.pair("augment_image.shift", blk.get("shift", (0.0, 0.0)))
    if not (0.0 <= shift[0] <= 0.5 and 0.0 <= shift[1] <= 0.5):
        raise ValueError("augment_image.shift: fractions of the width and height in [0, 0.5] (got %r)" % (blk.get("shift"),))
    out = {"seed": seed, "zoom": zoom, "shift": shift, "flip_prob": C.probability("augment_image.flip_prob", blk.get("flip_prob", 0.0)),
           "brightness": _factor_interval(blk, "brightness"), "contrast": _factor_interval(blk, "contrast"),
           "channel_gain": _factor_interval(blk, "channel_gain"), "drop_prob": C.probability("augment_image.drop_prob", blk.get("drop_prob", 0.0))}
    return out if enabled else None


def params_from(width, height, zoom=1.0, flip=False, dx=0.0, dy=0.0, brightness=1.0, contrast=1.0, gain=(1.0, 1.0, 1.0), drop=False):
    """The parameter set of one frame of a [3, height, width] image from its float64 zoom s, flip flag, shift (dx, dy) in pixels and
    photometric factors: the eight fp32 numbers are rounded here, once."""
    W, H, s = float(width), float(height), float(zoom)
    su, sv = (-s if flip else s), s
    tu = W / 2 - su * W / 2 + float(dx)
    tv = H / 2 - sv * H / 2 + float(dy)
    kappa, beta = float(contrast), float(brightness)
    g = [0.0] * 3 if drop else [kappa * beta * float(c) for c in gain]
    bias = 0.0 if drop else 255.0 * 0.5 * (1.0 - kappa)
    q = np.array([1.0 / su, 0.0 - tu / su, 1.0 / sv, 0.0 - tv / sv, g[0], g[1], g[2], bias], dtype=np.float64).astype(np.float32)
    return {"width": int(width), "height": int(height), "zoom": s, "flip": bool(flip), "dx": float(dx), "dy": float(dy),
            "brightness": beta, "contrast": kappa, "gain": tuple(float(c) for c in gain), "drop": bool(drop), "q": q}


def identity(width, height):
    return params_from(width, height)


def draw(cfg, seed, rank, call, b, width, height):
    """Parameters of frame b of the call-th augmented step on `rank` for a [3, height, width] image: s ~ U(zoom),
    dx ~ U(-fx W, fx W), dy ~ U(-fy H, fy H) with (fx, fy) = shift, a flip with probability flip_prob, beta ~ U(brightness),
    kappa ~ U(contrast), gamma_c ~ U(channel_gain) per channel, the frame blacked out with probability drop_prob.  cfg: the dict
    of parse_config (or any dict with those keys)."""
    base = (int(seed) * 0x9E3779B1 + int(call) + int(rank) * 0x85EBCA77C2B2AE63) & M64      # augment.draw's formula

    # the ten streams in one vectorised hash (the values of augment.draw's h(stream), two numpy calls instead of twenty)
    with np.errstate(over="ignore"):
        hv = mix64(np.uint64(base) ^ mix64(np.uint64((int(b) << 8) & M64) | _STREAMS))
    uni = (hv >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))       # [0, 1): the top 53 bits, exactly

    def u(stream):
        return float(uni[stream - _ZOOM])

    def within(key, stream, default=(1.0, 1.0)):
        lo, hi = (float(v) for v in cfg.get(key, default))
        return min(max(lo + (hi - lo) * u(stream), lo), hi)

    fx, fy = (float(v) for v in cfg.get("shift", (0.0, 0.0)))
    return params_from(width, height, zoom=within("zoom", _ZOOM), flip=u(_FLIP) < float(cfg.get("flip_prob", 0.0)),
                       dx=fx * float(width) * (2.0 * u(_DX) - 1.0), dy=fy * float(height) * (2.0 * u(_DY) - 1.0),
                       brightness=within("brightness", _BRIGHT), contrast=within("contrast", _CONTRAST),
                       gain=(within("channel_gain", _GAIN0), within("channel_gain", _GAIN1), within("channel_gain", _GAIN2)),
                       drop=u(_DROP) < float(cfg.get("drop_prob", 0.0)))


def vector8(params):
    """(ku, cu, kv, cv, g0, g1, g2, bias) as fp32 -- one `q` row of dcf_augment_image_batch."""
    return np.asarray(params["q"], dtype=np.float32).reshape(NQ)


def _taps(k, c, n):
    """Source coordinate of the n output positions of one axis: (i0, frac) with fx = fl(fl(fl(k (i + .5)) + c) - .5) in np.float32,
    i0 = floor(fx) as int64, frac = fl(fx - i0) (a rounded difference like the others: a tiny negative fx gives frac = 1)."""
    half = np.float32(0.5)
    pos = np.arange(n, dtype=np.float32) + half                  # exact below 2^23
    fx = ((k * pos).astype(np.float32) + c).astype(np.float32) - half
    f0 = np.floor(fx)
    return f0.astype(np.int64), (fx - f0).astype(np.float32)


def resample(img_u8, params):
    """The value of transform_image before its photometric part: fp32 [3,H,W], two-tap bilinear per axis, taps outside the image
    contribute 0 (grid_sample's padding_mode="zeros", align_corners=False)."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] != 3:
        raise ValueError("image must be uint8 [3,H,W] (got %s %s)" % (img.dtype, img.shape))
    _, H, W = img.shape
    q = vector8(params)
    x0, wx = _taps(q[0], q[1], W)
    y0, wy = _taps(q[2], q[3], H)
    one = np.float32(1.0)

    def gather(yy, xx):                             # [3,H,W] fp32, 0 outside
        ok = ((yy >= 0) & (yy <= H - 1))[:, None] & ((xx >= 0) & (xx <= W - 1))[None, :]
        v = img[:, np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]].astype(np.float32)
        return v * ok.astype(np.float32)[None]

    ax, bx = (one - wx)[None, None, :], wx[None, None, :]
    ay, by = (one - wy)[None, :, None], wy[None, :, None]
    top = (gather(y0, x0) * ax).astype(np.float32) + (gather(y0, x0 + 1) * bx).astype(np.float32)
    bot = (gather(y0 + 1, x0) * ax).astype(np.float32) + (gather(y0 + 1, x0 + 1) * bx).astype(np.float32)
    return ((top * ay).astype(np.float32) + (bot * by).astype(np.float32)).astype(np.float32)


def quantise(t_f32):
    """clamp(rint(t), 0, 255) as uint8, round-half-to-even (np.rint)."""
    return np.clip(np.rint(np.asarray(t_f32, dtype=np.float32)), 0.0, 255.0).astype(np.uint8)


def transform_image(img_u8, params):
    """uint8 [3,H,W] -> uint8 [3,H,W]: the host statement of k_augment_image_b, bit for bit.  All arithmetic in np.float32, every
    product and sum rounded, nothing contracted.  For the output pixel (h, w):

        fx = fl(fl(fl(ku (w + .5)) + cu) - .5)    x0 = floor(fx)   wx = fl(fx - x0)          (fy, y0, wy from h, kv, cv)
        top = fl(fl(p00 fl(1 - wx)) + fl(p01 wx))     bot likewise from the row below
        val = fl(fl(top fl(1 - wy)) + fl(bot wy))     t = fl(fl(g_c val) + bias)     out = clamp(rint(t), 0, 255), half to even

    A tap whose column is outside [0, W-1] or whose row is outside [0, H-1] contributes 0.  A two-tap bilinear covers every source
    pixel only up to a 2x minification (|ku|, |kv| <= 2): hence the config's zoom >= 0.5 -- a bound derived from the footprint of
    the filter, not a measured one.

    Exact cases (every intermediate is representable, so nothing rounds and the output is the input rearranged):
    * identity (ku = 1, cu = 0): w + .5 is a half-integer below 2^23, fx = w, wx = 0, top = p00 * 1 + p01 * 0.
    * a pure flip (ku = -1, cu = W): -(w + .5) + W = W - w - .5 is again a half-integer below 2^23, fx = W - 1 - w, wx = 0.
    * an integer shift (ku = 1, cu = -d): w + .5 - d is a half-integer, fx = w - d, wx = 0; columns read outside are zero.
    * ku = .5: .5 (w + .5) = w/2 + .25 needs two more fraction bits than w (exact below 2^21), fx = w/2 - .25, so wx is .75
      (w even) or .25 (w odd); a byte times a multiple of 1/4 has 10 significant bits, and the sums of such terms, with the
      second axis (multiples of 1/16), stay far inside 24 bits."""
    q = vector8(params)
    val = resample(img_u8, params)
    t = (q[4:7].reshape(3, 1, 1) * val).astype(np.float32) + q[7]
    return quantise(t)


def affine(params):
    """(su, tu, sv, tv) in float64 from the fp32 numbers the device applies: su = 1/ku, tu = -cu/ku, likewise v."""
    q = vector8(params).astype(np.float64)
    return 1.0 / q[0], 0.0 - q[1] / q[0], 1.0 / q[2], 0.0 - q[3] / q[2]


def compose_crt_image(crt_4x3, params):
    """The [4,3] matrix that projects a point to the pixel its original pixel moved to: [p, 1] . crt = (a0, a1, a2) with u = a0 / a2,
    so u' = su u + tu = (su a0 + tu a2) / a2 -- column 0 becomes su col0 + tu col2, column 1 sv col1 + tv col2, column 2 (the
    depth) is unchanged.  (su, tu, sv, tv) = affine(params), float64 from the fp32 values the kernel applies; rounded to fp32.
    Composes with augment.compose_crt in either order (that one acts on rows 0..2, this one on columns 0..1).

    The crop: a point whose new pixel is outside (0, ulim) x (0, vlim) is rejected by the projection kernel's own limit test, as
    it is.  A point that lands on the zero padding of a zoomed-out or shifted image stays and samples the padding's features --
    there is no second limit test."""
    crt = np.asarray(crt_4x3, dtype=np.float64).reshape(4, 3)
    su, tu, sv, tv = affine(params)
    out = crt.copy()
    out[:, 0] = su * crt[:, 0] + tu * crt[:, 2]
    out[:, 1] = sv * crt[:, 1] + tv * crt[:, 2]
    return np.ascontiguousarray(out.astype(np.float32))

"""Train-time camera image augmentation without a GPU (augment_image.py, train.parse_image_augment_config):
the config block, the stateless draw, the fp32 host statement of the gather kernel with its exact cases, an independent pin against
grid_sample, the projection matrix that moves a point's pixel along with the image, and the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

from _util import M64, ROOT, mix64, pkg

FULL = {"zoom": (0.6, 1.5), "shift": (0.1, 0.2), "flip_prob": 0.5, "brightness": (0.8, 1.2), "contrast": (0.7, 1.3), "channel_gain": (0.9, 1.1),
        "drop_prob": 0.25}
GOOD = {"enabled": True, "seed": 4, "zoom": [0.8, 1.25], "shift": [0.1, 0.05], "flip_prob": 0.5, "brightness": [0.8, 1.2], "contrast": [0.8, 1.2],
        "channel_gain": [0.95, 1.05], "drop_prob": 0.1}
EPS = 2.0 ** -24                       # half an ulp of fp32, relative


def _image(h, w, seed):
    return pkg("detfill").uniform((3, h, w), 4100 + seed, 0.0, 256.0).astype(np.uint8)


def _raw(ku=1.0, cu=0.0, kv=1.0, cv=0.0, g=(1.0, 1.0, 1.0), bias=0.0):
    return {"q": np.array([ku, cu, kv, cv, g[0], g[1], g[2], bias], dtype=np.float32)}


# ------------------------------------------------------------------------------------------------ config
def test_parse_off_by_default():
    parse = pkg("train").parse_image_augment_config
    assert parse({}) is None
    assert parse({"augment_image": None}) is None
    assert parse({"augment_image": {"enabled": False, "zoom": [0.8, 1.2]}}) is None
    assert parse({"augment_image": dict(GOOD, enabled=False)}) is None
    assert parse({"augment_image": dict(GOOD)}) == {"seed": 4, "zoom": (0.8, 1.25), "shift": (0.1, 0.05), "flip_prob": 0.5, "brightness": (0.8, 1.2),
                                                    "contrast": (0.8, 1.2), "channel_gain": (0.95, 1.05), "drop_prob": 0.1}
    assert parse({"augment_image": {"enabled": True}}) == {"seed": 0, "zoom": (1.0, 1.0), "shift": (0.0, 0.0), "flip_prob": 0.0, "brightness": (1.0, 1.0),
                                                           "contrast": (1.0, 1.0), "channel_gain": (1.0, 1.0), "drop_prob": 0.0}
    # a block of its own: the BEV block's parser neither sees it nor changes
    assert pkg("train").parse_augment_config({"augment_image": dict(GOOD)}) is None


BAD = [{"enabled": "yes"}, {"enabled": 1}, {"seed": 1.5}, {"seed": True}, {"seed": "3"}, {"zom": [1.0, 1.0]}, {"rotation_deg": 10.0}]
for _key in ("zoom", "brightness", "contrast", "channel_gain"):
    BAD += [{_key: [1.1, 0.9]}, {_key: [0.0, 1.0]}, {_key: [-1.0, 1.0]}, {_key: 1.0}, {_key: [1.0]}, {_key: [1.0, 1.0, 1.0]}, {_key: [1.0, float("inf")]},
            {_key: [float("nan"), 1.0]}, {_key: ["a", 1.0]}, {_key: [True, 1.0]}]
BAD += [{"zoom": [0.49, 1.0]}, {"zoom": [0.25, 0.4]}]
BAD += [{"shift": [0.6, 0.0]}, {"shift": [0.0, 0.51]}, {"shift": [-0.1, 0.0]}, {"shift": 0.1}, {"shift": [0.1]}, {"shift": [float("nan"), 0.0]}, {"shift": ["a", 0.0]}]
for _key in ("flip_prob", "drop_prob"):
    BAD += [{_key: 1.5}, {_key: -0.1}, {_key: float("nan")}, {_key: "half"}, {_key: True}, {_key: [0.5, 0.5]}]


@pytest.mark.parametrize("enabled", [True, False])
@pytest.mark.parametrize("bad", BAD, ids=lambda b: "%s=%r" % next(iter(b.items())))
def test_parse_rejects_bad_values(bad, enabled):
    parse = pkg("train").parse_image_augment_config
    blk = {"enabled": enabled}
    blk.update(bad)
    with pytest.raises(ValueError):
        parse({"augment_image": blk})


def test_parse_rejects_a_non_mapping_and_accepts_the_zoom_bound():
    parse = pkg("train").parse_image_augment_config
    with pytest.raises(ValueError):
        parse({"augment_image": True})
    assert parse({"augment_image": {"enabled": True, "zoom": [0.5, 2.0]}})["zoom"] == (0.5, 2.0)


# ------------------------------------------------------------------------------------------------ draw
def test_draw_is_a_pure_function_of_its_arguments():
    AI = pkg("augment_image")
    base = AI.draw(FULL, 3, 1, 7, 2, 1242, 375)
    again = AI.draw(dict(FULL), 3, 1, 7, 2, 1242, 375)
    assert np.array_equal(base["q"], again["q"]) and {k: v for k, v in base.items() if k != "q"} == {k: v for k, v in again.items() if k != "q"}
    assert base["q"].dtype == np.float32 and base["q"].shape == (8,)
    for other in ((4, 1, 7, 2), (3, 0, 7, 2), (3, 1, 8, 2), (3, 1, 7, 3)):
        q = AI.draw(FULL, *other, 1242, 375)
        for key in ("zoom", "dx", "dy", "brightness", "contrast", "gain"):
            assert q[key] != base[key], (other, key)


def test_draw_stays_inside_the_configured_ranges_and_fills_them():
    AI = pkg("augment_image")
    W, H = 1242, 375
    rows = [AI.draw(FULL, 11, i % 4, i // 8, i % 8, W, H) for i in range(10000)]
    z = np.array([r["zoom"] for r in rows]); dx = np.array([r["dx"] for r in rows]); dy = np.array([r["dy"] for r in rows])
    be = np.array([r["brightness"] for r in rows]); ka = np.array([r["contrast"] for r in rows]); ga = np.array([r["gain"] for r in rows])
    assert z.min() >= 0.6 and z.max() <= 1.5 and np.abs(dx).max() <= 0.1 * W and np.abs(dy).max() <= 0.2 * H
    assert be.min() >= 0.8 and be.max() <= 1.2 and ka.min() >= 0.7 and ka.max() <= 1.3 and ga.min() >= 0.9 and ga.max() <= 1.1
    # 10 000 uniform draws leave a gap of more than 1 % of the range at an end with probability 2e-44
    assert z.min() < 0.609 and z.max() > 1.491 and dx.min() < -0.098 * W and dx.max() > 0.098 * W and dy.min() < -0.196 * H and dy.max() > 0.196 * H
    assert ga.shape == (10000, 3) and (ga.min(0) < 0.902).all() and (ga.max(0) > 1.098).all()
    assert np.abs(np.corrcoef(ga.T) - np.eye(3)).max() < 0.05            # the channels draw on their own (10 000 pairs: 5 sigma)
    assert 0.45 < np.mean([r["flip"] for r in rows]) < 0.55              # 10 000 fair coins: 10 sigma
    assert 0.22 < np.mean([r["drop"] for r in rows]) < 0.28              # p = 0.25: 7 sigma
    for r in rows[:500]:                                                 # the eight numbers are the documented formulas, rounded once
        s, f = r["zoom"], (-1.0 if r["flip"] else 1.0)
        su, sv = f * s, s
        tu, tv = W / 2 - su * W / 2 + r["dx"], H / 2 - sv * H / 2 + r["dy"]
        geo = [1.0 / su, -tu / su, 1.0 / sv, -tv / sv]
        pho = [0.0] * 4 if r["drop"] else [r["contrast"] * r["brightness"] * g for g in r["gain"]] + [255.0 * 0.5 * (1.0 - r["contrast"])]
        assert np.array_equal(r["q"], np.array(geo + pho, dtype=np.float64).astype(np.float32))
    assert not any(AI.draw(dict(FULL, flip_prob=0.0, drop_prob=0.0), 11, 0, i, 0, W, H)[k] for i in range(2000) for k in ("flip", "drop"))
    assert all(AI.draw(dict(FULL, flip_prob=1.0, drop_prob=1.0), 11, 0, i, 0, W, H)[k] for i in range(2000) for k in ("flip", "drop"))


def test_neutral_config_draws_the_identity():
    AI = pkg("augment_image")
    for i in range(50):
        q = AI.draw({}, 5, i % 3, i, i % 4, 1242, 375)
        assert q["q"].tobytes() == np.array([1, 0, 1, 0, 1, 1, 1, 0], dtype=np.float32).tobytes()     # +0.0, not -0.0
    assert AI.identity(7, 5)["q"].tobytes() == np.array([1, 0, 1, 0, 1, 1, 1, 0], dtype=np.float32).tobytes()


def test_the_bev_block_draws_what_it_drew_before_the_image_block_existed():
    """augment.draw restated from the documented construction with the test suite's own mix64: hash streams 0..4 of
    base = seed * 0x9E3779B1 + call + rank * 0x85EBCA77C2B2AE63, 53 bits each.  The image block draws on streams of its own."""
    A, AI = pkg("augment"), pkg("augment_image")
    cfg = {"rotation_deg": 45.0, "scale": (0.9, 1.1), "flip_prob": 0.5, "point_drop": (0.05, 0.3)}
    for seed, rank, call, b in ((3, 1, 7, 2), (0, 0, 0, 0), (11, 3, 12345, 7), (2 ** 40 + 1, 2, 1, 1)):
        base = (seed * 0x9E3779B1 + call + rank * 0x85EBCA77C2B2AE63) & M64

        def h(stream):
            return mix64(base ^ mix64((b << 8) | stream))

        def u(stream):
            return (h(stream) >> 11) * (1.0 / (1 << 53))

        got = A.draw(cfg, seed, rank, call, b)
        assert got["theta"] == math.radians(-45.0 + 90.0 * u(0)) and got["scale"] == min(max(0.9 + (1.1 - 0.9) * u(1), 0.9), 1.1)
        assert got["flip"] == (u(2) < 0.5) and got["p"] == min(max(0.05 + (0.3 - 0.05) * u(3), 0.05), 0.3) and got["drop_key"] == h(4)
        # the image block's zoom is stream 16 of the same base
        zi = AI.draw({"zoom": (0.6, 1.5)}, seed, rank, call, b, 64, 48)["zoom"]
        assert zi == min(max(0.6 + (1.5 - 0.6) * u(16), 0.6), 1.5)
        # ... and every value of the image block is its documented stream, 16..25, of that construction
        q = AI.draw(FULL, seed, rank, call, b, 64, 48)

        def within(lo, hi, stream):
            return min(max(lo + (hi - lo) * u(stream), lo), hi)
        assert q["zoom"] == within(0.6, 1.5, 16) and q["dx"] == 0.1 * 64.0 * (2.0 * u(17) - 1.0) and q["dy"] == 0.2 * 48.0 * (2.0 * u(18) - 1.0)
        assert q["flip"] == (u(19) < 0.5) and q["brightness"] == within(0.8, 1.2, 20) and q["contrast"] == within(0.7, 1.3, 21)
        assert q["gain"] == (within(0.9, 1.1, 22), within(0.9, 1.1, 23), within(0.9, 1.1, 24)) and q["drop"] == (u(25) < 0.25)
    streams = [AI._ZOOM, AI._DX, AI._DY, AI._FLIP, AI._BRIGHT, AI._CONTRAST, AI._GAIN0, AI._GAIN1, AI._GAIN2, AI._DROP]
    assert len(set(streams)) == len(streams) and min(streams) > 4 and max(streams) < 256
    assert (A._THETA, A._SCALE, A._FLIP, A._DROP_P, A._DROP_KEY) == (0, 1, 2, 3, 4)


# ------------------------------------------------------------------------------------------------ the host statement: exact cases
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (37, 131)])
def test_identity_flip_and_integer_shift_are_exact(H, W):
    AI = pkg("augment_image")
    img = _image(H, W, H + W)
    assert np.array_equal(AI.transform_image(img, AI.identity(W, H)), img)
    flip = AI.params_from(W, H, flip=True)
    assert flip["q"][0] == -1.0 and flip["q"][1] == W
    assert np.array_equal(AI.transform_image(img, flip), img[:, :, ::-1])
    if W > 3 and H > 2:
        sh = AI.params_from(W, H, dx=3.0, dy=-2.0)                   # +3 columns, -2 rows
        want = np.zeros_like(img)
        want[:, :H - 2, 3:] = img[:, 2:, :W - 3]
        assert np.array_equal(AI.transform_image(img, sh), want)
        both = AI.params_from(W, H, flip=True, dx=3.0, dy=-2.0)     # flipped, then shifted
        want = np.zeros_like(img)
        want[:, :H - 2, 3:] = img[:, 2:, ::-1][:, :, :W - 3]
        assert np.array_equal(AI.transform_image(img, both), want)


def test_half_rate_sampling_equals_hand_written_averages():
    """ku = .5 (and kv = .5): output column 2j reads .25 p[j-1] + .75 p[j], column 2j+1 reads .75 p[j] + .25 p[j+1] -- every value is a
    multiple of 1/4 (1/16 with both axes), so float64 gives the exact value and np.rint its half-to-even integer."""
    AI = pkg("augment_image")
    H, W = 6, 10
    img = _image(H, W, 1)
    p = np.zeros((3, H + 2, W + 2), dtype=np.float64)
    p[:, 1:-1, 1:-1] = img                                          # p[.., j + 1] = pixel j, zeros around

    def half(a, axis, n):                                           # the n outputs of one axis
        a = np.moveaxis(a, axis, -1)
        out = np.empty(a.shape[:-1] + (n,), dtype=np.float64)
        for i in range(n):
            j = i // 2
            out[..., i] = (0.25 * a[..., j] + 0.75 * a[..., j + 1]) if i % 2 == 0 else (0.75 * a[..., j + 1] + 0.25 * a[..., j + 2])
        return np.moveaxis(out, -1, axis)

    want_x = half(p[:, 1:-1, :], 2, W)
    got = AI.transform_image(img, _raw(ku=0.5))
    assert np.array_equal(got, np.rint(want_x).astype(np.uint8))
    frac = want_x - np.floor(want_x)
    assert (frac == 0.5).any()                                      # the quantiser met ties
    want_xy = half(half(p, 2, W)[:, :, :], 1, H)
    assert np.array_equal(AI.resample(img, _raw(ku=0.5, kv=0.5)).astype(np.float64), want_xy)
    assert np.array_equal(AI.transform_image(img, _raw(ku=0.5, kv=0.5)), np.rint(want_xy).astype(np.uint8))


def test_quantiser_rounds_half_to_even_and_clamps():
    AI = pkg("augment_image")
    t = np.array([0.5, 1.5, 2.5, 3.5, 254.5, 255.5, -0.5, -0.4999, -7.0, 255.49, 300.0, 1e9, -1e9, 0.0], dtype=np.float32)
    assert AI.quantise(t).tolist() == [0, 2, 2, 4, 254, 255, 0, 0, 0, 255, 255, 255, 0, 0]
    img = np.zeros((3, 1, 8), dtype=np.uint8)
    img[:, 0, :] = [1, 3, 5, 7, 200, 255, 0, 128]
    # t = .5 p: .5 1.5 2.5 3.5 -> 0 2 2 4
    assert AI.transform_image(img, _raw(g=(0.5, 0.5, 0.5)))[0, 0].tolist() == [0, 2, 2, 4, 100, 128, 0, 64]
    # per channel: above 255, below 0, in between
    got = AI.transform_image(img, _raw(g=(2.0, 1.0, 1.0), bias=-6.5))
    assert got[0, 0].tolist() == [0, 0, 4, 8, 255, 255, 0, 250]      # 2 p - 6.5: -4.5 -.5 3.5 7.5 393.5 503.5 -6.5 249.5 (ties to even)
    assert got[1, 0].tolist() == [0, 0, 0, 0, 194, 248, 0, 122]      # p - 6.5: -5.5 -3.5 -1.5 .5 193.5 248.5 -6.5 121.5


def test_a_dropped_frame_is_all_zeros():
    AI = pkg("augment_image")
    img = _image(5, 7, 9)
    q = AI.params_from(7, 5, zoom=1.3, dx=0.4, brightness=1.2, contrast=0.8, drop=True)
    assert q["q"][4:].tobytes() == np.zeros(4, np.float32).tobytes()
    assert not AI.transform_image(img, q).any() and img.any()


def test_transform_image_refuses_other_layouts():
    AI = pkg("augment_image")
    with pytest.raises(ValueError):
        AI.transform_image(np.zeros((3, 4, 4), np.float32), AI.identity(4, 4))
    with pytest.raises(ValueError):
        AI.transform_image(np.zeros((4, 4, 3), np.uint8), AI.identity(4, 4))


# ------------------------------------------------------------------------------------------------ an independent pin: grid_sample
@pytest.mark.parametrize("kind", ["zoom_in", "zoom_out", "flip", "shift", "all"])
def test_resample_against_grid_sample_in_float64(kind):
    """The value before the photometric line against torch's grid_sample (bilinear, zeros, align_corners=False) in float64, the grid
    built in float64 from the same fp32 numbers.
    Bound, derived: the fp32 source coordinate is three rounded operations on values no larger than M = |k| n + |c| + .5, and the
    fraction one more on a value below 1: at most (3 M + 1) 2^-24 from the float64 coordinate.  A bilinear surface is continuous and
    its slope along an axis is at most the largest difference D of neighbouring pixels along it (the zero padding counted as
    pixels), so a coordinate error e moves the value by at most e D -- also where the two floors differ.  The value's own arithmetic
    is four weights' roundings (1 - w), four products and three sums on values up to 255: 11 roundings of at most 255 * 2^-24."""
    AI = pkg("augment_image")
    H, W = 41, 57
    img = _image(H, W, 21)
    q = {"zoom_in": AI.params_from(W, H, zoom=1.7), "zoom_out": AI.params_from(W, H, zoom=0.5), "flip": AI.params_from(W, H, flip=True),
         "shift": AI.params_from(W, H, dx=4.3, dy=-2.6), "all": AI.params_from(W, H, zoom=0.83, flip=True, dx=-3.2, dy=1.9)}[kind]
    got = AI.resample(img, q).astype(np.float64)
    ku, cu, kv, cv = (float(v) for v in q["q"][:4])
    xs = ku * (np.arange(W, dtype=np.float64) + 0.5) + cu           # source position in pixel-edge coordinates
    ys = kv * (np.arange(H, dtype=np.float64) + 0.5) + cv
    grid = torch.from_numpy(np.stack(np.broadcast_arrays((2.0 * xs / W - 1.0)[None, :], (2.0 * ys / H - 1.0)[:, None]), -1)[None])
    ref = torch.nn.functional.grid_sample(torch.from_numpy(img.astype(np.float64))[None], grid, mode="bilinear", padding_mode="zeros",
                                          align_corners=False)[0].numpy()
    pad = np.zeros((3, H + 2, W + 2), dtype=np.float64)
    pad[:, 1:-1, 1:-1] = img
    Dx, Dy = np.abs(np.diff(pad, axis=2)).max(), np.abs(np.diff(pad, axis=1)).max()
    ex = (3.0 * (abs(ku) * W + abs(cu) + 0.5) + 1.0) * EPS
    ey = (3.0 * (abs(kv) * H + abs(cv) + 0.5) + 1.0) * EPS
    bound = ex * Dx + ey * Dy + 11 * 255.0 * EPS
    err = np.abs(got - ref).max()
    print("grid_sample pin (%s): max |fp32 statement - float64 grid_sample| = %.3e, bound %.3e" % (kind, err, bound))
    assert bound < 0.05 and err <= bound
    assert ref.max() > 100.0
    if kind in ("zoom_out", "shift", "all"):
        assert (ref == 0).any()                                     # part of the output looks at the padding


# ------------------------------------------------------------------------------------------------ projection matrix
def _points(n, seed):
    return pkg("detfill").synthetic_points(n, (0.0, 70.4, -40.0, 40.0, -2.4, 0.8), seed).astype(np.float64)


@pytest.mark.parametrize("zoom,flip,dx,dy", [(1.3, False, 17.5, -6.25), (0.7, True, -40.0, 11.0), (1.0, True, 0.0, 0.0), (0.5, False, 0.0, 0.0)])
def test_compose_crt_image_moves_every_pixel_with_the_image(zoom, flip, dx, dy):
    """In float64: projecting with crt' gives su u + tu, sv v + tv of the projection with crt.  crt' is the float64 composition
    rounded entry by entry to fp32 (checked), so a0' = [p, 1] . col0' is off by at most 2^-24 |[p, 1]| . |col0'|, and u' by that over
    the depth a2; the float64 evaluation itself adds a relative 1e-12."""
    AI, calib = pkg("augment_image"), pkg("calib")
    W, H = 1242, 375
    crt = calib.kitti_like_crt()
    q = AI.params_from(W, H, zoom=zoom, flip=flip, dx=dx, dy=dy)
    su, tu, sv, tv = AI.affine(q)
    ku, cu, kv, cv = (float(v) for v in q["q"][:4])
    assert (su, tu, sv, tv) == (1.0 / ku, -cu / ku, 1.0 / kv, -cv / kv)
    c64 = np.asarray(crt, dtype=np.float64).reshape(4, 3)
    exact = c64.copy()
    exact[:, 0] = su * c64[:, 0] + tu * c64[:, 2]
    exact[:, 1] = sv * c64[:, 1] + tv * c64[:, 2]
    crt2 = AI.compose_crt_image(crt, q)
    assert crt2.dtype == np.float32 and crt2.shape == (4, 3) and np.array_equal(crt2[:, 2], np.asarray(crt, np.float32).reshape(4, 3)[:, 2])
    assert (np.abs(crt2.astype(np.float64) - exact) <= EPS * np.abs(exact) + 1e-45).all()
    h = np.concatenate([_points(3000, 9), np.ones((3000, 1))], 1)
    a, a2 = h @ c64, h @ crt2.astype(np.float64)
    front = a[:, 2] > 1.0
    assert front.sum() > 1000 and np.array_equal(a[:, 2], a2[:, 2])
    h, a, a2 = h[front], a[front], a2[front]
    u, v = a[:, 0] / a[:, 2], a[:, 1] / a[:, 2]
    u2, v2 = a2[:, 0] / a2[:, 2], a2[:, 1] / a2[:, 2]
    mag = np.abs(h) @ np.abs(exact)
    assert (np.abs(u2 - (su * u + tu)) <= (EPS + 1e-12) * mag[:, 0] / a[:, 2]).all()
    assert (np.abs(v2 - (sv * v + tv)) <= (EPS + 1e-12) * mag[:, 1] / a[:, 2]).all()
    assert np.abs(u2 - u).max() > 1.0                               # (the matrix did move the pixels)
    if flip and zoom == 1.0:
        # a flip alone: su = -1 and tu = W exactly, u' = W - u; column 0 is W col2 - col0 with ONE rounding, the others are untouched
        assert (su, tu, sv, tv) == (-1.0, float(W), 1.0, 0.0)
        want = np.asarray(crt, np.float32).reshape(4, 3).copy()
        want[:, 0] = (W * c64[:, 2] - c64[:, 0]).astype(np.float32)
        assert np.array_equal(crt2, want)
        dyadic = np.array([[0.5, -2.0, 0.0], [-721.5, 0.25, 0.0], [3.0, -700.0, 0.0], [609.25, 172.5, 1.0]], dtype=np.float32)
        dyadic[:3, 2] = [1.0, 0.0, 0.0]                             # short entries: nothing rounds, so the flip is exact end to end
        d2 = AI.compose_crt_image(dyadic, q).astype(np.float64)
        assert np.array_equal(d2[:, 0], W * dyadic[:, 2].astype(np.float64) - dyadic[:, 0].astype(np.float64)) and np.array_equal(d2[:, 1:], dyadic[:, 1:])


def test_compose_crt_image_commutes_with_the_bev_composition():
    """compose_crt acts on rows 0..2, compose_crt_image on columns 0..1: in exact arithmetic they commute.  Each order rounds twice;
    both are compared with the float64 composite E.  BEV first: M1 = fl(A^-T crt) is off by 2^-24 |M1| per entry, which the column
    step turns into 2^-24 (|su| |M1 col0| + |tu| |M1 col2|), plus the final rounding 2^-24 |E|.  Image first: N1 = fl(columns) is off
    by 2^-24 |N1|, which the row step turns into |A^-T| times that on rows 0..2, plus the final rounding."""
    A, AI, calib = pkg("augment"), pkg("augment_image"), pkg("calib")
    W, H = 1242, 375
    crt = calib.kitti_like_crt()
    c64 = np.asarray(crt, dtype=np.float64).reshape(4, 3)
    qb = A.params_from(math.radians(17.0), 1.03, True)
    qi = AI.params_from(W, H, zoom=0.8, flip=True, dx=25.0, dy=-9.0)
    su, tu, sv, tv = AI.affine(qi)
    inv_t = np.linalg.inv(A.matrix3(qb)).T

    def rows(m):
        out = m.copy()
        out[:3] = inv_t @ m[:3]
        return out

    def cols(m, absolute=False):
        out = m.copy()
        f = abs if absolute else (lambda x: x)
        out[:, 0] = f(su) * m[:, 0] + f(tu) * m[:, 2]
        out[:, 1] = f(sv) * m[:, 1] + f(tv) * m[:, 2]
        return out

    E = cols(rows(c64))
    assert np.abs(E - rows(cols(c64))).max() <= 1e-12 * np.abs(E).max()
    bev_first = AI.compose_crt_image(A.compose_crt(crt, qb), qi).astype(np.float64)
    img_first = A.compose_crt(AI.compose_crt_image(crt, qi), qb).astype(np.float64)
    slack = 1.0 + 1e-6
    m1 = np.abs(rows(c64))
    prop1 = cols(m1, absolute=True)
    prop1[:, 2] = 0.0                                               # column 2 passes through the column step unchanged ...
    b1 = EPS * (prop1 + np.abs(E)) * slack
    b1[:, 2] = EPS * np.abs(E[:, 2]) * slack                        # ... so it carries its first rounding only
    n1 = np.abs(cols(c64))
    prop2 = n1.copy()
    prop2[:3] = np.abs(inv_t) @ n1[:3]
    prop2[3] = 0.0                                                  # row 3 passes through the row step unchanged
    b2 = EPS * (prop2 + np.abs(E)) * slack
    b2[3] = EPS * np.abs(E[3]) * slack
    assert (np.abs(bev_first - E) <= b1 + 1e-300).all() and (np.abs(img_first - E) <= b2 + 1e-300).all()
    assert (np.abs(bev_first - img_first) <= b1 + b2).all()


# ------------------------------------------------------------------------------------------------ C ABI
def test_export_declared_bound_and_built():
    H = pkg("_hip")
    header = open(os.path.join(ROOT, "include", "dcf_hip.h")).read()
    assert re.search(r"\bdcf_augment_image_batch\s*\(", header)
    assert "dcf_augment_image_batch" in H.SIGNATURES
    assert getattr(H.lib(), "dcf_augment_image_batch") is not None
    assert callable(pkg("ops").augment_image_batch)
    # bad arguments are refused on the host, before anything touches a device
    L = H.lib()
    assert L.dcf_augment_image_batch(None, 1, 4, 4, None, None, None) == -1 and b"dcf_augment_image_batch" in L.dcf_last_error()
    q = np.array([1, 0, 1, 0, 1, 1, 1, 0] * 9, dtype=np.float32)
    assert L.dcf_augment_image_batch(4096, 9, 4, 4, q.ctypes.data, 8192, None) == -1 and b"frames" in L.dcf_last_error()
    assert L.dcf_augment_image_batch(4096, 1, 4, 4, q.ctypes.data, 4100, None) == -1 and b"overlaps" in L.dcf_last_error()
    q[1] = np.inf
    assert L.dcf_augment_image_batch(4096, 1, 4, 4, q.ctypes.data, 8192, None) == -1 and b"finite" in L.dcf_last_error()

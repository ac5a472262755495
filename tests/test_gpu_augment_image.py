"""GPU suite: train-time camera image augmentation (csrc/image_aug.hip k_augment_image_b, augment_image.py,
Train.one_step_raw / geometry_async(image_augment=...)) -- the kernel against its host statement byte for byte,
the exact cases, the image and the projection moving together, and the trainer."""
import copy
import os

import numpy as np
import pytest
import torch

from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 7), (6, 10), (13, 66), (37, 131), (3, 1030)]        # 3 H W % 4 = 3 1 0 2 1 2; H W % 4 = 1 3 0 2 3 2; a row of 1030 > one block's 1024 bytes
EPS = 2.0 ** -24


def _image(shape, seed):
    return pkg("detfill").uniform(tuple(shape), 5200 + seed, 0.0, 256.0).astype(np.uint8)


def _presets(AI, W, H):
    """Eleven parameter sets: zoom .5 / .8 / 1 / 1.7, both flips, fractional shifts that push part of the frame out, photometric values
    that saturate both ends, one dropped frame."""
    P = AI.params_from
    return [P(W, H, zoom=0.5),
            P(W, H, zoom=0.8, flip=True, dx=0.37 * W, dy=-0.21 * H, contrast=1.9, brightness=1.4),        # 2.66 p - 114.75: both ends clamp
            P(W, H, zoom=1.0, dx=2.5, dy=-1.25),
            P(W, H, zoom=1.7, flip=True, gain=(0.7, 1.0, 1.3)),
            P(W, H, zoom=1.2, dx=1.0, brightness=1.1, drop=True),
            P(W, H, flip=True),
            P(W, H, zoom=1.3, dx=-0.45 * W, dy=0.4 * H, brightness=0.6),
            P(W, H, zoom=0.63, dx=0.2 * W + 0.3, contrast=0.5, gain=(1.2, 0.9, 1.0)),
            P(W, H),
            P(W, H, zoom=0.5, flip=True, dy=0.3 * H),
            P(W, H, zoom=1.7, dx=0.49 * W, contrast=1.5, brightness=2.0)]


# ------------------------------------------------------------------------------------------------ 1. kernel against statement
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_host_statement_bytewise(H, W):
    """Batches of 1, 3, 8 and 11 (two launches) frames, every frame with its own parameters; the input a [:B] view that starts 5 bytes
    into a larger buffer, the output 29 bytes into one filled with a guard value."""
    AI, ops = pkg("augment_image"), pkg("ops")
    N = 3 * H * W
    host = _image((11, 3, H, W), H * W)
    big = torch.zeros(5 + 11 * N + 7, dtype=torch.uint8, device="cuda")
    big[5:5 + 11 * N].copy_(torch.from_numpy(host).reshape(-1))
    frames = big[5:5 + 11 * N].view(11, 3, H, W)
    before = big.clone()
    presets = _presets(AI, W, H)
    want_all = {}
    sat_lo = sat_hi = 0
    for B in (1, 3, 8, 11):
        params = [presets[(b + B) % 11] for b in range(B)]
        inp = frames[:B]
        assert inp.is_contiguous() and inp.data_ptr() % 16 != 0
        obuf = torch.full((29 + B * N + 35,), 0xA5, dtype=torch.uint8, device="cuda")
        out = obuf[29:29 + B * N].view(B, 3, H, W)
        got = ops.augment_image_batch(inp, params, out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        g = out.cpu().numpy()
        for b in range(B):
            key = (b, (b + B) % 11)
            if key not in want_all:
                want_all[key] = AI.transform_image(host[b], params[b])
            assert np.array_equal(g[b], want_all[key]), "B = %d, frame %d (preset %d)" % (B, b, key[1])
            if params[b]["drop"]:
                assert not g[b].any()
            sat_lo += int((g[b] == 0).sum()); sat_hi += int((g[b] == 255).sum())
        guard = obuf.cpu().numpy()
        assert (guard[:29] == 0xA5).all() and (guard[29 + B * N:] == 0xA5).all()
        assert torch.equal(big, before)                                # the input is left alone
    if H * W > 1:
        assert sat_lo > 0 and sat_hi > 0
    # out=None allocates
    res = ops.augment_image_batch(frames[:2], [presets[1], presets[3]])
    assert res.shape == (2, 3, H, W) and res.dtype == torch.uint8 and np.array_equal(res[1].cpu().numpy(), AI.transform_image(host[1], presets[3]))


def test_overlapping_out_and_bad_arguments_are_refused():
    AI, ops, Hh = pkg("augment_image"), pkg("ops"), pkg("_hip")
    buf = torch.zeros(4 * 3 * 5 * 7 + 64, dtype=torch.uint8, device="cuda")
    n = 2 * 3 * 5 * 7
    a = buf[0:n].view(2, 3, 5, 7)
    ident = [AI.identity(7, 5)] * 2
    for off in (0, 1, n - 1):
        with pytest.raises(ValueError):
            ops.augment_image_batch(a, ident, buf[off:off + n].view(2, 3, 5, 7))
    ops.augment_image_batch(a, ident, buf[n:2 * n].view(2, 3, 5, 7))          # adjacent is fine
    with pytest.raises(Hh.DcfError):
        ops.augment_image_batch(a, ident[:1])
    with pytest.raises(Hh.DcfError):
        ops.augment_image_batch(a, [AI.identity(8, 5)] * 2)                      # parameters of another image size
    with pytest.raises(Hh.DcfError):
        ops.augment_image_batch(a.float(), ident)
    with pytest.raises(Hh.DcfError):
        ops.augment_image_batch(buf[0:2 * n].view(2, 3, 5, 14)[:, :, :, :7], ident)   # not contiguous
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. exact cases on the device
def test_identity_flip_and_integer_shift_are_exact_on_the_device():
    AI, ops = pkg("augment_image"), pkg("ops")
    H, W = 37, 131
    img = torch.from_numpy(_image((3, 3, H, W), 77)).cuda()
    out = ops.augment_image_batch(img, [AI.identity(W, H), AI.params_from(W, H, flip=True), AI.params_from(W, H, dx=3.0, dy=-2.0)])
    torch.cuda.synchronize()
    assert torch.equal(out[0], img[0])
    assert torch.equal(out[1], torch.flip(img[1], dims=[2]))
    want = torch.zeros_like(img[2])
    want[:, :H - 2, 3:] = img[2][:, 2:, :W - 3]
    assert torch.equal(out[2], want)


# ------------------------------------------------------------------------------------------------ 3. image and projection move together
def _tiny_crt():
    calib = pkg("calib")
    return calib.crt_from(np.array([[60.0, 0.0, 64.0], [0.0, 60.0, 48.0], [0.0, 0.0, 1.0]]), calib.R_LIDAR_TO_CAM)


def _proj64(pts64, crt_f32):
    """Float64 projection with the fp32 matrix entries, and the bound on what the projection kernel's fp32 chain (ProjPred: a rounded
    product and three fused multiply-adds per column, then a correctly rounded division) can differ from it: every partial sum is at
    most mag = |[p, 1]| . |col| in size, so a column is off by at most 4 * 2^-24 * mag, and u = a0 / a2 by
    (4 * 2^-24 (mag0 + |u| mag2)) / (a2 - 4 * 2^-24 mag2) plus the division's 2^-24 |u|."""
    c = np.asarray(crt_f32, dtype=np.float32).astype(np.float64).reshape(4, 3)
    h = np.concatenate([pts64, np.ones((len(pts64), 1))], 1)
    a, mag = h @ c, np.abs(h) @ np.abs(c)
    uv = a[:, :2] / a[:, 2:3]
    den = a[:, 2:3] - 4 * EPS * mag[:, 2:3]
    err = 4 * EPS * (mag[:, :2] + np.abs(uv) * mag[:, 2:3]) / den * (1 + 1e-6) + EPS * (np.abs(uv) + 1e-30) * (1 + 1e-6)
    return uv, a[:, 2], err


def _bilinear64(img_u8, uv):
    """Float64 two-tap bilinear of a [3,H,W] image at positions (u, v) in pixel-edge coordinates (pixel w spans [w, w + 1)), zeros outside."""
    _, H, W = img_u8.shape
    pad = np.zeros((3, H + 2, W + 2), dtype=np.float64)
    pad[:, 1:-1, 1:-1] = img_u8
    x, y = uv[:, 0] - 0.5, uv[:, 1] - 0.5
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    wx, wy = x - x0, y - y0
    assert x0.min() >= -1 and x0.max() <= W - 1 and y0.min() >= -1 and y0.max() <= H - 1
    x0, y0 = x0 + 1, y0 + 1
    top = pad[:, y0, x0] * (1 - wx) + pad[:, y0, x0 + 1] * wx
    bot = pad[:, y0 + 1, x0] * (1 - wx) + pad[:, y0 + 1, x0 + 1] * wx
    return top * (1 - wy) + bot * wy


@pytest.mark.parametrize("zoom,flip,dx,dy", [(1.3, False, 9.5, -4.25), (0.7, True, -6.0, 3.5), (1.0, True, 0.0, 0.0)])
def test_image_and_projection_move_together(zoom, flip, dx, dy):
    """The 128 x 96 image and the matrix of the trainer tests' tiny config.  The image is a ramp, channel c = gx_c w + gy_c h: a bilinear
    surface reproduces a linear function exactly, so the augmented image (photometric identity) is the ramp seen through the inverse
    affine, quantised -- every pixel within half a level -- wherever its taps lie inside the original, and a bilinear sample of it at
    uv' differs from the original sampled at uv by at most

        1/2 + r  +  (gx |ku| + gy |kv|)-weighted [ e(uv') + m(uv') ]  +  (gx, gy)-weighted e(uv)

    e(.) the projection kernel's own rounding (_proj64), m the rounding of the composed matrix's entries (2^-24 |[p,1]| . |col'| over
    the depth), r the fp32 resampling error in front of the quantiser (the bound test_augment_image_host.py derives, with the ramp's
    slope for the neighbouring-pixel difference).  Condition on the inputs, asserted from the host statement alone: the chosen points project at least
    1.02 + max(|ku|, |kv|) pixels inside both images -- every tap of both samples, and every tap of the kernel behind them, is a
    real pixel -- which is far more than e."""
    AI, ops, Hh = pkg("augment_image"), pkg("ops"), pkg("_hip")
    W, H = 128, 96
    lim = np.array([0.0, 15.8, -6.0, 5.8, -2.4, 0.6], dtype=np.float32)
    crt = _tiny_crt()
    q = AI.params_from(W, H, zoom=zoom, flip=flip, dx=dx, dy=dy)
    crt2 = AI.compose_crt_image(crt, q)
    ku, cu, kv, cv = (float(v) for v in q["q"][:4])
    su, tu, sv, tv = AI.affine(q)
    grad = np.array([[1.0, 1.0], [2.0, 0.0], [0.0, 2.0]])                  # (gx, gy) per channel; 127 + 95, 254, 190 <= 255
    ww, hh = np.meshgrid(np.arange(W), np.arange(H))
    ramp = np.stack([(g[0] * ww + g[1] * hh) for g in grad], 0).astype(np.uint8)
    aug = ops.augment_image_batch(torch.from_numpy(ramp)[None].cuda(), [q])[0].cpu().numpy()
    assert np.array_equal(aug, AI.transform_image(ramp, q))
    host = pkg("detfill").synthetic_points(4000, (6.0, 11.0, -1.0, 1.0, -2.0, 0.2), 61)      # (the generator adds 5 m / 0.4 m of margin: x from 1 m)
    p64 = host.astype(np.float64)
    uv, depth, e = _proj64(p64, crt)
    uv2, depth2, e2 = _proj64(p64, crt2)
    hmag = np.abs(np.concatenate([p64, np.ones((len(p64), 1))], 1)) @ np.abs(crt2.astype(np.float64))
    m2 = EPS * hmag[:, :2] / depth2[:, None] * (1 + 1e-6)
    assert depth.min() > 0.4 and np.array_equal(depth, depth2)
    # the composed matrix does what the host test pins, here too
    assert (np.abs(uv2 - (uv * [su, sv] + [tu, tv])) <= m2 + 1e-9).all()
    in_range = ((host[:, 0] > lim[0]) & (host[:, 0] < lim[1]) & (host[:, 1] > lim[2]) & (host[:, 1] < lim[3]) & (host[:, 2] > lim[4]) & (host[:, 2] < lim[5]))
    margin = 1.02 + max(abs(ku), abs(kv))

    def inside(p, m):
        return (p[:, 0] > m) & (p[:, 0] < W - m) & (p[:, 1] > m) & (p[:, 1] < H - m)

    chosen = in_range & inside(uv, margin) & inside(uv2, margin)
    assert chosen.sum() > 200 and max(e[chosen].max(), e2[chosen].max() + m2[chosen].max()) < 1e-3 < margin
    dev = torch.from_numpy(host).cuda()
    uvd, _, cnt, src = ops.project_filter(dev, lim, crt, float(W), float(H), Hh.PROJ_CORRECT, want_src=True)
    uvd2, _, cnt2, src2 = ops.project_filter(dev, lim, crt2, float(W), float(H), Hh.PROJ_CORRECT, want_src=True)
    n, n2 = int(cnt.item()), int(cnt2.item())
    got = np.full((len(host), 2), np.nan); got2 = np.full((len(host), 2), np.nan)
    got[src[:n].cpu().numpy()] = uvd[:n].cpu().numpy()
    got2[src2[:n2].cpu().numpy()] = uvd2[:n2].cpu().numpy()
    kept, kept2 = ~np.isnan(got[:, 0]), ~np.isnan(got2[:, 0])
    assert kept[chosen].all() and kept2[chosen].all()
    # the kernel's uv are within their bound of the float64 ones (the yardstick holds before it is used)
    assert (np.abs(got[chosen] - uv[chosen]) <= e[chosen]).all() and (np.abs(got2[chosen] - uv2[chosen]) <= e2[chosen]).all()
    s_orig = _bilinear64(ramp, got[chosen])
    s_aug = _bilinear64(aug, got2[chosen])
    k = np.array([abs(ku), abs(kv)])
    # the fp32 resampling behind a pixel of the augmented image, as test_augment_image_host.py derives it: the quantiser sees the ramp's
    # value within r, so a pixel is within 1/2 + r of it
    coord = np.array([(3.0 * (abs(ku) * W + abs(cu) + 0.5) + 1.0) * EPS, (3.0 * (abs(kv) * H + abs(cv) + 0.5) + 1.0) * EPS])
    for c in range(3):
        r = (coord * grad[c]).sum() + 11 * 255.0 * EPS
        bound = 0.5 + r + ((e2[chosen] + m2[chosen]) * k * grad[c]).sum(1) + (e[chosen] * grad[c]).sum(1) + 1e-9
        diff = np.abs(s_aug[c] - s_orig[c])
        print("channel %d: max |aug(uv') - orig(uv)| = %.4f levels, bound %.4f" % (c, diff.max(), bound.min()))
        assert (diff <= bound).all()
    assert np.abs(s_aug - s_orig).max() > 0.0 or (zoom == 1.0)
    # the crop: a point is dropped under crt' exactly when its uv' leaves the image (points within the kernel's rounding of an edge left out)
    edge2 = np.minimum(np.minimum(np.abs(uv2[:, 0]), np.abs(uv2[:, 0] - W)), np.minimum(np.abs(uv2[:, 1]), np.abs(uv2[:, 1] - H)))
    sure = edge2 > e2.max(1)
    assert (~sure).mean() <= 0.005                                          # from the host statement alone
    want2 = in_range & (uv2[:, 0] > 0) & (uv2[:, 0] < W) & (uv2[:, 1] > 0) & (uv2[:, 1] < H)
    assert np.array_equal(kept2[sure], want2[sure])
    if zoom > 1.0:
        assert (kept & ~kept2).sum() > 20                                   # points the un-augmented frame keeps and the crop removes
    if zoom < 1.0:
        assert (kept2 & ~kept).sum() > 20                                   # points from beyond the original frame: they stay, on the padding


# ------------------------------------------------------------------------------------------------ 4. the trainer
def _tiny_cfg(**over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dtype="f32", loss_reduction="mean",
                    bn_mode="eval", learning_rate=1e-3, batch_size=2, loss_sampling="device", loss_seed=5, deterministic=True))
    cfg["lidar_module"] = dict(cfg["lidar_module"], out_feature2=64, out_feature3=128, out_feature4=192, out_feature5=256)   # deterministic fusion widths
    cfg["fusion"] = dict(enabled=True, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    cfg.update(over)
    return cfg


IMG = dict(enabled=True, seed=9, zoom=[0.8, 1.25], shift=[0.1, 0.1], flip_prob=0.5, brightness=[0.8, 1.2], contrast=[0.8, 1.2], channel_gain=[0.9, 1.1],
           drop_prob=0.2)
BEV = dict(enabled=True, seed=9, rotation_deg=20.0, scale=[0.95, 1.05], flip_prob=0.5, point_drop=[0.05, 0.2])


def _trainer(cfg):
    tr = pkg("train").Train(cfg)
    pkg("detfill").fill_state_dict(tr.model)
    return tr


def _batch(cfg, first=0, frames=2):
    """A FrameLoader batch of SyntheticDataset frames, staged by hand (device points and image, host labels)."""
    D, FL = pkg("data_import_carla"), pkg("frame_loader")
    ds = D.SyntheticDataset(cfg, length=8, num_points=1500, crt=_tiny_crt(), raw=True)
    host = FL.collate_raw([ds[first + i] for i in range(frames)])
    batch = FL.Batch(bboxes=host["bboxes"], num_bboxes=host["num_bboxes"], crt=host["crt"])
    batch["points"] = [p.cuda() for p in host["points"]]
    batch["image"] = torch.stack(host["image"], 0).cuda()
    return ds, batch


def _steps(tr, ds, batch, n, grab=None):
    """n one_step_raw calls; the (loss, gradient arena, parameter arena) after each.  grab: a list that receives (x_lidar, image) as
    one_step is handed them."""
    out = []
    if grab is not None:
        orig = tr.one_step

        def spy(x, image, *a, **k):
            torch.cuda.synchronize()                                  # x is still being written on the geometry side stream
            grab.append((x.clone(), image.clone()))
            return orig(x, image, *a, **k)
        tr.one_step = spy
    for _ in range(n):
        tr.one_step_raw(ds.geometry, batch)
        torch.cuda.synchronize()
        out.append((tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone()))
    return out


def test_geometry_async_composes_the_matrices_and_the_trainer_passes_its_draw():
    """geometry_async(points, image_augment=params) == geometry_async(points, crts=compose_crt_image(crt_b, params_b)): counts, the valid
    rows of xyz and uv, bit for bit, with the geometry's own matrix and with per-frame ones; the voxel input is the plain one.  And
    one_step_raw hands geometry_async the parameters it drew: the uv the step consumes are those of the composed matrices."""
    AI, T = pkg("augment_image"), pkg("train")
    cfg = _tiny_cfg(augment_image=dict(IMG))
    tr = _trainer(cfg)
    ds, batch = _batch(cfg)
    geo = ds.geometry

    def snap(points, **kw):
        x, g = tr.geometry_async(geo, points, **kw)
        torch.cuda.synchronize()
        return x.clone(), g["cnt"].clone(), g["xyz"].clone(), g["uv"].clone()

    def same(a, b):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1].min()) > 20
        for f in range(2):
            n = int(a[1][f])
            assert torch.equal(a[2][f, :n].view(torch.int32), b[2][f, :n].view(torch.int32))
            assert torch.equal(a[3][f, :n].view(torch.int32), b[3][f, :n].view(torch.int32))

    params = [AI.params_from(128, 96, zoom=1.2, flip=True, dx=5.5, dy=-3.0), AI.params_from(128, 96, zoom=0.75, dx=-4.0)]
    plain = snap(batch["points"])
    got = snap(batch["points"], image_augment=params)
    same(got, snap(batch["points"], crts=[AI.compose_crt_image(geo.crt, q) for q in params]))
    assert torch.equal(got[0], plain[0])                                       # the image block leaves the points alone ...
    assert not torch.equal(got[1], plain[1]) or not torch.equal(got[3], plain[3])     # ... and moves their pixels
    own = [geo.crt, AI.compose_crt_image(geo.crt, AI.params_from(128, 96, dx=2.0, dy=1.0))]       # a calibration per frame
    same(snap(batch["points"], crts=own, image_augment=params), snap(batch["points"], crts=[AI.compose_crt_image(c, q) for c, q in zip(own, params)]))
    with pytest.raises(ValueError):
        tr.geometry_async(geo, batch["points"], image_augment=params[:1])
    torch.cuda.synchronize()
    # the trainer
    seen = []
    orig = tr.one_step

    def spy(x, image, *a, **k):
        torch.cuda.synchronize()
        seen.append((k["geom"]["cnt"].clone(), k["geom"]["uv"].clone()))
        return orig(x, image, *a, **k)
    tr.one_step = spy
    tr.one_step_raw(geo, batch)
    torch.cuda.synchronize()
    drawn = [AI.draw(T.parse_image_augment_config(cfg), 9, 0, 0, f, 128, 96) for f in range(2)]
    want = snap(batch["points"], crts=[AI.compose_crt_image(geo.crt, q) for q in drawn])
    assert torch.equal(seen[0][0], want[1])
    for f in range(2):
        n = int(want[1][f])
        assert torch.equal(seen[0][1][f, :n].view(torch.int32), want[3][f, :n].view(torch.int32))
    assert not torch.equal(seen[0][0], plain[1]) or not torch.equal(seen[0][1], plain[3])


def test_trainer_block_off_is_the_plain_step():
    cfg = _tiny_cfg()
    ds, batch = _batch(cfg)
    plain = _steps(_trainer(cfg), ds, batch, 2)
    tr = _trainer(_tiny_cfg(augment_image=dict(IMG, enabled=False)))
    assert tr.image_augment is None
    off = _steps(tr, ds, batch, 2)
    assert tr._aug_image is None and tr.aug_calls == 0 and np.isfinite(float(plain[0][0]))
    for s in range(2):
        for u, v in zip(plain[s], off[s]):
            assert torch.equal(u, v)
    with pytest.raises(ValueError):
        pkg("train").Train(_tiny_cfg(augment_image=dict(IMG, enabled=False, zoom=[0.4, 1.0])))


def test_trainer_augmented_steps_repeat_depend_on_the_seed_and_feed_the_host_statement():
    AI, T = pkg("augment_image"), pkg("train")
    cfg = _tiny_cfg(augment_image=dict(IMG))
    ds, batch = _batch(cfg)
    original = batch["image"].clone()
    xa, xb, xc = [], [], []
    ta = _trainer(cfg)
    a = _steps(ta, ds, batch, 3, xa)
    b = _steps(_trainer(copy.deepcopy(cfg)), ds, batch, 3, xb)
    assert ta.aug_calls == 3
    for s in range(3):
        assert torch.equal(xa[s][0], xb[s][0]) and torch.equal(xa[s][1], xb[s][1])
        for u, v in zip(a[s], b[s]):
            assert torch.equal(u, v)
    assert torch.equal(batch["image"], original)                       # the batch's image is not written
    # one persistent buffer, handed to the model as it is
    assert ta._aug_image is not None and ta._aug_image.shape == original.shape and ta._aug_image.dtype == torch.uint8
    # the image handed to the model is the host statement of the drawn parameters
    parsed = T.parse_image_augment_config(cfg)
    src = original.cpu().numpy()
    moved = 0
    for s in range(3):
        for f in range(2):
            q = AI.draw(parsed, 9, 0, s, f, 128, 96)
            want = AI.transform_image(src[f], q)
            assert np.array_equal(xa[s][1][f].cpu().numpy(), want), (s, f)
            moved += int(not np.array_equal(want, src[f]))
    assert moved >= 5 and not torch.equal(xa[0][1], xa[1][1])          # the call count enters the draw
    _steps(_trainer(_tiny_cfg(augment_image=dict(IMG, seed=10))), ds, batch, 1, xc)
    assert not torch.equal(xa[0][1], xc[0][1])
    plain = _steps(_trainer(_tiny_cfg()), ds, batch, 1)
    assert not torch.equal(a[0][0], plain[0][0])


def test_trainer_counter_ticks_once_per_step_with_one_block_or_both():
    """aug_calls after three steps is 3 with the BEV block alone, the image block alone and both; with both on, the BEV block draws
    what it draws alone (the voxel input is bit-identical: the image block leaves the points alone) and the image block what IT draws
    alone."""
    ds, batch = _batch(_tiny_cfg())
    seen = {}
    for name, over in (("bev", dict(augment=dict(BEV))), ("img", dict(augment_image=dict(IMG))), ("both", dict(augment=dict(BEV), augment_image=dict(IMG)))):
        tr = _trainer(_tiny_cfg(**over))
        grab = []
        _steps(tr, ds, batch, 3, grab)
        assert tr.aug_calls == 3, name
        seen[name] = grab
    for s in range(3):
        assert torch.equal(seen["both"][s][0], seen["bev"][s][0]) and torch.equal(seen["both"][s][1], seen["img"][s][1])
        assert torch.equal(seen["bev"][s][1], batch["image"]) and not torch.equal(seen["img"][s][0], seen["bev"][s][0])


def test_trainer_checkpoint_resumes_the_draw_sequence(tmp_path):
    cfg = _tiny_cfg(augment_image=dict(IMG))
    ds, batch = _batch(cfg)
    tr = _trainer(cfg)
    _steps(tr, ds, batch, 1)
    path = os.path.join(str(tmp_path), "ckpt.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert ck["aug_calls"] == 1 and not [k for k in ck if "image" in k]           # no new field
    want = _steps(tr, ds, batch, 1)[0]
    tr2 = _trainer(copy.deepcopy(cfg))
    tr2.load_checkpoint(path)
    assert tr2.aug_calls == 1
    got = _steps(tr2, ds, batch, 1)[0]
    for u, v in zip(want, got):
        assert torch.equal(u, v)


def test_trainer_hip_graphs_batch1_equals_eager():
    runs = {}
    for graphs in (False, True):
        cfg = _tiny_cfg(augment_image=dict(IMG), batch_size=1, hip_graphs=graphs)
        ds, batch = _batch(cfg, frames=1)
        tr = _trainer(cfg)
        assert tr.model.graphs_wanted(1) == graphs
        runs[graphs] = _steps(tr, ds, batch, 3)
        if graphs:
            assert tr.model._graphs is not None and len(tr.model._graphs.sets) >= 1 and not tr.model._graphs.disabled
    for s in range(3):
        print("step %d: loss eager %.9g, graphs %.9g" % (s, float(runs[False][s][0]), float(runs[True][s][0])))
    for s in range(3):
        assert torch.equal(runs[False][s][0], runs[True][s][0]), s
    assert not torch.equal(runs[False][0][0], runs[False][1][0])


class _SpyTester(object):
    """What train.evaluate() needs of a tester; records the inputs it is handed."""

    def __init__(self, tr):
        self.tr, self.seen = tr, []

    def initialize_ap(self):
        pass

    def get_eval_value_onestep(self, x_lidar, image, boxes, nb, **extra):
        torch.cuda.synchronize()                                      # (the side stream may still be writing it)
        self.seen.append((x_lidar.clone(), image.clone()))
        return self.tr.get_loss_value(x_lidar, image, boxes, nb, **extra)[0], None

    def display_average_precision(self):
        pass

    def get_num_P(self):
        return 0

    def get_num_T(self):
        return 0

    def get_num_TP_set(self):
        return {}


def test_evaluation_is_never_augmented():
    T = pkg("train")
    ds, batch = _batch(_tiny_cfg())
    res = {}
    for name, cfg in (("off", _tiny_cfg()), ("on", _tiny_cfg(augment_image=dict(IMG)))):
        tr = _trainer(cfg)
        x_lidar, geom = tr.geometry_async(ds.geometry, batch["points"], crts=batch.get("crt"))
        value, cls, reg = tr.get_loss_value(x_lidar, batch["image"], batch["bboxes"], batch["num_bboxes"], geom=geom)
        spy = _SpyTester(tr)
        mean = T.evaluate(tr, spy, ds, [batch])[0]
        torch.cuda.synchronize()
        assert tr.aug_calls == 0 and tr._aug_image is None
        res[name] = (value, mean, cls.clone(), reg.clone(), spy.seen[0][0], spy.seen[0][1])
    assert res["on"][0] == res["off"][0] and res["on"][1] == res["off"][1] and np.isfinite(res["off"][0]) and np.isfinite(res["off"][1])
    for i in (2, 3, 4, 5):
        assert torch.equal(res["on"][i], res["off"][i])
    assert torch.equal(res["on"][5], batch["image"])

"""GPU suite: train-time BEV augmentation (csrc/geometry.hip k_augment_points_b, augment.py, Train.geometry_async(augment=...);
DESIGN.md section 14) -- the kernel against its host statement bit for bit, dropped points rejected by every consumer, a point
kept on the pixel of its original, the composed geometry, and the trainer."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

LIM = np.array([0.0, 70.2, -40.0, 39.8, -2.4, 0.6], dtype=np.float32)          # the cfg2 grid's range test
SYM = np.array([0.0, 70.0, -40.0, 40.0, -2.4, 0.6], dtype=np.float32)          # a range symmetric in y
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4100]


def _points(n, seed, lim6=(0.0, 70.4, -40.0, 40.0, -2.4, 0.8)):
    return pkg("detfill").synthetic_points(max(n, 1), lim6, seed)[:n]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expected(A, pts, q):
    want = A.transform_points(pts, q)
    want[~A.keep_mask(len(pts), q)] = np.inf
    return want


# ------------------------------------------------------------------------------------------------ 1. kernel against statement
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_kernel_equals_host_statement_bitwise(B, p, inplace):
    """Every size of SIZES in some frame (the B = 8 case carries them all, B = 1 the multi-block one), a different n per frame, frame 1
    at an odd point offset of a larger buffer (a 12-byte-aligned address that is not 16-byte aligned)."""
    A, ops = pkg("augment"), pkg("ops")
    sizes = {1: [4100], 3: [1025, 257, 0], 8: [0, 1, 63, 64, 65, 255, 256, 1023]}[B]
    rounds = [sizes] if B != 8 else [sizes, [257, 1025, 4100, 65, 1, 0, 64, 255]]
    for r, ns in enumerate(rounds):
        params = [A.params_from(math.radians(17.0 + 3 * b), 1.03 - 0.01 * b, b % 2 == 0, p=p, drop_key=0xA5A5A5A5DEADBEEF + 977 * b) for b in range(B)]
        host = [_points(n, 500 + 10 * r + b) for b, n in enumerate(ns)]
        big = torch.zeros((sum(ns) + 2 * B + 16, 3), dtype=torch.float32, device="cuda")
        frames, off, used = [], 1, np.zeros(sum(ns) + 2 * B + 16, bool)
        for b, h in enumerate(host):
            if b == (1 if B > 1 else 0) and off % 2 == 0:
                off += 1                                        # this frame starts at an odd point offset
            v = big[off:off + len(h)]
            v.copy_(torch.from_numpy(h))
            frames.append(v)
            used[off:off + len(h)] = True
            off += len(h) + 1
        odd = frames[1 if B > 1 else 0]
        assert odd.storage_offset() % 6 == 3 and (odd.data_ptr() % 16 != 0 or big.data_ptr() % 16 != 0)
        outs = None if inplace else [torch.full((len(h) + 1, 3), -7.0, dtype=torch.float32, device="cuda")[:len(h)] for h in host]
        got = ops.augment_points_batch(frames, params, outs)
        torch.cuda.synchronize()
        for b, h in enumerate(host):
            g = got[b].cpu().numpy()
            want = _expected(A, h, params[b])
            assert np.array_equal(_bits(g), _bits(want)), "frame %d (n = %d)" % (b, len(h))
            keep = A.keep_mask(len(h), params[b])
            if p == 0.0:
                assert keep.all() and np.isfinite(g).all()
            else:
                assert np.array_equal(np.isposinf(g).all(1), ~keep) and np.isfinite(g[keep]).all()
            if not inplace:
                assert np.array_equal(frames[b].cpu().numpy(), h)          # the input is left alone
        # the rows between and around the frames were not touched
        assert float(big[torch.from_numpy(~used).cuda()].abs().sum()) == 0.0


def test_identity_reproduces_the_input_and_more_than_eight_frames_are_chunked():
    A, ops = pkg("augment"), pkg("ops")
    host = [_points(300 + 41 * b, 700 + b) for b in range(11)]
    frames = [torch.from_numpy(h).cuda() for h in host]
    outs = [torch.empty_like(f) for f in frames]
    ops.augment_points_batch(frames, [A.identity()] * 11, outs)
    for h, o in zip(host, outs):
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(h))
    params = [A.draw({"rotation_deg": 30.0, "scale": (0.9, 1.1), "flip_prob": 0.5, "point_drop": (0.1, 0.2)}, 3, 0, 0, b) for b in range(11)]
    ops.augment_points_batch(frames, params)
    for h, f, q in zip(host, frames, params):
        assert np.array_equal(_bits(f.cpu().numpy()), _bits(_expected(A, h, q)))


def test_overlapping_frames_are_refused():
    A, ops, H = pkg("augment"), pkg("ops"), pkg("_hip")
    buf = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(H.DcfError):
        ops.augment_points_batch([buf[0:32]], [A.identity()], [buf[8:40]])
    with pytest.raises(H.DcfError):
        ops.augment_points_batch([buf[0:16], buf[32:48]], [A.identity()] * 2, [buf[16:32], buf[24:40]])


# ------------------------------------------------------------------------------------------------ 2. the consumers reject dropped points
def test_consumers_reject_dropped_points():
    """Range filter, compat voxeliser (a 32 x 64 x 48 grid) and projection on the augmented buffer == the same three on the host-compacted
    list of kept, host-transformed points: count, compacted rows, grid, uv, bit for bit."""
    A, ops, H, calib = pkg("augment"), pkg("ops"), pkg("_hip"), pkg("calib")
    lim = np.array([0.0, 15.8, -6.0, 5.8, -2.4, 0.6], dtype=np.float32)
    aff = np.array([4, 0, 4, 24, 10, 24], dtype=np.float32)
    dims = (32, 64, 48)
    crt = calib.crt_from(np.array([[60.0, 0.0, 64.0], [0.0, 60.0, 48.0], [0.0, 0.0, 1.0]]), calib.R_LIDAR_TO_CAM)
    q = A.params_from(math.radians(-11.0), 0.97, True, p=0.3, drop_key=0x0123456789ABCDEF)
    host = _points(3000, 81, (0.0, 17.0, -6.5, 6.5, -2.6, 0.9))
    dev = ops.augment_points_batch([torch.from_numpy(host).cuda()], [q])[0]
    keep = A.keep_mask(len(host), q)
    ref = torch.from_numpy(np.ascontiguousarray(A.transform_points(host, q)[keep])).cuda()
    assert 600 < int((~keep).sum()) < 1200 and ref.shape[0] == int(keep.sum())
    crt2 = A.compose_crt(crt, q)
    # range filter
    o1, _, c1 = ops.range_filter(dev, lim)
    o2, _, c2 = ops.range_filter(ref, lim)
    n = int(c1.item())
    assert n == int(c2.item()) and 0 < n < ref.shape[0] and torch.equal(o1[:n].view(torch.int32), o2[:n].view(torch.int32))
    # voxeliser
    g1 = ops.voxelize(dev, lim, aff, dims, H.VOXEL_COMPAT)
    g2 = ops.voxelize(ref, lim, aff, dims, H.VOXEL_COMPAT)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and int((g1 != 0).sum()) > 1000
    # projection
    uv1, x1, k1, _ = ops.project_filter(dev, lim, crt2, 128.0, 96.0, H.PROJ_CORRECT)
    uv2, x2, k2, _ = ops.project_filter(ref, lim, crt2, 128.0, 96.0, H.PROJ_CORRECT)
    m = int(k1.item())
    assert m == int(k2.item()) and m > 50
    assert torch.equal(uv1[:m].view(torch.int32), uv2[:m].view(torch.int32)) and torch.equal(x1[:m].view(torch.int32), x2[:m].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. exact fusion consistency
def _project(pts_dev, lim, crt, ulim=1242.0, vlim=375.0):
    ops, H = pkg("ops"), pkg("_hip")
    uv, xyz, cnt, src = ops.project_filter(pts_dev, lim, crt, ulim, vlim, H.PROJ_CORRECT, want_src=True)
    n = int(cnt.item())
    return uv[:n].cpu().numpy(), src[:n].cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("kind", ["flip", "half"])
def test_flip_and_power_of_two_scale_keep_uv_bitwise(kind):
    """5 000 random points.  Flip alone: (-y)(-c) is the product y c, the y range is symmetric, so the kept sources are the same set and
    uv under crt' is uv under crt bit for bit.  s = 0.5 alone: the rows of crt' are exact doubles, (x / 2)(2 c) = x c, so uv is the same
    for every source both runs keep (the range test sees other coordinates)."""
    A, ops, calib = pkg("augment"), pkg("ops"), pkg("calib")
    crt = calib.kitti_like_crt()
    host = _points(5000, 33, (-2.0, 72.0, -42.0, 42.0, -2.6, 0.9))
    q = A.params_from(0.0, 1.0, True) if kind == "flip" else A.params_from(0.0, 0.5, False)
    uv0, src0 = _project(torch.from_numpy(host).cuda(), SYM, crt)
    aug = ops.augment_points_batch([torch.from_numpy(host).cuda()], [q])[0]
    uv1, src1 = _project(aug, SYM, A.compose_crt(crt, q))
    assert len(src0) > 500
    if kind == "flip":
        assert np.array_equal(src0, src1) and np.array_equal(_bits(uv0), _bits(uv1))
    else:
        both, i0, i1 = np.intersect1d(src0, src1, return_indices=True)
        assert len(both) > 500 and len(src1) > len(src0)              # halved coordinates: more points pass the range test
        assert np.array_equal(_bits(uv0[i0]), _bits(uv1[i1]))


# ------------------------------------------------------------------------------------------------ 4. consistency under rotation
def test_rotation_keeps_uv_within_the_projection_kernels_own_error():
    """theta = 17 deg, s = 1.03, flip on; every point at a camera depth of 2 m or more.
    Yardstick: e0 = max |uv_device(original, crt) - uv_float64(original, crt)|, the parent's projection kernel against float64.
    Bound: the augmented uv, matched by source index, within 8 e0 of the same float64 values (three more roundings in the point
    transform and one per entry of crt' on top of the chain's four: about twice the roundings; 8 leaves room).
    Membership: the kept set equals the host statement's -- in_range on the bit-exact fp32 transformed points, the image test on the
    float64 uv -- with the sources whose float64 uv lies within 8 e0 of an image edge left out; at most 0.5 % may be left out, which
    the test asserts from the host statement alone for a margin of 0.05 px that 8 e0 has to stay under.
    Measured: DESIGN.md section 14."""
    A, ops, calib = pkg("augment"), pkg("ops"), pkg("calib")
    crt = calib.kitti_like_crt()
    ulim, vlim = 1242.0, 375.0
    host = _points(5000, 57, (7.0, 55.0, -25.0, 25.0, -1.8, 0.2))          # (the generator adds 5 m / 0.4 m of margin)
    assert host[:, 0].min() >= 2.0                                    # camera depth = x for this extrinsic
    q = A.params_from(math.radians(17.0), 1.03, True)
    c64 = np.asarray(crt, dtype=np.float64).reshape(4, 3)
    a = np.concatenate([host.astype(np.float64), np.ones((len(host), 1))], 1) @ c64
    assert a[:, 2].min() >= 2.0
    uv64 = a[:, :2] / a[:, 2:3]
    # host statement of the two kept sets
    def in_range(p):
        return (p[:, 0] > LIM[0]) & (p[:, 0] < LIM[1]) & (p[:, 1] > LIM[2]) & (p[:, 1] < LIM[3]) & (p[:, 2] > LIM[4]) & (p[:, 2] < LIM[5])
    in_img = (uv64[:, 0] > 0) & (uv64[:, 0] < ulim) & (uv64[:, 1] > 0) & (uv64[:, 1] < vlim)
    edge = np.minimum(np.minimum(np.abs(uv64[:, 0]), np.abs(uv64[:, 0] - ulim)), np.minimum(np.abs(uv64[:, 1]), np.abs(uv64[:, 1] - vlim)))
    CAP = 0.05
    assert (edge <= CAP).mean() <= 0.005                              # the inputs stay under the cap, from the host statement alone
    moved = A.transform_points(host, q)
    want0, want1 = in_range(host) & in_img, in_range(moved) & in_img
    assert want0.sum() > 300 and want1.sum() > 300
    # the yardstick
    uv0, src0 = _project(torch.from_numpy(host).cuda(), LIM, crt, ulim, vlim)
    e0 = float(np.abs(uv0.astype(np.float64) - uv64[src0]).max())
    assert 0.0 < 8 * e0 <= CAP
    # the augmented path
    aug = ops.augment_points_batch([torch.from_numpy(host).cuda()], [q])[0]
    assert np.array_equal(_bits(aug.cpu().numpy()), _bits(moved))
    uv1, src1 = _project(aug, LIM, A.compose_crt(crt, q), ulim, vlim)
    dev1 = float(np.abs(uv1.astype(np.float64) - uv64[src1]).max())
    print("rotation consistency: e0 = %.3e px, augmented deviation = %.3e px (%.2f e0), %d / %d kept" % (e0, dev1, dev1 / e0, len(src1), len(src0)))
    assert dev1 <= 8 * e0
    sure = edge > 8 * e0
    assert (~sure).mean() <= 0.005
    got0, got1 = np.zeros(len(host), bool), np.zeros(len(host), bool)
    got0[src0], got1[src1] = True, True
    assert np.array_equal(got0[sure], want0[sure]) and np.array_equal(got1[sure], want1[sure])


# ------------------------------------------------------------------------------------------------ 5 / 6: the trainer
def _tiny_cfg(**over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dtype="f32", loss_reduction="mean",
                    bn_mode="eval", learning_rate=1e-3, batch_size=2, loss_sampling="device", loss_seed=5, deterministic=True))
    cfg["lidar_module"] = dict(cfg["lidar_module"], out_feature2=64, out_feature3=128, out_feature4=192, out_feature5=256)   # deterministic fusion widths
    cfg["fusion"] = dict(enabled=True, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    cfg.update(over)
    return cfg


AUG = dict(enabled=True, seed=9, rotation_deg=20.0, scale=[0.95, 1.05], flip_prob=0.5, point_drop=[0.05, 0.2])
NEUTRAL = dict(enabled=True, seed=9, rotation_deg=0.0, scale=[1.0, 1.0], flip_prob=0.0, point_drop=[0.0, 0.0])


def _tiny_crt():
    calib = pkg("calib")
    return calib.crt_from(np.array([[60.0, 0.0, 64.0], [0.0, 60.0, 48.0], [0.0, 0.0, 1.0]]), calib.R_LIDAR_TO_CAM)


def _trainer(cfg):
    tr = pkg("train").Train(cfg)
    pkg("detfill").fill_state_dict(tr.model)
    return tr


def _batch(cfg, first=0):
    """A FrameLoader batch of two SyntheticDataset frames, staged by hand (device points and image, host labels)."""
    D, FL = pkg("data_import_carla"), pkg("frame_loader")
    ds = D.SyntheticDataset(cfg, length=8, num_points=1500, crt=_tiny_crt(), raw=True)
    host = FL.collate_raw([ds[first + i] for i in range(2)])
    batch = FL.Batch(bboxes=host["bboxes"], num_bboxes=host["num_bboxes"], crt=host["crt"])
    batch["points"] = [p.cuda() for p in host["points"]]
    batch["image"] = torch.stack(host["image"], 0).cuda()
    return ds, batch


def test_geometry_async_composition():
    """geometry_async(points, augment=params) == geometry_async(host-transformed, host-compacted points, crts'): x_lidar, cnt, the valid
    rows of xyz and uv, every KNN idx map, bit for bit."""
    A = pkg("augment")
    cfg = _tiny_cfg()
    tr = _trainer(cfg)
    ds, batch = _batch(cfg)
    geo = ds.geometry
    params = [A.params_from(math.radians(14.0), 1.04, True, p=0.25, drop_key=1234567), A.params_from(math.radians(-9.0), 0.96, False, p=0.1, drop_key=7654321)]
    x1, g1 = tr.geometry_async(geo, batch["points"], augment=params)
    torch.cuda.synchronize()
    x1 = x1.clone()
    got = dict(cnt=g1["cnt"].clone(), xyz=g1["xyz"].clone(), uv=g1["uv"].clone(), idx=[t.clone() for t in g1["idx"]])
    ref_pts, crts = [], []
    for p, q in zip(batch["points"], params):
        h = p.cpu().numpy()
        ref_pts.append(torch.from_numpy(np.ascontiguousarray(A.transform_points(h, q)[A.keep_mask(len(h), q)])).cuda())
        crts.append(A.compose_crt(geo.crt, q))
    x2, g2 = tr.geometry_async(geo, ref_pts, crts=crts)
    torch.cuda.synchronize()
    assert torch.equal(x1, x2) and int((x1 != 0).sum()) > 100
    assert torch.equal(got["cnt"], g2["cnt"]) and int(got["cnt"].min()) > 20
    for b in range(2):
        n = int(got["cnt"][b])
        assert torch.equal(got["xyz"][b, :n].view(torch.int32), g2["xyz"][b, :n].view(torch.int32))
        assert torch.equal(got["uv"][b, :n].view(torch.int32), g2["uv"][b, :n].view(torch.int32))
    assert len(got["idx"]) == len(g2["idx"]) > 0
    for i1, i2 in zip(got["idx"], g2["idx"]):
        assert torch.equal(i1, i2)
    # ... and not the un-augmented geometry
    x0, _ = tr.geometry_async(geo, batch["points"])
    torch.cuda.synchronize()
    assert not torch.equal(x0, x1)


def _steps(tr, ds, batch, n, grab=None):
    out = []
    if grab is not None:
        orig = tr.one_step

        def spy(x, *a, **k):
            torch.cuda.synchronize()                                  # x is still being written on the geometry side stream
            grab.append(x.clone())
            return orig(x, *a, **k)
        tr.one_step = spy
    for _ in range(n):
        tr.one_step_raw(ds.geometry, batch)
        torch.cuda.synchronize()
        out.append((tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone()))
    return out


def test_trainer_neutral_augmentation_is_the_plain_step():
    cfg = _tiny_cfg()
    ds, batch = _batch(cfg)
    plain = _steps(_trainer(cfg), ds, batch, 1)[0]
    tr = _trainer(_tiny_cfg(augment=dict(NEUTRAL)))
    assert tr.augment is not None
    neutral = _steps(tr, ds, batch, 1)[0]
    assert tr.aug_calls == 1 and np.isfinite(float(plain[0]))
    assert torch.equal(plain[0], neutral[0]) and torch.equal(plain[1], neutral[1]) and torch.equal(plain[2], neutral[2])


def test_trainer_augmented_steps_repeat_and_depend_on_the_seed():
    cfg = _tiny_cfg(augment=dict(AUG))
    ds, batch = _batch(cfg)
    labels = (batch["bboxes"].clone(), batch["num_bboxes"].clone())
    xa, xb, xc = [], [], []
    a = _steps(_trainer(cfg), ds, batch, 2, xa)
    b = _steps(_trainer(copy.deepcopy(cfg)), ds, batch, 2, xb)
    for s in range(2):
        assert torch.equal(xa[s], xb[s])
        for u, v in zip(a[s], b[s]):
            assert torch.equal(u, v)
    assert not torch.equal(xa[0], xa[1])                              # the call count enters the draw
    assert torch.equal(batch["bboxes"], labels[0]) and torch.equal(batch["num_bboxes"], labels[1])     # the batch's labels are not written
    _steps(_trainer(_tiny_cfg(augment=dict(AUG, seed=10))), ds, batch, 1, xc)
    assert not torch.equal(xa[0], xc[0])
    x0 = []
    plain = _steps(_trainer(_tiny_cfg()), ds, batch, 1, x0)
    assert not torch.equal(xa[0], x0[0]) and not torch.equal(a[0][0], plain[0][0])


def test_trainer_checkpoint_carries_the_augmentation_count(tmp_path):
    cfg = _tiny_cfg(augment=dict(AUG))
    ds, batch = _batch(cfg)
    tr = _trainer(cfg)
    _steps(tr, ds, batch, 2)
    path = os.path.join(str(tmp_path), "ckpt.pt")
    tr.save_checkpoint(path)
    assert torch.load(path, map_location="cpu")["aug_calls"] == 2
    want = _steps(tr, ds, batch, 1)[0]
    tr2 = _trainer(copy.deepcopy(cfg))
    tr2.load_checkpoint(path)
    assert tr2.aug_calls == 2
    got = _steps(tr2, ds, batch, 1)[0]
    for u, v in zip(want, got):
        assert torch.equal(u, v)
    # a checkpoint without the count resumes from the optimiser's step count
    ck = torch.load(path, map_location="cpu")
    del ck["aug_calls"]
    torch.save(ck, path)
    tr2.aug_calls = 77
    tr2.load_checkpoint(path)
    assert tr2.aug_calls == 2


class _SpyTester(object):
    """What train.evaluate() needs of a tester; records the voxel input it is handed."""

    def __init__(self, tr):
        self.tr, self.seen = tr, []

    def initialize_ap(self):
        pass

    def get_eval_value_onestep(self, x_lidar, image, boxes, nb, **extra):
        torch.cuda.synchronize()                                      # (the side stream may still be writing it)
        self.seen.append(x_lidar.clone())
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
    for name, cfg in (("off", _tiny_cfg()), ("on", _tiny_cfg(augment=dict(AUG)))):
        tr = _trainer(cfg)
        x_lidar, geom = tr.geometry_async(ds.geometry, batch["points"], crts=batch.get("crt"))
        value, cls, reg = tr.get_loss_value(x_lidar, batch["image"], batch["bboxes"], batch["num_bboxes"], geom=geom)
        spy = _SpyTester(tr)
        mean = T.evaluate(tr, spy, ds, [batch])[0]
        torch.cuda.synchronize()
        assert tr.aug_calls == 0
        res[name] = (value, cls.clone(), reg.clone(), x_lidar.clone(), spy.seen[0], mean)
    assert res["on"][0] == res["off"][0] and res["on"][5] == res["off"][5] and np.isfinite(res["off"][0]) and np.isfinite(res["off"][5])
    for i in (1, 2, 3, 4):
        assert torch.equal(res["on"][i], res["off"][i])
    assert torch.equal(res["on"][3], res["on"][4])

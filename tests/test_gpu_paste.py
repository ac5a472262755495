"""GPU: train-time object pasting (csrc/paste.hip, ops.paste_points_batch / paste_patches_batch, Train.one_step_raw with the
`augment_paste` block) against the host statements of paste.py."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from _paste_util import CAR, Frames, box_points, label_row, make_frame, plan_of, random_bank, tiny_crt
from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

GUARD_F = 12345.0
GUARD_B = 0xA5


# ------------------------------------------------------------------------------------------------ 1. points
# (n_b, m_b) of the frames a batch takes from the front: every n of {0, 1, 63, 64, 65, 1000} and every m of {0, 1, 16}; the one-row
# frame has no records (a single row cannot be both removed and kept)
SPECS = [(1000, 16), (0, 1), (1, 0), (63, 1), (64, 16), (65, 1), (1000, 0), (0, 0), (64, 1), (65, 16), (63, 0)]
YAWS = [0.0, math.pi / 2, 0.7, -2.1]


def _points_frame(n, m, seed, bank):
    """(points [n,3], plan): m records on a grid of box positions (yaws 0, pi/2 and two arbitrary ones in turn, margin 0.25); about a
    third of the rows inside the records' boxes, the six points exactly on the faces of the first (yaw 0, dyadic) box, NaN and +-inf
    rows, the rest far away; every record appends a stretch of the bank."""
    P = pkg("paste")
    rng = np.random.RandomState(300 + seed)
    boxes = [label_row(6.0 + 6.0 * (j % 4), -12.0 + 6.0 * (j // 4), -1.0, YAWS[j % 4]) for j in range(m)]
    recs = [P.record(b, 0.25) for b in boxes]
    M = len(bank["boxes"])
    app = []
    for j in range(m):
        r = int(rng.randint(0, M))
        app.append((int(bank["point_start"][r]), int(bank["point_start"][r + 1] - bank["point_start"][r])))
    pts = rng.uniform(40.0, 60.0, (n, 3)).astype(np.float32)              # far from every box (x <= 27)
    if m and n >= 2:
        k = max(n // 3, 1)
        pts[:k] = np.concatenate([box_points(boxes[i % m], 1, rng) for i in range(k)], 0)
        if n >= 63:
            hl, hw, hh = CAR[0] / 2 + 0.25, CAR[1] / 2 + 0.25, CAR[2] / 2 + 0.25
            cx, cy, cz = (float(v) for v in boxes[0][:3])
            pts[k:k + 6] = [[cx + hl, cy, cz], [cx - hl, cy, cz], [cx, cy + hw, cz], [cx, cy - hw, cz], [cx, cy, cz + hh], [cx, cy, cz - hh]]
            pts[k + 6:k + 11] = [[np.nan, cy, cz], [np.inf, cy, cz], [-np.inf, cy, cz], [cx, cy, np.nan], [cx, np.inf, cz]]
        pts[:] = pts[rng.permutation(n)]
    return pts, plan_of(records=recs if m else None, append=app if m else None, n_points=n)


@pytest.mark.parametrize("B", [1, 3, 8, 11])
def test_points_kernel_equals_host_statement_bitwise(B):
    P, ops = pkg("paste"), pkg("ops")
    bank = random_bank(40, (96, 128), 21)
    bank_big = torch.full((len(bank["points"]) + 2, 3), GUARD_F)
    bank_big[1:-1] = torch.from_numpy(bank["points"])
    bank_all = bank_big.cuda()
    bank_dev = bank_all[1:-1]                                             # 12 bytes into a larger buffer
    frames = [_points_frame(n, m, 10 * B + i, bank) for i, (n, m) in enumerate(SPECS[:B])]
    ins, outs, want = [], [], []
    for pts, plan in frames:
        big = torch.full((len(pts) + 3, 3), GUARD_F)
        big[1:1 + len(pts)] = torch.from_numpy(pts)
        ins.append(big.cuda())
        want.append(P.paste_points(pts, plan, bank))
        outs.append(torch.full((5 + len(want[-1]) + 4, 3), GUARD_F, device="cuda"))
    keep = [t.clone() for t in ins]
    views = [t[1:1 + len(f[0])] for t, f in zip(ins, frames)]
    got = ops.paste_points_batch(views, [f[1] for f in frames], bank_dev, [o[5:] for o in outs])
    torch.cuda.synchronize()
    for i, ((pts, plan), (n, m)) in enumerate(zip(frames, SPECS)):
        rows = len(want[i])
        assert tuple(got[i].shape) == (rows, 3) and (rows == 0 or got[i].data_ptr() == outs[i][5:].data_ptr())
        assert np.array_equal(got[i].cpu().numpy().view(np.uint32), want[i].view(np.uint32)), (B, i)
        host = outs[i].cpu().numpy()
        assert (host[:5] == GUARD_F).all() and (host[5 + rows:] == GUARD_F).all()          # nothing before row 0 or past row n + a
        assert torch.equal(ins[i].view(torch.int32), keep[i].view(torch.int32))            # the inputs are not written
        if n >= 2 and m >= 1:                                                              # both branches are exercised
            gone = np.isposinf(want[i][:n]).all(1) & ~np.isposinf(pts).all(1)
            assert gone.sum() >= 1 and (~gone).sum() >= 1
            if n >= 63:
                assert gone.sum() >= n // 3 + 6                                            # the six face points among them
                odd = ~np.isfinite(pts).all(1)
                assert odd.sum() == 5 and np.array_equal(want[i][:n][odd].view(np.uint32), pts[odd].view(np.uint32))
    assert torch.equal(bank_all.cpu(), bank_big)


def test_points_kernel_refuses_bad_arguments():
    ops, Hh = pkg("ops"), pkg("_hip")
    bank = torch.zeros((50, 3), device="cuda")
    pts = torch.zeros((10, 3), device="cuda")
    plan = plan_of(records=[[0, 0, 0, 1, 0, 1, 1, 1]], append=[(40, 10)], n_points=10)
    out = torch.zeros((20, 3), device="cuda")
    ops.paste_points_batch([pts], [plan], bank, [out])
    with pytest.raises(Hh.DcfError):                                      # an output too small for n + a rows
        ops.paste_points_batch([pts], [plan], bank, [out[:19]])
    with pytest.raises(Hh.DcfError):                                      # bank rows that do not exist
        ops.paste_points_batch([pts], [plan_of(records=[[0, 0, 0, 1, 0, 1, 1, 1]], append=[(41, 10)], n_points=10)], bank, [out])
    with pytest.raises(Hh.DcfError):                                      # the output over its own input
        ops.paste_points_batch([out[:10]], [plan], bank, [out])
    with pytest.raises(Hh.DcfError):
        ops.paste_points_batch([pts], [plan, plan], bank, [out])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. patches
SHAPES = [(1, 1), (5, 7), (13, 66), (3, 1030)]        # the image test's own list: W = 1030 is a row longer than one block


def _patch_bank(H, W, seed):
    """Six patches [3,ph,pw] of random bytes, as large as the image allows: (pw, ph, start) each, and the bytes."""
    rng = np.random.RandomState(400 + seed)
    dims = [(W, H), (1, 1), (max(W // 2, 1), max(H // 2, 1)), (max(W - 1, 1), H), (min(W, 5), min(H, 3)), (max(W // 3, 1), H)]
    out, start = [], 0
    for pw, ph in dims:
        out.append((pw, ph, start))
        start += 3 * pw * ph
    return out, rng.randint(0, 256, start).astype(np.uint8)


def _record_sets(H, W, pb):
    """The six record sets of one image size: none; one covering the whole image; a 1x1; three deep overlapping; one touching each
    border; one clipped with non-zero source offsets (where the image leaves room for them)."""
    def rec(x0, y0, w, h, sx, sy, k):
        pw, ph, start = pb[k]
        assert 0 <= x0 and x0 + w <= W and 0 <= y0 and y0 + h <= H and w >= 1 and h >= 1 and 0 <= sx and sx + w <= pw and 0 <= sy and sy + h <= ph
        return (x0, y0, w, h, sx, sy, pw, ph, start)
    w2, h2 = pb[2][0], pb[2][1]
    deep = [rec(0, 0, w2, h2, 0, 0, 2), rec(min(w2 // 2, W - w2), min(h2 // 2, H - h2), w2, h2, 0, 0, 2), rec(W - pb[4][0], H - pb[4][1], pb[4][0], pb[4][1], 0, 0, 4)]
    w5 = pb[5][0]
    borders = [rec(0, 0, w5, 1, 0, 0, 5), rec(W - w5, H - 1, w5, 1, 0, H - 1, 5), rec(0, 0, 1, H, 0, 0, 5), rec(W - 1, 0, 1, H, w5 - 1, 0, 5)]
    pw, ph = pb[3][0], pb[3][1]
    sx, sy = (1 if pw >= 2 else 0), (1 if ph >= 2 else 0)
    clipped = [rec(0, 0, pw - sx, ph - sy, sx, sy, 3)]
    return [[], [rec(0, 0, W, H, 0, 0, 0)], [rec(W // 2, H // 2, 1, 1, 0, 0, 1)], deep, borders, clipped]


@pytest.mark.parametrize("H,W", SHAPES)
def test_patch_kernel_equals_host_statement_bytewise(H, W):
    P, ops = pkg("paste"), pkg("ops")
    pb, patch = _patch_bank(H, W, H + W)
    sets = _record_sets(H, W, pb)
    if W >= 2:
        assert sets[5][0][4] == 1                                         # a non-zero source offset is really exercised
    bank = {"patch": patch}
    bank_dev = torch.from_numpy(np.concatenate([[GUARD_B] * 3, patch, [GUARD_B] * 3]).astype(np.uint8)).cuda()[3:-3]
    rng = np.random.RandomState(H * 31 + W)
    N = 3 * H * W
    for B in (1, 3, 8, 11):
        img = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
        plans = [plan_of(patches=sets[(b + B) % 6], hw=(H, W)) for b in range(B)]
        big_in = torch.full((5 + B * N + 7,), GUARD_B, dtype=torch.uint8)
        big_in[5:5 + B * N] = torch.from_numpy(img).reshape(-1)
        big_in = big_in.cuda()
        big_out = torch.full((29 + B * N + 9,), GUARD_B, dtype=torch.uint8, device="cuda")
        src = big_in[5:5 + B * N].view(B, 3, H, W)                        # 5 bytes into its buffer
        dst = big_out[29:29 + B * N].view(B, 3, H, W)                     # 29 bytes into its buffer
        got = ops.paste_patches_batch(src, plans, bank_dev, dst)
        torch.cuda.synchronize()
        assert got.data_ptr() == dst.data_ptr()
        host = big_out.cpu().numpy()
        assert (host[:29] == GUARD_B).all() and (host[29 + B * N:] == GUARD_B).all()
        assert np.array_equal(big_in.cpu().numpy()[5:5 + B * N], img.reshape(-1))
        for b in range(B):
            want = P.paste_image(img[b], plans[b], bank)
            assert np.array_equal(host[29 + b * N:29 + (b + 1) * N].reshape(3, H, W), want), (H, W, B, b)
            if not len(plans[b]["patches"]):
                assert np.array_equal(want, img[b])


def test_patch_kernel_refuses_overlap_and_bad_records():
    ops, Hh = pkg("ops"), pkg("_hip")
    buf = torch.zeros(2 * 210 + 16, dtype=torch.uint8, device="cuda")
    img = buf[:210].view(2, 3, 5, 7)
    bank = torch.zeros(3 * 2 * 2, dtype=torch.uint8, device="cuda")
    ok = plan_of(patches=[(1, 1, 2, 2, 0, 0, 2, 2, 0)], hw=(5, 7))
    plans = [ok, plan_of(hw=(5, 7))]
    ops.paste_patches_batch(img, plans, bank, torch.empty_like(img))
    for off in (0, 1, 209):
        with pytest.raises(ValueError):                                   # out over the input
            ops.paste_patches_batch(img, plans, bank, buf[off:off + 210].view(2, 3, 5, 7))
    with pytest.raises(ValueError):                                       # a plan drawn for another image size
        ops.paste_patches_batch(img, [plan_of(hw=(5, 8)), ok], bank, torch.empty_like(img))
    for bad in ((6, 1, 2, 2, 0, 0, 2, 2, 0), (1, 4, 2, 2, 0, 0, 2, 2, 0), (1, 1, 2, 2, 1, 0, 2, 2, 0), (1, 1, 2, 2, 0, 0, 2, 2, 1), (1, 1, 0, 2, 0, 0, 2, 2, 0),
                (-1, 1, 2, 2, 0, 0, 2, 2, 0)):
        with pytest.raises(Hh.DcfError):                                  # every index is checked on the host before anything is copied
            ops.paste_patches_batch(img, [plan_of(patches=[bad], hw=(5, 7)), ok], bank, torch.empty_like(img))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. points and pixels agree
def test_pasted_points_project_into_their_patches():
    """A bank from two small frames under calib.kitti_like_crt() (375 x 1242 ramp images), its objects pasted into a third frame of
    the same calibration; the pasted rows are projected with the project kernel (projection_mode: correct).  Every valid pixel must
    lie inside its object's destination rectangle.  Allowed excess: ONE pixel -- the floor / ceil slack of the rectangle; a point
    inside a box projects inside the hull of the box's projected corners, and the kernel's fp32 projection rounding is orders of
    magnitude below a pixel.  Then the pasted image, read back at those pixels, holds the bank's bytes."""
    P, B, ops, Hh = pkg("paste"), pkg("objbank"), pkg("ops"), pkg("_hip")
    crt = pkg("calib").kitti_like_crt()
    hw = (375, 1242)
    lim6 = (0.0, 70.4, -40.0, 40.0, -3.0, 1.0)
    config = dict(lidar_x_min=0.0, lidar_x_max=70.4, lidar_y_min=-40.0, lidar_y_max=40.0, max_num_bbox=20, max_num_pc=4096)
    spots = [[(9.0, 2.0, 0.4), (15.0, -3.5, 1.2), (24.0, 5.0, 2.0)], [(12.0, -1.0, 0.1), (19.0, 4.0, 2.6), (30.0, -6.0, 1.6)]]
    items = [make_frame([label_row(x, y, -1.0, yaw) for x, y, yaw in s], [60, 50, 40], 300, lim6, hw, 40 + f) for f, s in enumerate(spots)]
    bank = B.build(Frames(items, crt), config)
    assert len(bank["boxes"]) == 6 and (bank["rect"][:, 2] > 0).all()
    target = make_frame([], [], 500, lim6, hw, 49)
    pts, img = target["lidar_points"].numpy(), target["image"].numpy()
    plan = P.draw({"seed": 1, "target_objects": 15, "max_candidates": 16, "margin": 0.25, "paste_image": True}, 1, 0, 0, 0, bank,
                  target["bboxes"].numpy(), 0, len(pts), crt, config)
    assert len(plan["rows"]) >= 3                                         # (from the host plan alone)
    bank_pts, bank_patch = torch.from_numpy(bank["points"]).cuda(), torch.from_numpy(bank["patch"]).cuda()
    out = torch.empty((len(pts) + int(plan["append"][:, 1].sum()), 3), device="cuda")
    pasted = ops.paste_points_batch([torch.from_numpy(pts).cuda()], [plan], bank_pts, [out])[0]
    image = ops.paste_patches_batch(torch.from_numpy(img)[None].cuda(), [plan], bank_patch, torch.empty((1, 3) + hw, dtype=torch.uint8, device="cuda"))[0]
    lim = np.array(lim6, dtype=np.float32)
    uv, _, cnt, src = ops.project_filter(pasted, lim, crt, float(hw[1]), float(hw[0]), Hh.PROJ_CORRECT, want_src=True)
    torch.cuda.synchronize()
    n = int(cnt.item())
    uv, src, image = uv[:n].cpu().numpy().astype(np.float64), src[:n].cpu().numpy(), image.cpu().numpy()
    assert np.array_equal(image, P.paste_image(img, plan, bank)) and np.array_equal(pasted.cpu().numpy().view(np.uint32), P.paste_points(pts, plan, bank).view(np.uint32))
    owner = np.full(hw, -1)
    for j, q in enumerate(plan["patches"]):
        owner[q[1]:q[1] + q[3], q[0]:q[0] + q[2]] = j
    first = len(pts)
    worst, checked, read = 0.0, 0, 0
    for k, r in enumerate(plan["rows"]):
        a = int(plan["append"][k, 1])
        mine = (src >= first) & (src < first + a)
        first += a
        j = plan["patch_rows"].index(r)
        x0, y0, w, h, sx, sy, pw, ph, start = (int(v) for v in plan["patches"][j])
        u, v = uv[mine, 0], uv[mine, 1]
        assert mine.sum() >= 0.9 * a                                      # the object is in front of this camera, inside its image
        excess = np.maximum.reduce([x0 - u, u - (x0 + w), y0 - v, v - (y0 + h), np.zeros_like(u)])
        worst, checked = max(worst, float(excess.max())), checked + int(mine.sum())
        px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        sel = (px >= x0) & (px < x0 + w) & (py >= y0) & (py < y0 + h)
        sel[sel] = owner[py[sel], px[sel]] == j                           # not under a nearer object's patch
        patch = bank["patch"][start:start + 3 * pw * ph].reshape(3, ph, pw)
        assert np.array_equal(image[:, py[sel], px[sel]], patch[:, py[sel] - y0 + sy, px[sel] - x0 + sx])
        # ... which are the SOURCE frame's pixels at the same place (equal calibrations: the shift is 0)
        f = int(bank["source"][r][0])
        assert np.array_equal(image[:, py[sel], px[sel]], items[f]["image"].numpy()[:, py[sel], px[sel]])
        read += int(sel.sum())
    print("pasted points: %d projected, largest excess over the destination rectangle %.6f px; %d pixels read back" % (checked, worst, read))
    assert checked >= 100 and read >= 80
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the trainer
def _tiny_cfg(**over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dtype="f32", loss_reduction="mean",
                    bn_mode="eval", learning_rate=1e-3, batch_size=2, loss_sampling="device", loss_seed=5, deterministic=True))
    cfg["lidar_module"] = dict(cfg["lidar_module"], out_feature2=64, out_feature3=128, out_feature4=192, out_feature5=256)   # deterministic fusion widths
    cfg["fusion"] = dict(enabled=True, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    cfg.update(over)
    return cfg


LIM_TINY = (0.0, 16.0, -4.0, 4.0, -2.4, 0.8)
SLOTS = [(3.0, -2.5), (8.0, 2.5), (13.0, -2.5), (13.0, 2.5), (3.0, 2.5), (8.0, -2.5)]
BEV = dict(enabled=True, seed=9, rotation_deg=20.0, scale=[0.95, 1.05], flip_prob=0.5, point_drop=[0.05, 0.2])
IMG = dict(enabled=True, seed=9, zoom=[0.8, 1.25], shift=[0.1, 0.1], flip_prob=0.5, brightness=[0.8, 1.2], contrast=[0.8, 1.2], channel_gain=[0.9, 1.1],
           drop_prob=0.2)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A bank of 8 objects (two frames, four cars each, on the slots of a 16 m x 8 m grid) saved as .npz, and a staged batch of two
    frames of about 1500 points with one label each."""
    B, D, FL = pkg("objbank"), pkg("data_import_carla"), pkg("frame_loader")
    cfg = _tiny_cfg()
    hw = (96, 128)
    src = [make_frame([label_row(x, y, -1.0, 0.2 * f + 0.1 * i) for i, (x, y) in enumerate(SLOTS[:4])], [30, 25, 35, 28], 600, LIM_TINY, hw, 60 + f)
           for f in range(2)]
    bank = B.build(Frames(src, tiny_crt()), cfg)
    assert len(bank["boxes"]) == 8
    path = os.path.join(str(tmp_path_factory.mktemp("paste")), "bank.npz")
    B.save(path, bank)
    frames = [make_frame([label_row(SLOTS[4 + f][0], SLOTS[4 + f][1], -1.0, 0.3)], [30], 1400, LIM_TINY, hw, 70 + f) for f in range(2)]
    host = FL.collate_raw(frames)
    batch = FL.Batch(bboxes=host["bboxes"], num_bboxes=host["num_bboxes"], crt=host["crt"])
    batch["points"] = [p.cuda() for p in host["points"]]
    batch["image"] = torch.stack(host["image"], 0).cuda()
    return {"bank": bank, "path": path, "batch": batch, "geo": D.FrameGeometry(cfg, tiny_crt())}


def _paste_block(world, **over):
    return dict(dict(enabled=True, seed=9, bank=world["path"], target_objects=4, max_candidates=8, margin=0.1, paste_image=True), **over)


def _trainer(cfg):
    tr = pkg("train").Train(cfg)
    pkg("detfill").fill_state_dict(tr.model)
    return tr


def _steps(tr, world, n, grab=None):
    """n one_step_raw calls; (loss, gradient arena, parameter arena) after each.  grab: receives what one_step is handed."""
    out = []
    if grab is not None:
        orig = tr.one_step

        def spy(x, image, boxes, nums, **k):
            torch.cuda.synchronize()                                      # x is still being written on the geometry side stream
            grab.append((x.clone(), image.clone(), boxes.clone(), torch.as_tensor(nums).clone(), k["geom"]["cnt"].clone()))
            return orig(x, image, boxes, nums, **k)
        tr.one_step = spy
    for _ in range(n):
        tr.one_step_raw(world["geo"], world["batch"])
        torch.cuda.synchronize()
        out.append((tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone()))
    return out


def test_trainer_block_off_is_the_plain_step(world):
    plain = _steps(_trainer(_tiny_cfg()), world, 2)
    tr = _trainer(_tiny_cfg(augment_paste=_paste_block(world, enabled=False)))
    assert tr.paste is None and tr._paste_dev is None and tr._paste_bank is None
    off = _steps(tr, world, 2)
    assert tr._paste_image_buf is None and tr.aug_calls == 0 and tr.last_paste == [] and np.isfinite(float(plain[0][0]))
    assert not [k for st in tr._geo_sets.values() for k in st if k == "paste"]
    for s in range(2):
        for u, v in zip(plain[s], off[s]):
            assert torch.equal(u, v)
    with pytest.raises(ValueError):
        pkg("train").Train(_tiny_cfg(augment_paste=_paste_block(world, enabled=False, max_candidates=17)))
    with pytest.raises(ValueError):                                       # a bank of another image size, when the trainer is built
        pkg("train").Train(_tiny_cfg(augment_paste=_paste_block(world), image_width=130))


def test_trainer_hands_the_loss_the_host_plans_labels_and_pastes_points_and_image(world):
    P, T = pkg("paste"), pkg("train")
    cfg = _tiny_cfg(augment_paste=_paste_block(world))
    tr = _trainer(cfg)
    original = world["batch"]["image"].clone()
    seen = []
    a = _steps(tr, world, 2, seen)
    parsed = T.parse_paste_config(cfg)
    batch, bank = world["batch"], world["bank"]
    pasted = 0
    for s in range(2):
        for f in range(2):
            n0 = int(batch["num_bboxes"][f])
            plan = P.draw(parsed, 9, 0, s, f, bank, batch["bboxes"][f].numpy(), n0, int(batch["points"][f].shape[0]), tiny_crt(), cfg)
            want_boxes, want_num = P.append_labels(batch["bboxes"][f].numpy(), n0, plan)
            assert int(seen[s][3][f]) == want_num and np.array_equal(seen[s][2][f].numpy(), want_boxes)
            assert np.array_equal(seen[s][1][f].cpu().numpy(), P.paste_image(original[f].cpu().numpy(), plan, bank))
            if s == 1:
                assert tr.last_paste[f] == plan["rows"]
            pasted += len(plan["rows"])
    assert pasted >= 3                                                    # (from the host plans alone)
    assert torch.equal(batch["image"], original)                          # the batch's image is not written
    assert tr._paste_image_buf is not None and tr.aug_calls == 2
    plain = _steps(_trainer(_tiny_cfg()), world, 1)
    assert not torch.equal(a[0][0], plain[0][0])
    # the voxel input is that of the pasted points: geometry_async(paste=plans) == geometry_async of the host statement's points
    plans = [P.draw(parsed, 9, 0, 0, f, bank, batch["bboxes"][f].numpy(), int(batch["num_bboxes"][f]), int(batch["points"][f].shape[0]), tiny_crt(), cfg)
             for f in range(2)]
    x, g = tr.geometry_async(world["geo"], batch["points"], paste=plans)
    torch.cuda.synchronize()
    assert torch.equal(x, seen[0][0]) and torch.equal(g["cnt"], seen[0][4])
    g = {"cnt": g["cnt"].clone()}                                         # (the geometry sets are reused two calls on)
    host_pts = [torch.from_numpy(P.paste_points(batch["points"][f].cpu().numpy(), plans[f], bank)).cuda() for f in range(2)]
    x2, g2 = tr.geometry_async(world["geo"], host_pts)
    torch.cuda.synchronize()
    assert torch.equal(x, x2) and torch.equal(g["cnt"], g2["cnt"])
    x3, g3 = tr.geometry_async(world["geo"], batch["points"])
    torch.cuda.synchronize()
    assert not torch.equal(g3["cnt"], g["cnt"])
    with pytest.raises(ValueError):
        tr.geometry_async(world["geo"], batch["points"], paste=plans[:1])
    torch.cuda.synchronize()


def test_trainer_counter_ticks_once_and_the_other_blocks_draw_what_they_draw_alone(world):
    A, T = pkg("augment"), pkg("train")
    for over in (dict(augment_paste=_paste_block(world)), dict(augment_paste=_paste_block(world), augment=dict(BEV), augment_image=dict(IMG))):
        tr = _trainer(_tiny_cfg(**over))
        drawn = []
        orig = tr.geometry_async

        def spy(*a, _orig=orig, **k):
            drawn.append((k.get("augment"), k.get("image_augment")))
            return _orig(*a, **k)
        tr.geometry_async = spy
        _steps(tr, world, 3)
        assert tr.aug_calls == 3
        if "augment" in over:
            cfg = _tiny_cfg(**over)
            for s in range(3):
                for f in range(2):                                        # the `augment` block's parameters are what they are without paste
                    want = A.draw(T.parse_augment_config(cfg), 9, 0, s, f)
                    assert np.array_equal(drawn[s][0][f]["a"], want["a"]) and drawn[s][0][f]["drop_key"] == want["drop_key"]
                    wi = pkg("augment_image").draw(T.parse_image_augment_config(cfg), 9, 0, s, f, 128, 96)
                    assert np.array_equal(drawn[s][1][f]["q"], wi["q"])
        else:
            assert all(d == (None, None) for d in drawn)


def test_trainer_deterministic_runs_agree_and_a_checkpoint_resumes(world, tmp_path):
    cfg = _tiny_cfg(augment_paste=_paste_block(world), augment=dict(BEV))
    ta = _trainer(cfg)
    a1 = _steps(ta, world, 1)
    path = os.path.join(str(tmp_path), "ckpt.pt")
    ta.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert ck["aug_calls"] == 1 and not [k for k in ck if "paste" in k]   # no new field
    a2 = _steps(ta, world, 1)
    b = _steps(_trainer(copy.deepcopy(cfg)), world, 2)
    for u, v in zip(a1[0] + a2[0], b[0] + b[1]):                          # two trainers, same seed, bit for bit after two steps
        assert torch.equal(u, v)
    assert not torch.equal(a1[0][0], a2[0][0])
    tr2 = _trainer(copy.deepcopy(cfg))
    tr2.load_checkpoint(path)
    assert tr2.aug_calls == 1
    got = _steps(tr2, world, 1)[0]
    for u, v in zip(a2[0], got):
        assert torch.equal(u, v)


def test_trainer_hip_graphs_batch1_equals_eager(world):
    """The two launches sit outside the captured graphs: three steps at batch 1 with hip_graphs equal the eager ones bit for bit."""
    FL = pkg("frame_loader")
    full = world["batch"]
    one = FL.Batch(bboxes=full["bboxes"][:1], num_bboxes=full["num_bboxes"][:1], crt=None)
    one["points"], one["image"] = full["points"][:1], full["image"][:1]
    small = dict(world, batch=one)
    runs = {}
    for graphs in (False, True):
        tr = _trainer(_tiny_cfg(augment_paste=_paste_block(world), batch_size=1, hip_graphs=graphs))
        assert tr.model.graphs_wanted(1) == graphs
        runs[graphs] = _steps(tr, small, 3)
        assert tr.aug_calls == 3 and len(tr.last_paste) == 1
        if graphs:
            assert tr.model._graphs is not None and len(tr.model._graphs.sets) >= 1 and not tr.model._graphs.disabled
    for s in range(3):
        assert torch.equal(runs[False][s][0], runs[True][s][0]), s
    assert not torch.equal(runs[False][0][0], runs[False][1][0])


def test_evaluation_is_never_pasted(world):
    tr = _trainer(_tiny_cfg(augment_paste=_paste_block(world)))
    batch = world["batch"]
    x, geom = tr.geometry_async(world["geo"], batch["points"], crts=batch.get("crt"))
    value, _, _ = tr.get_loss_value(x, batch["image"], batch["bboxes"], batch["num_bboxes"], geom=geom)
    torch.cuda.synchronize()
    plain = _trainer(_tiny_cfg())
    x0, geom0 = plain.geometry_async(world["geo"], batch["points"], crts=batch.get("crt"))
    value0, _, _ = plain.get_loss_value(x0, batch["image"], batch["bboxes"], batch["num_bboxes"], geom=geom0)
    torch.cuda.synchronize()
    assert value == value0 and torch.equal(x, x0) and tr.aug_calls == 0 and tr._paste_image_buf is None and tr.last_paste == []

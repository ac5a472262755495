"""GPU: the camera visibility mask (csrc/camera_mask.hip, ops.camera_mask_points_batch, FrameGeometry.mask_points, Train with the
`camera_mask` block) against the host statements of visibility.py."""
import copy
import os

import numpy as np
import pytest
import torch

from _paste_util import Frames, label_row, make_frame, tiny_crt
from _util import golden_cfg, load_golden, pkg
from _visibility_util import LIM_TINY, bits, lim_of, pasted_world

pytestmark = pytest.mark.gpu

HW = (96, 128)
GUARD = 0x7FC0BEEF                                                        # a NaN with a payload: guard rows must come back bit for bit


def _crts(B):
    """B different matrices: the dyadic tiny one, the KITTI-like one scaled to the tiny image, and perturbed copies."""
    base = [np.asarray(tiny_crt(), dtype=np.float32).reshape(4, 3)]
    k = np.asarray(pkg("calib").kitti_like_crt(), dtype=np.float64).reshape(4, 3).copy()
    k[:, 0] *= 128.0 / 1242
    k[:, 1] *= 96.0 / 375
    base.append(k.astype(np.float32))
    rng = np.random.RandomState(77)
    while len(base) < B:
        base.append((base[len(base) % 2] * (1.0 + 0.05 * rng.standard_normal((4, 3)))).astype(np.float32))
    return np.stack(base[:B], 0)


def _frame(n, seed):
    """n rows in and around the tiny range, with NaN (payload), +inf and -inf rows among them."""
    rng = np.random.RandomState(seed)
    pts = (rng.rand(n, 3) * np.array([20.0, 10.0, 4.0]) + np.array([-2.0, -5.0, -2.8])).astype(np.float32)
    if n >= 200:
        pts.view(np.uint32)[5] = [0x7FC12345, 0x3F800000, 0xFFC00001]
        pts.view(np.uint32)[6] = [0x40800000, 0x7F812345, 0x00000000]
        pts[7], pts[8], pts[9] = np.inf, -np.inf, [np.inf, 1.0, -1.0]
    return pts


def _occ(m, seed):
    rng = np.random.RandomState(seed)
    x0, y0 = rng.randint(0, 100, m), rng.randint(0, 70, m)
    return np.stack([x0, y0, x0 + rng.randint(0, 60, m), y0 + rng.randint(0, 40, m), rng.uniform(1.0, 12.0, m)], 1).astype(np.float32)


def _run(frames, crts, lim, ulim, vlim, mode, fov, occs, in_place=False):
    """One ops call over the frames, every input 12 bytes (one row) into a larger buffer, every output with guard rows in front of
    it and behind row n_b up to a capacity of n_b + 3: (outputs [n_b,3] as uint32, the guards' verdict)."""
    ops = pkg("ops")
    ins, outs, bufs = [], [], []
    for p in frames:
        n = len(p)
        src = torch.full((n + 2, 3), float("nan"), device="cuda")
        src[1:n + 1] = torch.from_numpy(p).cuda()
        ins.append(src[1:n + 1])
        if in_place:
            buf = src
        else:
            buf = torch.from_numpy(np.full((n + 5, 3), GUARD, dtype=np.uint32).view(np.float32)).cuda()
        bufs.append(buf)
        outs.append(buf[1:n + 1] if in_place else buf[1:n + 4])          # (not in place: an output with more rows than the frame)
    ops.camera_mask_points_batch(ins, crts, lim, ulim, vlim, mode, fov, occs, outs)
    torch.cuda.synchronize()
    got, clean = [], True
    for p, buf in zip(frames, bufs):
        n = len(p)
        raw = buf.cpu().numpy().view(np.uint32)
        got.append(raw[1:n + 1])
        if not in_place:
            clean = clean and (raw[0] == GUARD).all() and (raw[n + 1:] == GUARD).all()
    return got, clean


NS = {1: [5000], 3: [1024, 0, 257], 8: [0, 1, 255, 256, 257, 1023, 1025, 5000]}


@pytest.mark.parametrize("B", [1, 3, 8])
def test_kernel_equals_host_statement_bitwise(B):
    V = pkg("visibility")
    lim, crts = lim_of(LIM_TINY), _crts(B)
    frames = [_frame(n, 100 + b) for b, n in enumerate(NS[B])]
    ms = [[16], [0, 1, 16], [16, 1, 0, 5, 16, 0, 1, 16]][{1: 0, 3: 1, 8: 2}[B]]
    occs = [_occ(m, 200 + b) for b, m in enumerate(ms)]
    hidden_rows = masked_rows = 0
    for mode, (ulim, vlim) in ((0, HW), (1, HW[::-1])):                   # compat's limits come swapped (FrameGeometry.limits)
        for fov in (False, True):
            for with_occ in (False, True):
                oc = occs if with_occ else None
                want = [V.mask_points(p, crts[b], lim, ulim, vlim, mode, fov, occs[b] if with_occ else None) for b, p in enumerate(frames)]
                for in_place in (False, True):
                    got, clean = _run(frames, crts, lim, ulim, vlim, mode, fov, oc, in_place)
                    assert clean, (mode, fov, with_occ)
                    for b in range(B):
                        assert np.array_equal(got[b], bits(want[b])), (mode, fov, with_occ, in_place, b)
                if not fov and not with_occ:                              # both off: a copy
                    assert all(np.array_equal(bits(w), bits(p)) for w, p in zip(want, frames))
                gone = sum(int((bits(w) != bits(p)).any(1).sum()) for w, p in zip(want, frames))
                masked_rows += gone if fov and not with_occ else 0
                hidden_rows += gone if with_occ and not fov else 0
    total = 2 * sum(NS[B])
    if total:                                                             # both rules decide both ways on these frames
        assert 0.05 * total < masked_rows < 0.95 * total and 0 < hidden_rows < 0.9 * total


def test_kernel_more_than_eight_frames_and_the_nan_payload():
    V, ops = pkg("visibility"), pkg("ops")
    lim, crts = lim_of(LIM_TINY), _crts(11)
    frames = [_frame(300 + 7 * b, 300 + b) for b in range(11)]
    occs = [_occ(b % 3, 400 + b) for b in range(11)]
    outs = ops.camera_mask_points_batch([torch.from_numpy(p).cuda() for p in frames], crts, lim, 128, 96, 1, True, occs)     # out_list None: in place
    torch.cuda.synchronize()
    for b, p in enumerate(frames):
        want = V.mask_points(p, crts[b], lim, 128, 96, 1, True, occs[b])
        assert np.array_equal(outs[b].cpu().numpy().view(np.uint32), bits(want))
    keep = V.fov_keep(frames[0], crts[0], lim, 128, 96, 1)
    assert not keep[5] and np.isposinf(V.mask_points(frames[0], crts[0], lim, 128, 96, 1, True, None)[5]).all()     # a NaN row is not seen ...
    got, _ = _run(frames[:1], crts[:1], lim, 128, 96, 1, False, occs[:1])
    assert got[0][5].tolist() == [0x7FC12345, 0x3F800000, 0xFFC00001]                                              # ... and keeps its payload where it stays


def test_kernel_refuses_bad_arguments():
    ops, Hh = pkg("ops"), pkg("_hip")
    lim, crt = lim_of(LIM_TINY), _crts(2)
    buf = torch.zeros((100, 3), device="cuda")
    a, b = buf[0:20], buf[30:50]
    ok = np.array([[1.0, 2.0, 3.0, 4.0, 5.0]], dtype=np.float32)

    def call(ins, outs, occ=None, crts=crt):
        ops.camera_mask_points_batch(ins, crts[:len(ins)], lim, 128, 96, 1, True, occ, outs)

    call([a, b], [a, b])                                                  # in place: allowed
    call([a, b], [buf[60:80], buf[80:100]], [ok, None])
    for ins, outs in (([a, b], [b, a]),                                   # an output on the OTHER frame's input
                      ([a, b], [buf[10:30], torch.empty((20, 3), device="cuda")]),      # partial overlap with its own input
                      ([a, b], [buf[25:45], torch.empty((20, 3), device="cuda")]),      # partial overlap with the other input
                      ([a, b], [buf[60:80], buf[70:90]])):                # two outputs overlap
        with pytest.raises(Hh.DcfError):
            call(ins, outs)
    for bad in ([[np.nan, 2, 3, 4, 5]], [[1, 2, np.inf, 4, 5]], [[1, 2, 3, 4, -np.inf]], [[3, 2, 1, 4, 5]], [[1, 4, 3, 2, 5]]):
        with pytest.raises(Hh.DcfError):
            call([a, b], [a, b], [None, np.array(bad, dtype=np.float32)])
    with pytest.raises(Hh.DcfError):
        call([a, b], [a, b], [np.zeros((17, 5), dtype=np.float32), None])
    with pytest.raises(Hh.DcfError):
        call([a, b], [a])
    with pytest.raises(Hh.DcfError):
        call([a, b], [a, buf[30:40]])                                     # an output smaller than its frame
    with pytest.raises(Hh.DcfError):
        call([a.cpu(), b], [a, b])
    with pytest.raises(Hh.DcfError):
        ops.camera_mask_points_batch([a], crt[:1], lim, 128, 96, 7, True, None, [a])
    torch.cuda.synchronize()
    assert pkg("_hip").lib().dcf_version() == 202


def test_edges_with_the_dyadic_calibration():
    """tiny_crt: u = 64 - 60 y / x, v = 48 - 60 z / x, a2 = x.  (4, -1, 0) sits on u = 79, v = 48, a2 = 4 exactly."""
    V, ops = pkg("visibility"), pkg("ops")
    crt, lim = np.asarray(tiny_crt(), dtype=np.float32).reshape(1, 4, 3), lim_of(LIM_TINY)
    p = np.array([[4.0, -1.0, 0.0]], dtype=np.float32)
    u, v, a2 = V.project_chain(p, crt[0])
    assert (u[0], v[0], a2[0]) == (79.0, 48.0, 4.0)
    below, above = np.nextafter(np.float32(4), np.float32(0)), np.nextafter(np.float32(4), np.float32(8))
    cases = [((79, 40, 90, 60, 3), True), ((70, 40, 79, 60, 3), False),  # u == x0 is hidden, u == x1 is not
             ((70, 48, 90, 60, 3), True), ((70, 40, 90, 48, 3), False),  # v likewise
             ((70, 40, 90, 60, 4), False), ((70, 40, 90, 60, below), True), ((70, 40, 90, 60, above), False),     # a2 == D is not, its successor is
             ((79, 48, 79, 48, 3), False), ((79, 48, np.nextafter(np.float32(79), np.float32(80)), np.nextafter(np.float32(48), np.float32(49)), 3), True)]
    for q, hidden in cases:
        occ = np.array([q], dtype=np.float32)
        dev = torch.from_numpy(p).cuda()
        ops.camera_mask_points_batch([dev], crt, lim, 128, 96, 1, False, [occ])
        got = dev.cpu().numpy()
        assert bool(np.isposinf(got).all()) == hidden and bool(V.hidden(u, v, a2, occ)[0]) == hidden, q
        assert hidden or np.array_equal(got, p)
    # the successor of a2 against D = 4: the row one ulp deeper goes
    deeper = np.array([[above, -1.0, 0.0]], dtype=np.float32)
    dev = torch.from_numpy(deeper).cuda()
    ops.camera_mask_points_batch([dev], crt, lim, 128, 96, 1, False, [np.array([[0, 0, 128, 96, 4]], dtype=np.float32)])
    assert np.isposinf(dev.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ the mask and its consumers
def _tiny_cfg(**over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dtype="f32", loss_reduction="mean",
                    bn_mode="eval", learning_rate=1e-3, batch_size=2, loss_sampling="device", loss_seed=5, deterministic=True))
    cfg["lidar_module"] = dict(cfg["lidar_module"], out_feature2=64, out_feature3=128, out_feature4=192, out_feature5=256)   # deterministic fusion widths
    cfg["fusion"] = dict(enabled=True, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("mode", ["compat", "correct"])
def test_the_mask_is_the_projections_own_predicate_and_the_voxeliser_sees_the_kept_rows(mode):
    """project_filter_batch of the fov-masked frames equals that of the originals bit for bit (uv, xyz, counts); the voxel grid of the
    masked frames (compat fp32 and the NHWC image) equals the grid of the kept rows alone."""
    V, D, ops, Hh = pkg("visibility"), pkg("data_import_carla"), pkg("ops"), pkg("_hip")
    cfg = _tiny_cfg(projection_mode=mode)
    crts = _crts(3)
    geo = D.FrameGeometry(cfg, crts[0])
    frames = [_frame(n, 500 + b) for b, n in enumerate((1500, 257, 2048))]
    dev = [torch.from_numpy(p).cuda() for p in frames]
    masked = geo.mask_points(dev, [None, crts[1], crts[2]], True)
    torch.cuda.synchronize()
    ulim, vlim = geo.limits()
    keeps = [V.fov_keep(p, crts[b], geo.grid.lim, ulim, vlim, geo.proj_mode) for b, p in enumerate(frames)]
    for b, p in enumerate(frames):
        assert np.array_equal(dev[b].cpu().numpy().view(np.uint32), bits(p))                       # out=None: the frames are not written
        assert np.array_equal(masked[b].cpu().numpy().view(np.uint32), bits(V.mask_points(p, crts[b], geo.grid.lim, ulim, vlim, geo.proj_mode, True, None)))
    assert all(0 < k.sum() < len(k) for k in keeps)
    mp = 2048
    res = []
    for pts in (dev, masked):
        xyz, uv, cnt = torch.zeros((3, mp, 3), device="cuda"), torch.zeros((3, mp, 2), device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
        ops.project_filter_batch(pts, geo.grid.lim, crts, ulim, vlim, geo.proj_mode, uv, xyz, cnt)
        res.append((xyz, uv, cnt))
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res[0], res[1]))
    assert res[0][2].tolist() == [int(k.sum()) for k in keeps]
    Cz, L, W = geo.grid.dims
    kept = [torch.from_numpy(np.ascontiguousarray(p[k])).cuda() for p, k in zip(frames, keeps)]
    grids = [geo.voxelize_batch(pts, torch.empty((3, Cz, L, W), device="cuda")).clone() for pts in (masked, kept, dev)]
    assert torch.equal(grids[0], grids[1]) and not torch.equal(grids[0], grids[2])
    if geo.voxel_mode == Hh.VOXEL_COMPAT:
        nhwc = [geo.voxelize_batch(pts, torch.empty((3, L, W, Cz), dtype=torch.bfloat16, device="cuda"), Hh.BF16).clone()
                for pts in (masked, kept)]
        assert torch.equal(nhwc[0], nhwc[1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["tiny", "kitti"])
def test_paste_then_mask(which):
    """Pasted on the device, then masked with the plan's occluders: every surviving row whose pixel a record's rectangle holds is not
    deeper than that record's D; every appended row that is hidden is hidden by the record of ANOTHER object; no object hides its own."""
    V, ops = pkg("visibility"), pkg("ops")
    bank, plan, pasted_host, n, crt, lim6, hw = pasted_world(which)
    crt32 = np.asarray(crt, dtype=np.float32).reshape(4, 3)
    scene = np.ascontiguousarray(pasted_host[:n])                         # (the removed points are +inf rows already: pasting leaves them)
    out = torch.empty((len(pasted_host), 3), device="cuda")
    dev = ops.paste_points_batch([torch.from_numpy(scene).cuda()], [plan], torch.from_numpy(bank["points"]).cuda(), [out])[0]
    occ = V.occluders(plan, bank, crt)
    ops.camera_mask_points_batch([dev], crt32[None], lim_of(lim6), hw[1], hw[0], 1, False, [occ])
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(bits(got), bits(V.mask_points(pasted_host, crt32, lim_of(lim6), hw[1], hw[0], 1, False, occ)))
    u, v, a2 = V.project_chain(got, crt32)
    with np.errstate(invalid="ignore"):
        for q in occ:
            inside = (u >= q[0]) & (u < q[2]) & (v >= q[1]) & (v < q[3])
            assert (a2[inside] <= q[4]).all()
    pu, pv, pa = V.project_chain(pasted_host, crt32)
    gone = (bits(got) != bits(pasted_host)).any(1)
    first, by_others = n, 0
    for k, r in enumerate(plan["rows"]):
        a = int(plan["append"][k, 1])
        sl = slice(first, first + a)
        j = plan["patch_rows"].index(r)
        assert not V.hidden(pu[sl], pv[sl], pa[sl], occ[j:j + 1]).any()
        others = np.delete(occ, j, 0)
        assert np.array_equal(gone[sl], V.hidden(pu[sl], pv[sl], pa[sl], others))
        by_others, first = by_others + int(gone[sl].sum()), first + a
    assert gone[:n].sum() >= 100
    print("%s: %d scene rows hidden, %d appended rows hidden by another object's patch" % (which, int(gone[:n].sum()), by_others))


# ------------------------------------------------------------------------------------------------ the trainer
SLOTS = [(3.0, -2.5), (8.0, 2.5), (13.0, -2.5), (13.0, 2.5), (3.0, 2.5), (8.0, -2.5)]
BEV = dict(enabled=True, seed=9, rotation_deg=20.0, scale=[0.95, 1.05], flip_prob=0.5, point_drop=[0.05, 0.2])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The small world of the pasting tests: a bank of 8 objects (two frames, four cars each, on the slots of a 16 m x 8 m grid) saved
    as .npz, and a staged batch of two frames of about 1500 points with one NEAR label each -- pasted objects land behind it."""
    B, D, FL = pkg("objbank"), pkg("data_import_carla"), pkg("frame_loader")
    cfg = _tiny_cfg()
    src = [make_frame([label_row(x, y, -1.0, 0.2 * f + 0.1 * i) for i, (x, y) in enumerate(SLOTS[:4])], [30, 25, 35, 28], 600, LIM_TINY, HW, 60 + f)
           for f in range(2)]
    bank = B.build(Frames(src, tiny_crt()), cfg)
    assert len(bank["boxes"]) == 8
    path = os.path.join(str(tmp_path_factory.mktemp("mask")), "bank.npz")
    B.save(path, bank)
    frames = [make_frame([label_row(SLOTS[4 + f][0], SLOTS[4 + f][1], -1.0, 0.3)], [30], 1400, LIM_TINY, HW, 70 + f) for f in range(2)]
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
            grab.append((x.clone(), image.clone(), boxes.clone(), torch.as_tensor(nums).clone(), k["geom"]["cnt"].clone(), k["geom"]))
            return orig(x, image, boxes, nums, **k)
        tr.one_step = spy
    for _ in range(n):
        tr.one_step_raw(world["geo"], world["batch"])
        torch.cuda.synchronize()
        out.append((tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone()))
    return out


@pytest.mark.parametrize("pasting", [False, True])
def test_trainer_block_off_is_the_step_without_it(world, pasting):
    base = dict(augment_paste=_paste_block(world)) if pasting else {}
    plain = _steps(_trainer(_tiny_cfg(**base)), world, 2)
    for block in (None, {}, {"fov_crop": False, "paste_occlusion": False}):
        tr = _trainer(_tiny_cfg(camera_mask=block, **base))
        assert tr.camera_mask is None
        off = _steps(tr, world, 2)
        assert tr.last_masked == [] and not [k for st in tr._geo_sets.values() for k in st if k == "mask"]
        for s in range(2):
            for u, v in zip(plain[s], off[s]):
                assert torch.equal(u, v)
    T = pkg("train")
    for bad in ({"fov": True}, {"fov_crop": 1}, {"paste_occlusion": True} if not pasting else {"paste_occlusion": "yes"}):
        with pytest.raises(ValueError):                                   # when the trainer is built
            T.Train(_tiny_cfg(camera_mask=bad, **base))
    if pasting:
        with pytest.raises(ValueError):
            T.Train(_tiny_cfg(camera_mask={"paste_occlusion": True}, augment_paste=_paste_block(world, paste_image=False)))


def _kept_rows_input(tr, world, keeps):
    """x_lidar and the projection counts of the frames' kept rows alone, through a trainer WITHOUT the block."""
    batch = world["batch"]
    kept = [p[torch.from_numpy(k).cuda()].contiguous() for p, k in zip(batch["points"], keeps)]
    x, g = tr.geometry_async(world["geo"], kept, crts=batch.get("crt"))
    torch.cuda.synchronize()
    return x.clone(), g["cnt"].clone()


def test_trainer_fov_crop_in_the_step_and_in_evaluation(world):
    V, T = pkg("visibility"), pkg("train")
    geo, batch = world["geo"], world["batch"]
    ulim, vlim = geo.limits()
    keeps = [V.fov_keep(p.cpu().numpy(), geo.crt, geo.grid.lim, ulim, vlim, geo.proj_mode) for p in batch["points"]]
    assert all(0.2 * len(k) < k.sum() < 0.95 * len(k) for k in keeps)
    plain = _trainer(_tiny_cfg())
    want_x, want_cnt = _kept_rows_input(plain, world, keeps)
    x0, g0 = plain.geometry_async(geo, batch["points"], crts=batch.get("crt"))
    torch.cuda.synchronize()
    assert torch.equal(g0["cnt"], want_cnt) and not torch.equal(x0, want_x)      # the projection counts are unchanged, the BEV input is not
    cfg = _tiny_cfg(camera_mask={"fov_crop": True})
    tr = _trainer(cfg)
    original = [p.clone() for p in batch["points"]]
    seen = []
    _steps(tr, world, 1, seen)
    assert torch.equal(seen[0][0], want_x) and torch.equal(seen[0][4], want_cnt)
    st = seen[0][5]["_set"]
    for b, p in enumerate(original):
        want = V.mask_points(p.cpu().numpy(), geo.crt, geo.grid.lim, ulim, vlim, geo.proj_mode, True, None)
        assert np.array_equal(st["mask"][b, :len(want)].cpu().numpy().view(np.uint32), bits(want))
        assert torch.equal(batch["points"][b].view(torch.int32), p.view(torch.int32))          # the staged frames are not written
    # evaluation: train.evaluate goes through geometry_async, which crops as the step does
    calls = []
    orig = tr.geometry_async

    def spy(*a, **k):
        x, g = orig(*a, **k)
        torch.cuda.synchronize()
        calls.append((x.clone(), g["cnt"].clone()))
        return x, g
    tr.geometry_async = spy

    class Data(object):
        geometry = geo
    tester = T.make_tester(tr.model, cfg)
    T.evaluate(tr, tester, Data(), [batch], max_batches=1)
    assert len(calls) == 1 and torch.equal(calls[0][0], want_x) and torch.equal(calls[0][1], want_cnt)
    # a frame over max_num_pc takes the allocating path, as `augment` does
    big = [torch.cat([p, p], 0) for p in batch["points"]]
    xb, gb = orig(geo, big, crts=batch.get("crt"))
    xp, gp = plain.geometry_async(geo, [torch.cat([p[torch.from_numpy(k).cuda()]] * 2, 0) for p, k in zip(batch["points"], keeps)], crts=batch.get("crt"))
    torch.cuda.synchronize()
    assert torch.equal(xb, xp) and torch.equal(gb["cnt"], gp["cnt"])


def test_trainer_paste_occlusion(world):
    V, P, T = pkg("visibility"), pkg("paste"), pkg("train")
    geo, batch, bank = world["geo"], world["batch"], world["bank"]
    cfg = _tiny_cfg(augment_paste=_paste_block(world), camera_mask={"fov_crop": True, "paste_occlusion": True})
    tr = _trainer(cfg)
    parsed = T.parse_paste_config(cfg)
    ulim, vlim = geo.limits()
    original = batch["image"].clone()
    seen = []
    _steps(tr, world, 2, seen)
    dropped = hidden = 0
    for s in range(2):
        for f in range(2):
            n0, pts = int(batch["num_bboxes"][f]), batch["points"][f].cpu().numpy()
            drawn = P.draw(parsed, 9, 0, s, f, bank, batch["bboxes"][f].numpy(), n0, len(pts), tiny_crt(), cfg)
            plan = V.drop_covering(drawn, batch["bboxes"][f].numpy(), n0, tiny_crt(), bank)
            want_boxes, want_num = P.append_labels(batch["bboxes"][f].numpy(), n0, plan)
            assert int(seen[s][3][f]) == want_num and np.array_equal(seen[s][2][f].numpy(), want_boxes)      # the loss sees the filtered plan's labels
            assert np.array_equal(seen[s][1][f].cpu().numpy(), P.paste_image(original[f].cpu().numpy(), plan, bank))
            pasted = P.paste_points(pts, plan, bank)
            occ = V.occluders(plan, bank, tiny_crt())
            want = V.mask_points(pasted, geo.crt, geo.grid.lim, ulim, vlim, geo.proj_mode, True, occ)
            got = seen[s][5]["_set"]["paste"][f, :len(want)].cpu().numpy() if s == 1 else None      # (the last step's set is still as it was left)
            if got is not None:
                assert np.array_equal(got.view(np.uint32), bits(want))
                assert tr.last_paste[f] == plan["rows"] and tr.last_masked[f] == (len(plan["patches"]), len(drawn["rows"]) - len(plan["rows"]))
            dropped += len(drawn["rows"]) - len(plan["rows"])
            u, v, a2 = V.project_chain(pasted, geo.crt)
            hidden += int(V.hidden(u, v, a2, occ).sum())
    assert dropped >= 1 and hidden >= 10                                  # (from the host statements alone: both halves act in this world)
    assert torch.equal(batch["image"], original) and tr.aug_calls == 2
    # the BEV input is that of the host statement's points
    plans = [V.drop_covering(P.draw(parsed, 9, 0, 0, f, bank, batch["bboxes"][f].numpy(), int(batch["num_bboxes"][f]), int(batch["points"][f].shape[0]), tiny_crt(), cfg),
                             batch["bboxes"][f].numpy(), int(batch["num_bboxes"][f]), tiny_crt(), bank) for f in range(2)]
    host = []
    for f in range(2):
        pasted = P.paste_points(batch["points"][f].cpu().numpy(), plans[f], bank)
        host.append(torch.from_numpy(V.mask_points(pasted, geo.crt, geo.grid.lim, ulim, vlim, geo.proj_mode, True, V.occluders(plans[f], bank, tiny_crt()))).cuda())
    x2, g2 = _trainer(_tiny_cfg()).geometry_async(geo, host)
    torch.cuda.synchronize()
    assert torch.equal(seen[0][0], x2) and torch.equal(seen[0][4], g2["cnt"])


def test_trainer_deterministic_runs_agree_and_a_checkpoint_resumes(world, tmp_path):
    cfg = _tiny_cfg(augment_paste=_paste_block(world), augment=dict(BEV), camera_mask={"fov_crop": True, "paste_occlusion": True})
    ta = _trainer(cfg)
    a1 = _steps(ta, world, 1)
    path = os.path.join(str(tmp_path), "ckpt.pt")
    ta.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert ck["aug_calls"] == 1 and not [k for k in ck if "mask" in k]    # no new field
    a2 = _steps(ta, world, 1)
    b = _steps(_trainer(copy.deepcopy(cfg)), world, 2)
    for u, v in zip(a1[0] + a2[0], b[0] + b[1]):                          # two trainers, same seed, bit for bit after two steps
        assert torch.equal(u, v)
    assert not torch.equal(a1[0][0], a2[0][0])
    tr2 = _trainer(copy.deepcopy(cfg))
    tr2.load_checkpoint(path)
    got = _steps(tr2, world, 1)[0]
    for u, v in zip(a2[0], got):
        assert torch.equal(u, v)
    off = _steps(_trainer(_tiny_cfg(augment_paste=_paste_block(world), augment=dict(BEV))), world, 1)
    assert not torch.equal(off[0][0], a1[0][0])                           # the block acts


def test_datasets_read_the_switch(tmp_path):
    """The non-raw items of the datasets call FrameGeometry.mask_points (checked above) when fov_crop is set: the switch is read, and
    validated, when the dataset is built."""
    K = pkg("data_import_kitti")
    cfg = _tiny_cfg(camera_mask={"fov_crop": True})
    assert K.KittiDataset(cfg, root=str(tmp_path))._fov_crop and not K.KittiDataset(_tiny_cfg(), root=str(tmp_path))._fov_crop
    with pytest.raises(ValueError):
        K.KittiDataset(_tiny_cfg(camera_mask={"fov_crop": 1}), root=str(tmp_path))

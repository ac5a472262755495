"""Train-time object pasting without a GPU (objbank.py, paste.py, train.parse_paste_config): the bank builder,
the stateless sampler with its caps and its vectorised collision test, the destination rectangle under a shifted calibration, and the
host statements of the two kernels against independent restatements."""
import math
import os

import numpy as np
import pytest
import torch

from _paste_util import CAR, RANGE, Frames, label_row, make_frame, plan_of, random_bank, tiny_crt
from _util import M64, mix64, pkg

HW = (96, 128)
LIM6 = (0.0, 16.0, -6.0, 6.0, -2.4, 0.8)
CFG = {"seed": 3, "bank": "unused", "target_objects": 15, "max_candidates": 16, "margin": 0.0, "paste_image": True}


def _three_frames():
    """Three frames, three labels each: a car in front with 30..40 points, one with fewer than min_points (3), one BEHIND the camera
    (x < 0: every corner has a2 <= 0) with 20."""
    items = []
    for f in range(3):
        rows = [label_row(8.0 + f, 1.0 - f, -1.0, 0.3 + 0.5 * f), label_row(14.0, -3.0 + f, -1.0, 2.0 - f), label_row(-6.0 - f, 0.5 * f, -1.0, 0.25 * f)]
        items.append(make_frame(rows, [30 + 5 * f, 3, 20], 400, (-10.0, 16.0, -6.0, 6.0, -2.4, 0.8), HW, f))
    return Frames(items, tiny_crt())


# ------------------------------------------------------------------------------------------------ bank
def test_bank_holds_exactly_the_points_inside_each_box_and_its_patch():
    B, P = pkg("objbank"), pkg("paste")
    ds = _three_frames()
    bank = B.build(ds, dict(RANGE), min_points=5)
    assert bank["boxes"].shape == (6, 9) and bank["source"].tolist() == [[0, 0], [0, 2], [1, 0], [1, 2], [2, 0], [2, 2]]      # row 1 has 3 points
    assert bank["image_hw"].tolist() == list(HW) and bank["points"].dtype == np.float32 and bank["patch"].dtype == np.uint8
    for k in range(6):
        f, r = (int(v) for v in bank["source"][k])
        item = ds[f]
        pts = item["lidar_points"].numpy()
        row = item["bboxes"][r].numpy()
        assert np.array_equal(bank["boxes"][k], row)
        own = bank["points"][bank["point_start"][k]:bank["point_start"][k + 1]]
        mask = P.inside_mask(pts, P.record(row, 0.0))
        assert len(own) >= 5 and np.array_equal(own.view(np.uint32), pts[mask].view(np.uint32))         # exactly those, in frame order, unchanged
        assert mask.sum() == [30, 20, 35, 20, 40, 20][k]
        x0, y0, w, h = (int(v) for v in bank["rect"][k])
        patch = bank["patch"][bank["patch_start"][k]:bank["patch_start"][k + 1]]
        if r == 2:                                                        # behind the camera
            assert (w, h) == (0, 0) and patch.size == 0
            continue
        assert w > 0 and h > 0 and 0 <= x0 and x0 + w <= HW[1] and 0 <= y0 and y0 + h <= HW[0]
        assert np.array_equal(patch.reshape(3, h, w), item["image"].numpy()[:, y0:y0 + h, x0:x0 + w])
        # the rectangle holds the pixel of every point of the object (the hull of the projected corners), and the centre's
        u, v, a2 = P.project_px(own, tiny_crt())
        assert (a2 > 0).all() and (u >= x0).all() and (u <= x0 + w).all() and (v >= y0).all() and (v <= y0 + h).all()
        cu, cv, _ = P.project_px(row[None, :3], tiny_crt())
        assert bank["centre_px"][k].tolist() == [int(np.rint(cu[0])), int(np.rint(cv[0]))]
    # a rectangle that leaves the image is clipped; one that misses it has no patch
    wide = label_row(2.0, 0.0, -0.5, 0.0, size=(1.0, 6.0, 1.5))          # 1.5 m in front, 6 m across: u = 64 -+ 120
    x0, y0, w, h = B.patch_rect(wide, tiny_crt(), HW)
    assert (x0, w) == (0, HW[1]) and h > 0
    assert B.patch_rect(label_row(6.0, 30.0, -1.0, 0.0), tiny_crt(), HW) == (0, 0, 0, 0)
    assert B.build(ds, dict(RANGE), min_points=5, frames=[1])["source"].tolist() == [[1, 0], [1, 2]]
    assert B.build(ds, dict(RANGE), min_points=31)["source"][:, 0].tolist() == [1, 2]


def test_bank_save_load_round_trip_is_byte_equal(tmp_path):
    B = pkg("objbank")
    bank = B.build(_three_frames(), dict(RANGE))
    path = os.path.join(str(tmp_path), "bank.npz")
    B.save(path, bank)
    assert os.path.exists(path)
    back = B.load(path)
    assert sorted(back) == sorted(k for k, _ in B.ARRAYS)
    for k, dt in B.ARRAYS:
        assert back[k].dtype == dt and back[k].shape == bank[k].shape and back[k].tobytes() == bank[k].tobytes(), k
    with np.load(path, allow_pickle=False) as z:                          # plain arrays: readable with pickling refused
        assert sorted(z.files) == sorted(back)


# ------------------------------------------------------------------------------------------------ sampler
def _labels(n, seed=0):
    rng = np.random.RandomState(50 + seed)
    out = np.zeros((RANGE["max_num_bbox"], 9), dtype=np.float32)
    for i in range(n):
        out[i] = label_row(rng.uniform(5, 65), rng.uniform(-35, 35), -1.0, rng.uniform(0, 3.14))
    return out


def _draw(bank, cfg=CFG, seed=3, rank=0, call=0, b=0, boxes=None, num=0, n_points=1000, crt=None, config=RANGE):
    boxes = _labels(num) if boxes is None else boxes
    return pkg("paste").draw(cfg, seed, rank, call, b, bank, boxes, num, n_points, tiny_crt() if crt is None else crt, config)


def _same_plan(p, q):
    return (p["rows"] == q["rows"] and p["patch_rows"] == q["patch_rows"]
            and all(np.array_equal(p[k], q[k]) for k in ("labels", "records", "append", "patches")))


def test_draw_is_pure_and_call_rank_and_frame_each_change_it():
    bank = random_bank(200, HW, 1)
    cfg = dict(CFG, paste_image=False)
    base = _draw(bank, cfg)
    assert len(base["rows"]) >= 4 and _same_plan(base, _draw(bank, dict(cfg)))
    for other in (_draw(bank, cfg, call=1), _draw(bank, cfg, rank=1), _draw(bank, cfg, b=1), _draw(bank, cfg, seed=4)):
        assert other["rows"] != base["rows"]
    # candidate j is bank row floor(u(33 + j) M) on the hash of augment.draw: the accepted rows are a subsequence of the candidates
    seed, rank, call, b, M = 3, 0, 0, 0, 200
    hbase = (seed * 0x9E3779B1 + call + rank * 0x85EBCA77C2B2AE63) & M64
    cand = [int(math.floor((mix64(hbase ^ mix64((b << 8) | (33 + j))) >> 11) * (1.0 / (1 << 53)) * M)) for j in range(15)]
    it = iter(cand)
    assert all(r in it for r in base["rows"])
    # streams of its own: 33 .. 48, clear of augment's 0 .. 4 and augment_image's 16 .. 25
    P = pkg("paste")
    assert int(P._STREAMS.min()) == 33 and int(P._STREAMS.max()) == 48 and len(P._STREAMS) == P.MAX_RECORDS == 16


def test_accepted_boxes_overlap_neither_each_other_nor_the_labels():
    E, P = pkg("evalgeom"), pkg("paste")
    bank = random_bank(300, HW, 2, x=(5.0, 40.0), y=(-15.0, 15.0))          # crowded: most candidates collide
    total = 0
    for call in range(12):
        for margin in (0.0, 0.75):
            boxes = _labels(5, call)
            plan = _draw(bank, dict(CFG, margin=margin, paste_image=False), call=call, boxes=boxes, num=5)
            rows = plan["rows"]
            total += len(rows)
            fp = [P.footprint(bank["boxes"][r]) for r in rows]
            grown = [P.footprint(bank["boxes"][r], margin) for r in rows]
            lab = [P.footprint(boxes[i]) for i in range(5)]
            for i in range(len(rows)):
                assert not any(E.rects_overlap(grown[i].tolist(), l.tolist()) for l in lab)
                for j in range(i):                                        # the later one was tested, grown, against the earlier
                    assert not E.rects_overlap(grown[i].tolist(), fp[j].tolist())
            assert len(set(rows)) == len(rows)                            # a bank row drawn twice rejects itself
            assert np.array_equal(plan["labels"], bank["boxes"][rows]) and len(plan["records"]) == len(rows)
            for i, r in enumerate(rows):
                assert np.array_equal(plan["records"][i], P.record(bank["boxes"][r], margin))
                assert plan["append"][i].tolist() == [bank["point_start"][r], bank["point_start"][r + 1] - bank["point_start"][r]]
    assert total >= 30
    # a candidate outside the labelled range (valid_bbox) is never accepted
    far = random_bank(50, HW, 3, x=(71.0, 90.0))
    assert _draw(far, dict(CFG, paste_image=False))["rows"] == []


def test_every_cap_holds():
    bank = random_bank(400, HW, 4)
    cfg = dict(CFG, paste_image=False)
    for call in range(6):
        assert 8 <= len(_draw(bank, dict(cfg, target_objects=100), call=call)["rows"]) <= 16          # 16 records
        assert len(_draw(bank, dict(cfg, target_objects=100, max_candidates=3), call=call)["rows"]) <= 3
        p = _draw(bank, dict(cfg, target_objects=9), call=call, num=5)
        assert 1 <= len(p["rows"]) <= 4                                                               # target_objects - num
        assert _draw(bank, dict(cfg, target_objects=5), call=call, num=5)["rows"] == []
        assert _draw(bank, dict(cfg, target_objects=3), call=call, num=5)["rows"] == []
        p = _draw(bank, dict(cfg, target_objects=100), call=call, num=17)
        assert len(p["rows"]) == 3                                                                    # max_num_bbox = 20
        assert _draw(bank, dict(cfg, target_objects=100), call=call, num=20)["rows"] == []
        for cap in (1000, 1004, 1050, 1200):                                                          # max_num_pc, n_points = 1000
            p = _draw(bank, dict(cfg, target_objects=100), call=call, config=dict(RANGE, max_num_pc=cap))
            assert 1000 + int(p["append"][:, 1].sum()) <= cap
            assert (cap >= 1050) == (len(p["rows"]) > 0)
    boxes, num = pkg("paste").append_labels(_labels(17), 17, _draw(bank, dict(cfg, target_objects=100), num=17))
    assert num == 20 and np.array_equal(boxes[:17], _labels(17)[:17]) and (boxes[17:, 7] == 6).all()


def test_vectorised_overlap_equals_the_scalar_test_on_2000_pairs():
    E, P = pkg("evalgeom"), pkg("paste")
    rng = np.random.RandomState(7)
    A, Bs = [], []
    for i in range(2000):
        kind = i % 5
        a = E.bev_rect((rng.uniform(-5, 5), rng.uniform(-5, 5)), (rng.uniform(1, 5), rng.uniform(1, 3)), rng.uniform(-4, 4))
        if kind == 0:                                                     # identical
            b = list(a)
        elif kind == 1:                                                   # touching along an edge, dyadic: the projections tie exactly
            w = float(rng.randint(1, 9)) / 4
            a = E.bev_rect((1.0, 2.0), (2.0, w), 0.0)
            b = E.bev_rect((3.0, 2.0 + float(rng.randint(-3, 4)) / 8), (2.0, 1.5), 0.0)
        elif kind == 2:                                                   # touching at a corner / a hair apart or inside, rotated
            yaw = rng.uniform(-4, 4)
            a = E.bev_rect((0.0, 0.0), (2.0, 1.0), yaw)
            d = 2.0 + rng.choice([-1e-12, 0.0, 1e-12])
            b = E.bev_rect((d * math.cos(yaw), d * math.sin(yaw)), (2.0, 1.0), yaw)
        else:
            b = E.bev_rect((rng.uniform(-5, 5), rng.uniform(-5, 5)), (rng.uniform(1, 5), rng.uniform(1, 3)), rng.uniform(-4, 4))
        A.append(a); Bs.append(b)
    want = np.array([E.rects_overlap(a, b) for a, b in zip(A, Bs)])
    assert 400 < want.sum() < 1700
    # one rectangle against all 2000 at once, for a few of them ...
    Barr = np.array(Bs, dtype=np.float64)
    for i in (0, 1, 2, 3, 4, 1001, 1997):
        got = P.overlap_many(np.array(A[i]), Barr)
        assert np.array_equal(got, np.array([E.rects_overlap(A[i], b) for b in Bs])), i
    # ... and every pair (one against a batch of one: the same array code)
    got = np.array([bool(P.overlap_many(np.array(a), np.array([b]))[0]) for a, b in zip(A, Bs)])
    assert np.array_equal(got, want)
    assert P.overlap_many(np.array(A[0]), np.zeros((0, 4, 2))).shape == (0,)


def test_patch_records_are_ordered_far_to_near():
    bank = random_bank(300, HW, 5)
    bank["centre_px"][:] = 0                                              # (_crt_for_centres: every shift is then 0)
    seen = 0
    for call in range(8):
        plan = _draw(bank, dict(CFG, target_objects=100), call=call, crt=_crt_for_centres())
        rows, order = plan["rows"], plan["patch_rows"]
        assert sorted(order) == sorted(rows) and len(plan["patches"]) == len(rows)
        dist = [math.hypot(float(bank["boxes"][r][0]), float(bank["boxes"][r][1])) for r in order]
        assert all(dist[i] >= dist[i + 1] for i in range(len(dist) - 1))
        want = sorted(range(len(rows)), key=lambda k: (-math.hypot(float(bank["boxes"][rows[k]][0]), float(bank["boxes"][rows[k]][1])), k))
        assert order == [rows[k] for k in want]
        for q, r in zip(plan["patches"], order):
            assert q[6:9].tolist() == [bank["rect"][r][2], bank["rect"][r][3], bank["patch_start"][r]]
        seen += len(rows)
    assert seen >= 20
    # ties keep the acceptance order: two objects at the same distance
    tie = random_bank(2, HW, 6)
    tie["boxes"][0, :2], tie["boxes"][1, :2] = (10.0, 5.0), (10.0, -5.0)
    tie["centre_px"][:] = 0
    for call in range(20):
        plan = _draw(tie, dict(CFG), call=call, crt=_crt_for_centres())
        if len(plan["rows"]) == 2:
            assert plan["patch_rows"] == plan["rows"]
            seen = -1
    assert seen == -1


def _crt_for_centres():
    """A calibration that projects EVERY point to pixel (0, 0) + (a2 = 1): with centre_px = 0 every shift is 0, so the destination
    is the bank's own rectangle whatever the box (the order test wants many accepted patches, not geometry)."""
    crt = np.zeros((4, 3), dtype=np.float32)
    crt[3, 2] = 1.0
    return crt


def test_destination_rectangle_is_clipped_at_all_four_borders_with_the_right_source_offsets():
    P = pkg("paste")
    H, W = HW
    row = label_row(10.0, 0.0, -1.0, 0.0)
    crt = tiny_crt().astype(np.float64)
    u, v, _ = P.project_px(row[None, :3], crt)
    here = (int(np.rint(u[0])), int(np.rint(v[0])))
    assert P.centre_pixel(row, crt) == here
    rect = (50, 40, 30, 20)                                               # the patch in its source image

    def dest(shift):
        # the bank's centre_px is where the source frame saw the centre: `shift` away from where this frame sees it
        return P.destination(rect, (here[0] - shift[0], here[1] - shift[1]), row, crt, HW)

    assert dest((0, 0)) == (50, 40, 30, 20, 0, 0)
    assert dest((3, -2)) == (53, 38, 30, 20, 0, 0)
    assert dest((-60, 0)) == (0, 40, 20, 20, 10, 0)                       # left: the first 10 columns are cut, the source starts at 10
    assert dest((60, 0)) == (110, 40, 18, 20, 0, 0)                       # right: 110 + 30 > 128
    assert dest((0, -50)) == (50, 0, 30, 10, 0, 10)                       # top
    assert dest((0, 50)) == (50, 90, 30, 6, 0, 0)                         # bottom: 90 + 20 > 96
    assert dest((-60, -50)) == (0, 0, 20, 10, 10, 10)
    assert dest((-80, 0)) is None and dest((78, 0)) is None and dest((0, -60)) is None and dest((0, 56)) is None      # nothing left
    assert dest((-79, 0)) == (0, 40, 1, 20, 29, 0) and dest((77, 0)) == (127, 40, 1, 20, 0, 0)
    assert P.destination((0, 0, 0, 0), here, row, crt, HW) is None        # no patch
    assert P.destination(rect, here, label_row(-3.0, 0.0, -1.0, 0.0), crt, HW) is None      # the centre is behind this frame's camera
    # a calibration whose principal point moved by (+5, -7) pixels moves the patch by exactly that
    moved = crt.copy()
    moved[:, 0] += 5.0 * crt[:, 2]
    moved[:, 1] -= 7.0 * crt[:, 2]
    assert P.destination(rect, here, row, moved, HW) == (55, 33, 30, 20, 0, 0)
    # the sampler: with paste_image an object without a patch, or whose destination is empty, is not accepted; without it, it is
    bank = random_bank(40, HW, 8)
    bank["rect"][::2, 2:] = 0
    for call in range(5):
        plan = _draw(bank, dict(CFG), call=call, crt=_crt_for_centres())
        assert plan["rows"] and all(r % 2 == 1 for r in plan["rows"])
        gone = dict(bank, centre_px=bank["centre_px"] + 500)             # every destination lands left of / above the image
        assert _draw(gone, dict(CFG), call=call, crt=_crt_for_centres())["rows"] == []
        free = _draw(gone, dict(CFG, paste_image=False), call=call, crt=_crt_for_centres())
        assert free["rows"] and len(free["patches"]) == 0
    # the plan's records ARE destination()'s
    plan = _draw(bank, dict(CFG), crt=tiny_crt())
    for q, r in zip(plan["patches"], plan["patch_rows"]):
        assert tuple(q[:6]) == P.destination(bank["rect"][r], bank["centre_px"][r], bank["boxes"][r], tiny_crt(), HW)


def test_bad_values_raise():
    P, T = pkg("paste"), pkg("train")
    bank = random_bank(10, HW, 9)
    for bad in (dict(target_objects=-1), dict(target_objects=2.5), dict(max_candidates=0), dict(max_candidates=17), dict(max_candidates=True),
                dict(margin=-0.1), dict(margin=float("nan")), dict(margin="1")):
        with pytest.raises(ValueError):
            _draw(bank, dict(CFG, **bad))
        with pytest.raises(ValueError):
            T.parse_paste_config({"augment_paste": dict(CFG, enabled=False, **bad)})       # enabled or not
    for bad in (dict(enabled=1), dict(seed=1.5), dict(paste_image="yes"), dict(bank=3), dict(rotation=1)):
        with pytest.raises(ValueError):
            T.parse_paste_config({"augment_paste": dict(CFG, **bad)})
    with pytest.raises(ValueError):
        T.parse_paste_config({"augment_paste": {"enabled": True}})                          # an enabled block needs a bank
    with pytest.raises(ValueError):
        T.parse_paste_config({"augment_paste": [1]})
    empty = {k: v[:0] if k not in ("point_start", "patch_start", "image_hw") else v[:1] for k, v in bank.items()}
    empty["image_hw"] = bank["image_hw"]
    with pytest.raises(ValueError):
        _draw(empty)                                                                        # M = 0
    with pytest.raises(ValueError):
        P.check_bank(bank, (HW[0], HW[1] + 1))                                              # patches of another image size
    with pytest.raises(ValueError):
        P.check_bank({k: v for k, v in bank.items() if k != "rect"})
    P.check_bank(bank, HW)
    got = T.parse_paste_config({"augment_paste": dict(CFG, enabled=True)})
    assert got == {"seed": 3, "bank": "unused", "target_objects": 15, "max_candidates": 16, "margin": 0.0, "paste_image": True}
    assert T.parse_paste_config({"augment_paste": {"enabled": True, "bank": "b.npz"}}) == {"seed": 0, "bank": "b.npz", "target_objects": 15, "max_candidates": 16,
                                                                                            "margin": 0.0, "paste_image": True}


# ------------------------------------------------------------------------------------------------ statements
def _paint_one_after_another(img, records, patch):
    """The independent painter: the patches copied with numpy slices in record order, each over what is there."""
    out = img.copy()
    for x0, y0, w, h, sx, sy, pw, ph, start in (tuple(int(v) for v in q) for q in records):
        src = patch[start:start + 3 * ph * pw].reshape(3, ph, pw)
        out[:, y0:y0 + h, x0:x0 + w] = src[:, sy:sy + h, sx:sx + w]
    return out


def test_paste_image_equals_an_independent_painter():
    P = pkg("paste")
    rng = np.random.RandomState(11)
    for H, W in ((1, 1), (5, 7), (13, 66), (96, 128)):
        img = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
        recs, patch, start = [], [], 0
        for k in range(12):
            pw, ph = rng.randint(1, W + 1), rng.randint(1, H + 1)
            w, h = rng.randint(1, pw + 1), rng.randint(1, ph + 1)
            recs.append((rng.randint(0, W - w + 1), rng.randint(0, H - h + 1), w, h, rng.randint(0, pw - w + 1), rng.randint(0, ph - h + 1), pw, ph, start))
            patch.append(rng.randint(0, 256, 3 * ph * pw).astype(np.uint8))
            start += 3 * ph * pw
        bank = {"patch": np.concatenate(patch)}
        for m in (0, 1, 5, 12):
            plan = plan_of(patches=recs[:m], hw=(H, W))
            got = P.paste_image(img, plan, bank)
            assert np.array_equal(got, _paint_one_after_another(img, recs[:m], bank["patch"])), (H, W, m)
            if m == 0:
                assert np.array_equal(got, img)
        assert not np.array_equal(P.paste_image(img, plan_of(patches=recs, hw=(H, W)), bank), img) or (H, W) == (1, 1)
    with pytest.raises(ValueError):
        P.paste_image(np.zeros((3, 4), dtype=np.uint8), plan_of(), {"patch": np.zeros(0, dtype=np.uint8)})


def test_paste_points_removes_exactly_the_inside_rows_and_appends_the_banks_bytes():
    P = pkg("paste")
    rng = np.random.RandomState(12)
    bank = random_bank(30, HW, 13)
    rows = [3, 17, 8]
    boxes = bank["boxes"][rows]
    inside = np.concatenate([_box_pts(b, 25, rng) for b in boxes], 0)
    outside = rng.uniform(-60, -45, (200, 3)).astype(np.float32)          # (the bank's boxes have x >= 2)
    special = np.array([[np.nan, 1, 1], [np.inf, 0, 0], [-np.inf, 2, 2], [boxes[0][0], boxes[0][1], np.nan], [boxes[0][0], np.inf, boxes[0][2]]], dtype=np.float32)
    pts = np.concatenate([inside, outside, special], 0)[rng.permutation(280)]
    for margin in (0.0, 0.5):
        plan = plan_of(records=[P.record(b, margin) for b in boxes],
                       append=[(bank["point_start"][r], bank["point_start"][r + 1] - bank["point_start"][r]) for r in rows], n_points=len(pts))
        out = P.paste_points(pts, plan, bank)
        a = sum(int(bank["point_start"][r + 1] - bank["point_start"][r]) for r in rows)
        assert out.shape == (280 + a, 3) and out.dtype == np.float32
        # an independent float64 statement of the test (the points are well inside or far outside: no rounding decides)
        gone = np.zeros(280, dtype=bool)
        with np.errstate(invalid="ignore"):
            for b in boxes.astype(np.float64):
                dx, dy = pts[:, 0].astype(np.float64) - b[0], pts[:, 1].astype(np.float64) - b[1]
                lx, ly = dx * math.cos(b[6]) + dy * math.sin(b[6]), dy * math.cos(b[6]) - dx * math.sin(b[6])
                gone |= (np.abs(lx) <= b[3] / 2 + margin) & (np.abs(ly) <= b[4] / 2 + margin) & (np.abs(pts[:, 2] - b[2]) <= b[5] / 2 + margin)
        assert gone.sum() == 75
        assert np.isposinf(out[:280][gone]).all()
        assert np.array_equal(out[:280][~gone].view(np.uint32), pts[~gone].view(np.uint32))          # NaN / inf rows included, bit for bit
        tail = np.concatenate([bank["points"][bank["point_start"][r]:bank["point_start"][r + 1]] for r in rows], 0)
        assert out[280:].tobytes() == tail.tobytes()
    assert P.paste_points(pts, plan_of(n_points=280), bank).tobytes() == pts.tobytes()
    # yaw 0, dyadic numbers: points exactly on each face are inside (closed test), 2^-10 m beyond (exact in fp32 too) is not
    rec = P.record(label_row(8.0, -2.0, -1.0, 0.0), 0.25)
    hl, hw, hh = CAR[0] / 2 + 0.25, CAR[1] / 2 + 0.25, CAR[2] / 2 + 0.25
    faces = np.array([[8 + hl, -2, -1], [8 - hl, -2, -1], [8, -2 + hw, -1], [8, -2 - hw, -1], [8, -2, -1 + hh], [8, -2, -1 - hh]], dtype=np.float32)
    assert P.inside_mask(faces, rec).all()
    beyond = faces.copy()
    for i in range(6):
        beyond[i, i // 2] += np.float32(2.0 ** -10 if i % 2 == 0 else -2.0 ** -10)
    assert not P.inside_mask(beyond, rec).any()


def _box_pts(row, n, rng):
    from _paste_util import box_points
    return box_points(row, n, rng)


# ------------------------------------------------------------------------------------------------ trainer config
def test_block_absent_disabled_and_target_zero_draw_empty_plans():
    T = pkg("train")
    bank = random_bank(50, HW, 14)
    boxes = np.stack([_labels(4, 1), _labels(6, 2)], 0)
    nums = torch.tensor([4, 6])
    crts = [tiny_crt(), tiny_crt()]
    for config in ({}, {"augment_paste": None}, {"augment_paste": dict(CFG, enabled=False)}, {"augment_paste": dict(CFG, enabled=True, target_objects=0)},
                   {"augment_paste": dict(CFG, enabled=True, target_objects=4)}):
        cfg = T.parse_paste_config(config)
        assert (cfg is None) == (not (config.get("augment_paste") or {}).get("enabled", False))
        plans, new_boxes, new_nums = T.draw_paste_plans(cfg, bank if cfg is not None else None, 0, 5, boxes, nums, [900, 1100], crts, dict(RANGE))
        assert len(plans) == 2 and new_nums == [4, 6] and np.array_equal(new_boxes, boxes)
        for p in plans:
            assert p["rows"] == [] and p["records"].shape == (0, 8) and p["append"].shape == (0, 2) and p["patches"].shape == (0, 9)
    cfg = T.parse_paste_config({"augment_paste": dict(CFG, enabled=True, paste_image=False)})
    plans, new_boxes, new_nums = T.draw_paste_plans(cfg, bank, 0, 5, boxes, nums, [900, 1100], crts, dict(RANGE))
    assert all(p["rows"] for p in plans) and new_nums == [4 + len(plans[0]["rows"]), 6 + len(plans[1]["rows"])]
    for b in range(2):
        n0 = int(nums[b])
        assert np.array_equal(new_boxes[b, :n0], boxes[b, :n0]) and np.array_equal(new_boxes[b, n0:new_nums[b]], bank["boxes"][plans[b]["rows"]])
        assert not new_boxes[b, new_nums[b]:].any()
        assert _same_plan(plans[b], pkg("paste").draw(cfg, 3, 0, 5, b, bank, boxes[b], n0, [900, 1100][b], crts[b], dict(RANGE)))

"""Frames and helpers shared by the camera-mask tests (test infrastructure; no test lives here)."""
import numpy as np

from _paste_util import RANGE, Frames, label_row, make_frame, tiny_crt
from _util import pkg

LIM_TINY = (0.0, 16.0, -4.0, 4.0, -2.4, 0.8)
LIM_KITTI = (0.0, 70.4, -40.0, 40.0, -3.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def lim_of(lim6, delta=0.01):
    return np.array([lim6[0], lim6[1] - delta, lim6[2], lim6[3] - delta, lim6[4], lim6[5] - delta], dtype=np.float64).astype(np.float32)


def pasted_world(which):
    """A bank from two frames, its objects pasted into a third frame with 20 000 background points: (bank, plan, pasted fp32 points,
    n scene rows, crt, lim6, hw)."""
    P, B = pkg("paste"), pkg("objbank")
    if which == "tiny":
        crt, hw, lim6 = tiny_crt(), (96, 128), LIM_TINY
        spots = [[(5.0, -1.5, 0.1), (9.0, 1.5, 0.3)], [(7.0, 0.0, 0.2), (12.0, -1.0, 0.4)]]
    else:
        crt, hw, lim6 = pkg("calib").kitti_like_crt(), (375, 1242), LIM_KITTI
        spots = [[(9.0, 2.0, 0.4), (15.0, -3.5, 1.2), (24.0, 5.0, 2.0)], [(12.0, -1.0, 0.1), (19.0, 4.0, 2.6), (30.0, -6.0, 1.6)]]
    config = dict(RANGE, lidar_x_max=lim6[1], lidar_y_min=lim6[2], lidar_y_max=lim6[3], image_height=hw[0], image_width=hw[1])
    items = [make_frame([label_row(x, y, -1.0, yaw) for x, y, yaw in s], [40] * len(s), 200, lim6, hw, 80 + f) for f, s in enumerate(spots)]
    bank = B.build(Frames(items, crt), config)
    assert (bank["rect"][:, 2] > 0).all()
    target = make_frame([], [], 20000, lim6, hw, 89)
    pts = target["lidar_points"].numpy()
    plan = P.draw({"seed": 1, "target_objects": 15, "max_candidates": 16, "margin": 0.25, "paste_image": True}, 1, 0, 0, 0, bank,
                  target["bboxes"].numpy(), 0, len(pts), crt, config)
    assert len(plan["rows"]) >= 2
    return bank, plan, P.paste_points(pts, plan, bank), len(pts), crt, lim6, hw

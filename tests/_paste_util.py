"""Hand-made raw frames, banks and plans shared by the object-pasting tests (test infrastructure; no test lives here)."""
import numpy as np
import torch

from _util import pkg

CAR = (4.0, 1.75, 1.5)                   # l, w, h: dyadic, so a yaw-0 box has exactly representable faces


def tiny_crt():
    calib = pkg("calib")
    return calib.crt_from(np.array([[60.0, 0.0, 64.0], [0.0, 60.0, 48.0], [0.0, 0.0, 1.0]]), calib.R_LIDAR_TO_CAM)


def ramp_image(h, w, seed):
    """uint8 [3,h,w] whose bytes tell pixels apart: channel c = (a_c x + b_c y + seed-dependent offset) mod 251."""
    xx, yy = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    return np.stack([((3 + 2 * c) * xx + (7 + 4 * c) * yy + 17 * seed + 5 * c) % 251 for c in range(3)], 0).astype(np.uint8)


def label_row(x, y, z, yaw, size=CAR):
    return np.array([x, y, z, size[0], size[1], size[2], yaw, 6.0, 1.0], dtype=np.float32)


def box_points(row, n, rng, fill=0.9):
    """n fp32 points strictly inside the box of a label row (local coordinates within `fill` of the half sizes)."""
    loc = (rng.rand(n, 3) - 0.5) * np.asarray(row[3:6], dtype=np.float64) * fill
    c, s = np.cos(float(row[6])), np.sin(float(row[6]))
    out = np.empty((n, 3))
    out[:, 0] = row[0] + c * loc[:, 0] - s * loc[:, 1]
    out[:, 1] = row[1] + s * loc[:, 0] + c * loc[:, 1]
    out[:, 2] = row[2] + loc[:, 2]
    return out.astype(np.float32)


def make_frame(rows, counts, n_background, lim6, hw, seed, max_num_bbox=20, crt=None):
    """One raw item: the labelled objects `rows` with `counts` points each, n_background points of the range lim6 = (x0, x1, y0, y1,
    z0, z1) that keep half a metre from every box, in a shuffled order; a ramp image [3, hw[0], hw[1]]."""
    P = pkg("paste")
    rng = np.random.RandomState(1000 + seed)
    parts = [box_points(r, k, rng) for r, k in zip(rows, counts)]
    lo, hi = np.array(lim6[0::2]), np.array(lim6[1::2])
    bg = (lo + rng.rand(4 * n_background + 64, 3) * (hi - lo)).astype(np.float32)
    clear = np.ones(len(bg), dtype=bool)
    for r in rows:
        clear &= ~P.inside_mask(bg, P.record(r, 0.5))
    bg = bg[clear][:n_background]
    assert len(bg) == n_background
    pts = np.concatenate(parts + [bg], 0)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    boxes = torch.zeros(max_num_bbox, 9)
    for i, r in enumerate(rows):
        boxes[i] = torch.from_numpy(np.asarray(r, dtype=np.float32))
    return {"lidar_points": torch.from_numpy(pts), "image": torch.from_numpy(ramp_image(hw[0], hw[1], seed)), "bboxes": boxes,
            "num_bboxes": len(rows), "crt": crt}


class Frames(object):
    """A raw-mode dataset over a list of items (what objbank.build and FrameLoader ask of one)."""
    raw = True

    def __init__(self, items, crt):
        self.items, self._crt = list(items), crt

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def random_bank(M, hw, seed, x=(2.0, 68.0), y=(-38.0, 38.0)):
    """A bank of M objects made directly (no frames): random boxes of the range, 5..40 random points each (NOT inside the boxes: the
    sampler never looks), a random rectangle of the [hw] image with random bytes and its middle as centre_px."""
    rng = np.random.RandomState(seed)
    H, W = hw
    boxes = np.zeros((M, 9), dtype=np.float32)
    boxes[:, 0], boxes[:, 1], boxes[:, 2] = rng.uniform(x[0], x[1], M), rng.uniform(y[0], y[1], M), rng.uniform(-1.5, -0.5, M)
    boxes[:, 3], boxes[:, 4], boxes[:, 5] = rng.uniform(3.5, 4.8, M), rng.uniform(1.6, 2.1, M), rng.uniform(1.4, 1.8, M)
    boxes[:, 6], boxes[:, 7], boxes[:, 8] = rng.uniform(0.0, 3.14, M), 6.0, 1.0
    counts = rng.randint(5, 41, M)
    pstart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rect = np.zeros((M, 4), dtype=np.int32)
    rect[:, 2], rect[:, 3] = rng.randint(1, max(W // 3, 1) + 1, M), rng.randint(1, max(H // 3, 1) + 1, M)
    rect[:, 0], rect[:, 1] = rng.randint(0, W - rect[:, 2] + 1), rng.randint(0, H - rect[:, 3] + 1)
    qstart = np.concatenate([[0], np.cumsum(3 * rect[:, 2].astype(np.int64) * rect[:, 3])]).astype(np.int64)
    return {"points": rng.uniform(-50, 50, (int(pstart[-1]), 3)).astype(np.float32), "point_start": pstart, "boxes": boxes, "rect": rect,
            "patch": rng.randint(0, 256, int(qstart[-1])).astype(np.uint8), "patch_start": qstart,
            "centre_px": np.stack([rect[:, 0] + rect[:, 2] // 2, rect[:, 1] + rect[:, 3] // 2], 1).astype(np.int32),
            "image_hw": np.array([H, W], dtype=np.int32), "source": np.stack([np.arange(M), np.zeros(M)], 1).astype(np.int32)}


def plan_of(records=None, append=None, patches=None, n_points=0, hw=(1, 1), rows=None):
    """A plan put together by hand (the kernels' tests choose their own records)."""
    P = pkg("paste")
    plan = P.empty_plan(n_points, hw)
    if records is not None:
        plan["records"] = np.asarray(records, dtype=np.float32).reshape(-1, 8)
        plan["append"] = np.asarray(append, dtype=np.int64).reshape(-1, 2)
        plan["rows"] = list(range(len(plan["records"]))) if rows is None else list(rows)
    if patches is not None:
        plan["patches"] = np.asarray(patches, dtype=np.int64).reshape(-1, 9)
    return plan


RANGE = dict(lidar_x_min=0.0, lidar_x_max=70.4, lidar_y_min=-40.0, lidar_y_max=40.0, lidar_z_min=-3.0, lidar_z_max=1.0, max_num_bbox=20,
             max_num_pc=100000, image_height=96, image_width=128)

"""The object bank of train-time object pasting (paste.py): every labelled object of a raw-mode dataset as
its LiDAR points, its label row and its camera patch, built once on the host (numpy) and uploaded once by the trainer.

    points       fp32  [P,3]    the objects' points back to back, sensor coordinates, frame order, unchanged
    point_start  int64 [M+1]    object k owns points[point_start[k]:point_start[k+1]]
    boxes        fp32  [M,9]    the label rows as the dataset gave them (x, y, z, l, w, h, yaw, class, 1)
    rect         int32 [M,4]    (x0, y0, w, h) of the patch in its source image; w = h = 0: no patch
    patch        uint8 [Q]      the patches back to back, each [3,h,w] contiguous
    patch_start  int64 [M+1]
    centre_px    int32 [M,2]    the box centre's projected pixel (u, v), rounded: the sampler follows a frame's own calibration with it
    image_hw     int32 [2]      (H, W) of the images the patches were cut from
    source       int32 [M,2]    (frame, label row)

python -m <package>.objbank --out PATH builds the bank of train.make_dataset(config).
"""
import numpy as np

from . import paste

ARRAYS = (("points", np.float32), ("point_start", np.int64), ("boxes", np.float32), ("rect", np.int32), ("patch", np.uint8),
          ("patch_start", np.int64), ("centre_px", np.int32), ("image_hw", np.int32), ("source", np.int32))


def patch_rect(row, crt, image_hw):
    """(x0, y0, w, h) of a label row's patch in an [H, W] image under the [4,3] matrix crt: the eight corners -- evalgeom.bev_rect's
    footprint at z -+ h/2, z the mid-height centre (data_import_kitti.read_labels) -- projected in float64, the rectangle
    [floor(min u), ceil(max u)) x [floor(min v), ceil(max v)) clipped to the image.  (0, 0, 0, 0) when a corner has a2 <= 0 or
    nothing is left."""
    fp = paste.footprint(row)
    z, hh = float(row[2]), float(row[5]) / 2
    corners = np.array([(x, y, zz) for zz in (z - hh, z + hh) for x, y in fp], dtype=np.float64)
    u, v, a2 = paste.project_px(corners, crt)
    if not (a2 > 0).all() or not (np.isfinite(u).all() and np.isfinite(v).all()):
        return 0, 0, 0, 0
    H, W = int(image_hw[0]), int(image_hw[1])
    x0, x1 = max(float(np.floor(u.min())), 0.0), min(float(np.ceil(u.max())), float(W))
    y0, y1 = max(float(np.floor(v.min())), 0.0), min(float(np.ceil(v.max())), float(H))
    if x1 <= x0 or y1 <= y0:
        return 0, 0, 0, 0
    return int(x0), int(y0), int(x1 - x0), int(y1 - y0)


def _frame_crt(dataset, item):
    crt = item.get("crt")
    if crt is None:
        crt = getattr(dataset, "_crt", None)
    if crt is None:
        from . import calib
        crt = calib.carla_crt()
    return np.asarray(crt, dtype=np.float64).reshape(4, 3)


def build(dataset, config, min_points=5, frames=None):
    """The bank of every valid label row of every frame (frames: indices, None = all) of a raw-mode dataset -- items with
    lidar_points, image, bboxes, num_bboxes and crt (None = the dataset's one calibration).  An object's points are the frame's
    points that pass paste's inside test with margin 0, in frame order; objects with fewer than min_points are left out.  config:
    the dataset config (its image size stands in when no frame is visited)."""
    pts_out, boxes, rects, patches, centres, source = [], [], [], [], [], []
    pstart, qstart = [0], [0]
    image_hw = None
    for f in (range(len(dataset)) if frames is None else frames):
        item = dataset[int(f)]
        pts = np.ascontiguousarray(np.asarray(item["lidar_points"], dtype=np.float32).reshape(-1, 3))
        img = np.asarray(item["image"])
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] != 3:
            raise ValueError("objbank: frame %d: image must be uint8 [3,H,W] (got %s %s)" % (f, img.dtype, img.shape))
        if image_hw is None:
            image_hw = (int(img.shape[1]), int(img.shape[2]))
        elif image_hw != (int(img.shape[1]), int(img.shape[2])):
            raise ValueError("objbank: frame %d: image of %s among %s ones" % (f, img.shape[1:], image_hw))
        crt = _frame_crt(dataset, item)
        rows = np.asarray(item["bboxes"], dtype=np.float32)
        for k in range(int(item["num_bboxes"])):
            row = rows[k]
            own = pts[paste.inside_mask(pts, paste.record(row, 0.0))]
            if own.shape[0] < int(min_points):
                continue
            x0, y0, w, h = patch_rect(row, crt, image_hw)
            centre = paste.centre_pixel(row, crt) if w else None
            pts_out.append(own)
            pstart.append(pstart[-1] + own.shape[0])
            boxes.append(row.copy())
            rects.append((x0, y0, w, h))
            patches.append(np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w]).reshape(-1))
            qstart.append(qstart[-1] + 3 * h * w)
            centres.append(centre if centre is not None else (0, 0))
            source.append((int(f), k))
    if image_hw is None:                                  # no frame visited: the configured size
        image_hw = (int(config.get("image_height", 0)), int(config.get("image_width", 0)))
    M = len(boxes)
    return {"points": np.concatenate(pts_out, 0) if M else np.zeros((0, 3), dtype=np.float32),
            "point_start": np.asarray(pstart, dtype=np.int64),
            "boxes": np.stack(boxes, 0).astype(np.float32) if M else np.zeros((0, 9), dtype=np.float32),
            "rect": np.asarray(rects, dtype=np.int32).reshape(M, 4),
            "patch": np.concatenate(patches, 0).astype(np.uint8) if M else np.zeros((0,), dtype=np.uint8),
            "patch_start": np.asarray(qstart, dtype=np.int64),
            "centre_px": np.asarray(centres, dtype=np.int32).reshape(M, 2),
            "image_hw": np.asarray(image_hw, dtype=np.int32),
            "source": np.asarray(source, dtype=np.int32).reshape(M, 2)}


def save(path, bank):
    """One .npz of plain arrays (no pickled objects), written to exactly `path`."""
    with open(path, "wb") as f:
        np.savez(f, **{k: np.ascontiguousarray(np.asarray(bank[k], dtype=dt)) for k, dt in ARRAYS})


def load(path):
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k, _ in ARRAYS if k not in z.files]
        if missing:
            raise ValueError("object bank %s: missing arrays %s" % (path, missing))
        return {k: np.ascontiguousarray(z[k].astype(dt, copy=False)) for k, dt in ARRAYS}


def main(argv=None):
    import argparse
    import os
    import yaml
    from .train import make_dataset
    ap = argparse.ArgumentParser(description="build the object bank of augment_paste from the training set")
    ap.add_argument("--out", required=True)
    ap.add_argument("--config", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "config", "config_carla.yaml"))
    ap.add_argument("--min-points", type=int, default=5)
    a = ap.parse_args(argv)
    with open(a.config) as f:
        config = yaml.safe_load(f)
    bank = build(make_dataset(config), config, min_points=a.min_points)
    save(a.out, bank)
    M = int(bank["boxes"].shape[0])
    print("object bank: %d objects, %d points, %d with a patch, %d patch bytes -> %s"
          % (M, bank["points"].shape[0], int((bank["rect"][:, 2] > 0).sum()), bank["patch"].size, a.out))


if __name__ == "__main__":
    main()

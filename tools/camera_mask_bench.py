#!/usr/bin/env python3
"""Cost of the camera visibility mask (csrc/camera_mask.hip, visibility.py).

  python tools/camera_mask_bench.py [--iters 300] [--steps 40] [--warmup 10] [--rounds 3] [--out FILE]

1. The launch alone at the cfg2 shapes, HIP events around every call after a warm-up, the median: dcf_camera_mask_points_batch on
   2 x 100 000 rows with the field-of-view rule on and 16 occluders per frame, beside dcf_augment_points_batch on the same rows in
   the same process -- the yardstick of section 21, which moves the same bytes.
2. The whole cfg2 train step (frames resident in HBM, batch 2, bf16, 96 800 points per frame) through Train.one_step_raw with the
   block off, with fov_crop on, with `augment_paste` alone and with both switches on over it: trainers in one process on one GPU, alternating,
   --rounds rounds of --steps steps each, a host clock around steps that end in a device synchronise.
Prints one JSON line (and writes it to --out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
ROWS = 100000


def launch_alone(bank, iters):
    import numpy as np
    import torch
    PB = importlib.import_module("paste_bench")
    A, V, ops, D, det, calib = (importlib.import_module(PKG + "." + m) for m in ("augment", "visibility", "ops", "data_import_carla", "detfill", "calib"))
    bench = importlib.import_module("bench")
    B = 2
    cfg = bench.kitti_config(B)
    geo = D.FrameGeometry(cfg, calib.kitti_like_crt())
    lim6 = (0.0, 70.4, -40.0, 40.0, -2.4, 0.8)
    pts = [torch.from_numpy(det.synthetic_points(ROWS, lim6, 77 + b)).cuda() for b in range(B)]
    plans = PB.full_plans(bank, B)
    for p in plans:                                    # (hand-made plans: one patch record per object with a rectangle, in row order)
        p["patch_rows"] = [r for r in p["rows"] if bank["rect"][r][2] > 0]
    occ = [V.occluders(p, bank, geo.crt) for p in plans]
    dst = [torch.empty_like(p) for p in pts]
    out = {"mask": PB.timed(lambda: geo.mask_points(pts, None, True, occ, out=dst), iters)}
    torch.cuda.synchronize()
    out["mask"].update(rows=[B, ROWS], occluders=[len(q) for q in occ], masked=[int(torch.isinf(d[:, 0]).sum()) for d in dst])
    out["mask_occluders_only"] = PB.timed(lambda: geo.mask_points(pts, None, False, occ, out=dst), iters)
    out["mask_fov_only"] = PB.timed(lambda: geo.mask_points(pts, None, True, None, out=dst), iters)
    bev = [A.draw({"rotation_deg": 20.0, "scale": (0.95, 1.05), "flip_prob": 0.5, "point_drop": (0.05, 0.2)}, 1, 0, 0, b) for b in range(B)]
    out["yardstick_augment_points"] = PB.timed(lambda: ops.augment_points_batch(pts, bev, dst), iters)
    out["ratio_to_yardstick"] = out["mask"]["median_us"] / out["yardstick_augment_points"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("camera_mask_bench.py measures on the GPU; none is visible")
    PB = importlib.import_module("paste_bench")
    bench = importlib.import_module("bench")
    T, FL, det, objbank = (importlib.import_module(PKG + "." + m) for m in ("train", "frame_loader", "detfill", "objbank"))
    bank = PB.make_bank(64, 5)
    B = 2
    cfg = bench.kitti_config(B)
    out = {"launch": launch_alone(bank, args.iters)}

    pool = bench.FramePool(cfg, 4, PB.N_SCENE, 1234)
    trainers = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bank.npz")
        objbank.save(path, bank)
        for side in ("off", "fov", "paste", "both_paste"):
            c = dict(cfg)
            if side == "fov":
                c["camera_mask"] = {"fov_crop": True}
            if side in ("paste", "both_paste"):
                c["augment_paste"] = dict(PB.PASTE, bank=path)
            if side == "both_paste":
                c["camera_mask"] = {"fov_crop": True, "paste_occlusion": True}
            trainers[side] = T.Train(c)
            det.fill_state_dict(trainers[side].model)

    def batch(step):
        ids = pool.batch(step, B)
        b = FL.Batch(bboxes=torch.stack([pool.boxes[i] for i in ids], 0), num_bboxes=torch.tensor([pool.nb[i] for i in ids]), crt=None)
        b["points"], b["image"] = [pool.pts[i] for i in ids], pool.image_batch(ids)
        return b

    counts = {"occluders": 0, "dropped": 0, "frames": 0}

    def run(side, steps):
        tr = trainers[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            tr.one_step_raw(pool.geometry, batch(s))
            if side == "both_paste":
                counts["occluders"] += sum(m for m, _ in tr.last_masked)
                counts["dropped"] += sum(d for _, d in tr.last_masked)
                counts["frames"] += len(tr.last_masked)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    np.random.seed(0)
    for side in trainers:
        run(side, args.warmup)
    series = {side: [] for side in trainers}
    for _ in range(args.rounds):
        for side in trainers:
            series[side].append(run(side, args.steps))
    frames = max(counts["frames"], 1)
    out["step"] = {"batch": B, "dtype": cfg["dtype"], "points_per_frame": PB.N_SCENE, "steps_per_round": args.steps, "ms_per_step": series,
                   "median_ms": {side: statistics.median(v) for side, v in series.items()},
                   "occluders_per_frame": counts["occluders"] / frames, "dropped_objects_per_frame": counts["dropped"] / frames,
                   "loss": {side: float(tr.loss_value.item()) for side, tr in trainers.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

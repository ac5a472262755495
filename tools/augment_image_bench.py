#!/usr/bin/env python3
"""Cost of the train-time camera image augmentation (csrc/image_aug.hip k_augment_image_b).

  python tools/augment_image_bench.py [--iters 300] [--steps 40] [--warmup 10] [--rounds 3] [--out FILE]

1. The launch alone: dcf_augment_image_batch at 2 x 3 x 375 x 1242 (the cfg2 batch) and at 1 x 3 x 1080 x 1920, real ranges (zoom,
   shift, flip, photometric), into a fixed buffer as Train.one_step_raw issues it, HIP events around every launch after a warm-up,
   the median.
2. The whole cfg2 train step (bench.py's frames resident in HBM, batch 2, bf16) through Train.one_step_raw with `augment_image` off,
   on with ranges that draw the identity (same image, same projection, same downstream work: the feature's own cost) and on with
   real ranges (a zoomed-in frame crops points away, a blacked-out one changes nothing downstream): three trainers in one process on
   one GPU, alternating, --rounds rounds of --steps steps each, a host clock around steps that end in a device synchronise.
Prints one JSON line (and writes it to --out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
AUGMENT = dict(enabled=True, seed=1, zoom=[0.8, 1.25], shift=[0.1, 0.1], flip_prob=0.5, brightness=[0.8, 1.2], contrast=[0.8, 1.2],
               channel_gain=[0.9, 1.1], drop_prob=0.1)
# the block switched on with ranges that draw the identity: the launch, the per-frame matrices and the buffer are all there, the image
# and so everything downstream are the un-augmented step's -- the cost of the feature apart from what it does to the workload
NEUTRAL = dict(enabled=True, seed=1)
SIDES = (("off", None), ("neutral", NEUTRAL), ("on", AUGMENT))
SHAPES = ((2, 375, 1242), (1, 1080, 1920))


def launch_alone(shape, iters, warmup=50):
    import torch
    AI, ops, T = (importlib.import_module(PKG + "." + m) for m in ("augment_image", "ops", "train"))
    B, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(1234)
    img = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    out = torch.empty_like(img)
    cfg = T.parse_image_augment_config({"augment_image": dict(AUGMENT, drop_prob=0.0)})
    params = [AI.draw(cfg, 1, 0, 0, b, W, H) for b in range(B)]
    for _ in range(warmup):
        ops.augment_image_batch(img, params, out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        ops.augment_image_batch(img, params, out)
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    nbytes = img.numel() * 2
    med = statistics.median(us)
    return {"shape": [B, 3, H, W], "iters": iters, "median_us": med, "p10_us": us[len(us) // 10], "p90_us": us[len(us) * 9 // 10],
            "bytes": nbytes, "gbytes_per_s_at_median": nbytes / med / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("augment_image_bench.py measures on the GPU; none is visible")
    bench = importlib.import_module("bench")
    T, FL, det = (importlib.import_module(PKG + "." + m) for m in ("train", "frame_loader", "detfill"))
    out = {"launch": [launch_alone(s, args.iters) for s in SHAPES]}

    B = 2
    cfg = bench.kitti_config(B)
    pool = bench.FramePool(cfg, 4, 100000, 1234)
    trainers = {}
    for side, block in SIDES:
        c = dict(cfg)
        if block is not None:
            c["augment_image"] = dict(block)
        trainers[side] = T.Train(c)
        det.fill_state_dict(trainers[side].model)

    def batch(step):
        ids = pool.batch(step, B)
        b = FL.Batch(bboxes=torch.stack([pool.boxes[i] for i in ids], 0), num_bboxes=torch.tensor([pool.nb[i] for i in ids]), crt=None)
        b["points"], b["image"] = [pool.pts[i] for i in ids], pool.image_batch(ids)
        return b

    def run(side, steps):
        tr = trainers[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            tr.one_step_raw(pool.geometry, batch(s))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3 / steps
        tr._last_cnt = next(st for st in tr._geo_sets.values() if st["slot"] == tr._geo_slot)["cnt_host"].clone()   # points that reached the fusion sites
        return dt

    np.random.seed(0)
    for side, _ in SIDES:
        run(side, args.warmup)
    series = {side: [] for side, _ in SIDES}
    for _ in range(args.rounds):
        for side, _ in SIDES:
            series[side].append(run(side, args.steps))
    out["step"] = {"batch": B, "dtype": cfg["dtype"], "steps_per_round": args.steps, "augment_image": AUGMENT, "ms_per_step": series,
                   "median_ms": {side: statistics.median(v) for side, v in series.items()},
                   "valid_points_last_step": {side: [int(v) for v in tr._last_cnt.tolist()] for side, tr in trainers.items()},
                   "loss": {side: float(tr.loss_value.item()) for side, tr in trainers.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

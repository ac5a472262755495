#!/usr/bin/env python3
"""Cost of train-time object pasting (csrc/paste.hip, paste.py).

  python tools/paste_bench.py [--iters 300] [--steps 40] [--warmup 10] [--rounds 3] [--out FILE]

1. The two launches alone at the cfg2 shapes, HIP events around every call after a warm-up, the median: dcf_paste_points_batch on
   2 x 100 000 rows (96 800 scene rows and 16 records of 200 points each per frame) beside dcf_augment_points_batch on the same
   2 x 100 000 rows, and dcf_paste_patches_batch on 2 x 3 x 375 x 1242 bytes with 16 records per frame beside
   dcf_augment_image_batch on the same image -- the yardsticks move the same bytes, timed in the same process.  (At two frames the
   tables travel in the kernel argument; from five frames on a call is the table's asynchronous copy plus the launch.)
2. The sampler on the host: paste.draw for the two frames of a step (8 labels each, target_objects 15, 16 candidates), the median
   over --iters steps of a host clock.
3. The whole cfg2 train step (frames resident in HBM, batch 2, bf16, 96 800 points per frame so that pasted objects fit max_num_pc)
   through Train.one_step_raw with `augment_paste` off and on: two trainers in one process on one GPU, alternating, --rounds rounds
   of --steps steps each, a host clock around steps that end in a device synchronise.
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
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
N_SCENE, N_OBJ, OBJ_POINTS = 96800, 16, 200
HW = (375, 1242)
PASTE = dict(enabled=True, seed=1, target_objects=15, max_candidates=16, margin=0.1, paste_image=True)


def make_bank(M, seed):
    """M cars of the cfg2 range with OBJ_POINTS points each and the patch rectangle objbank.patch_rect gives them under
    calib.kitti_like_crt(), random bytes as pixels."""
    import numpy as np
    calib, objbank, P = (importlib.import_module(PKG + "." + m) for m in ("calib", "objbank", "paste"))
    crt = calib.kitti_like_crt()
    rng = np.random.RandomState(seed)
    boxes = np.zeros((M, 9), dtype=np.float32)
    boxes[:, 0], boxes[:, 1], boxes[:, 2] = rng.uniform(8.0, 60.0, M), rng.uniform(-12.0, 12.0, M), -1.0
    boxes[:, 3], boxes[:, 4], boxes[:, 5], boxes[:, 6], boxes[:, 7], boxes[:, 8] = 4.0, 1.75, 1.5, rng.uniform(0.0, 3.14, M), 6.0, 1.0
    rect = np.array([objbank.patch_rect(b, crt, HW) for b in boxes], dtype=np.int32)
    centre = np.array([P.centre_pixel(b, crt) for b in boxes], dtype=np.int32)
    pts = []
    for b in boxes:
        loc = (rng.rand(OBJ_POINTS, 3) - 0.5) * b[3:6] * 0.9
        c, s = np.cos(b[6]), np.sin(b[6])
        pts.append(np.stack([b[0] + c * loc[:, 0] - s * loc[:, 1], b[1] + s * loc[:, 0] + c * loc[:, 1], b[2] + loc[:, 2]], 1))
    qstart = np.concatenate([[0], np.cumsum(3 * rect[:, 2].astype(np.int64) * rect[:, 3])]).astype(np.int64)
    return {"points": np.concatenate(pts, 0).astype(np.float32), "point_start": np.arange(M + 1, dtype=np.int64) * OBJ_POINTS, "boxes": boxes,
            "rect": rect, "patch": rng.randint(0, 256, int(qstart[-1])).astype(np.uint8), "patch_start": qstart, "centre_px": centre,
            "image_hw": np.array(HW, dtype=np.int32), "source": np.stack([np.arange(M), np.zeros(M)], 1).astype(np.int32)}


def full_plans(bank, B):
    """B plans of 16 records each, put together by hand (the sampler would reject overlapping ones: the kernels do not care)."""
    import numpy as np
    P = importlib.import_module(PKG + ".paste")
    plans = []
    for b in range(B):
        rows = [(b * N_OBJ + j) % len(bank["boxes"]) for j in range(N_OBJ)]
        plan = P.empty_plan(N_SCENE, HW)
        plan["rows"] = rows
        plan["records"] = np.stack([P.record(bank["boxes"][r], PASTE["margin"]) for r in rows], 0)
        plan["append"] = np.array([(bank["point_start"][r], OBJ_POINTS) for r in rows], dtype=np.int64)
        plan["patches"] = np.array([(bank["rect"][r][0], bank["rect"][r][1], bank["rect"][r][2], bank["rect"][r][3], 0, 0, bank["rect"][r][2], bank["rect"][r][3],
                                     bank["patch_start"][r]) for r in rows if bank["rect"][r][2] > 0], dtype=np.int64).reshape(-1, 9)
        plans.append(plan)
    return plans


def timed(fn, iters, warmup=50):
    import torch
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": statistics.median(us), "p10_us": us[len(us) // 10], "p90_us": us[len(us) * 9 // 10]}


def launches_alone(bank, iters):
    import torch
    A, AI, ops, T, det = (importlib.import_module(PKG + "." + m) for m in ("augment", "augment_image", "ops", "train", "detfill"))
    B = 2
    plans = full_plans(bank, B)
    lim6 = (0.0, 70.4, -40.0, 40.0, -2.4, 0.8)
    pts = [torch.from_numpy(det.synthetic_points(N_SCENE, lim6, 77 + b)).cuda() for b in range(B)]
    bank_pts, bank_patch = torch.from_numpy(bank["points"]).cuda(), torch.from_numpy(bank["patch"]).cuda()
    total = N_SCENE + N_OBJ * OBJ_POINTS
    buf = torch.empty((B, total, 3), device="cuda")
    out = {"points": timed(lambda: ops.paste_points_batch(pts, plans, bank_pts, [buf[b] for b in range(B)]), iters)}
    full = [buf[b].clone() for b in range(B)]
    dst = [torch.empty_like(p) for p in full]
    bev = [A.draw({"rotation_deg": 20.0, "scale": (0.95, 1.05), "flip_prob": 0.5, "point_drop": (0.05, 0.2)}, 1, 0, 0, b) for b in range(B)]
    out["points_yardstick_augment_points"] = timed(lambda: ops.augment_points_batch(full, bev, dst), iters)
    out["points"].update(rows=[B, total], records=N_OBJ, removed=[int(torch.isinf(buf[b, :N_SCENE, 0]).sum()) for b in range(B)])
    g = torch.Generator(device="cpu").manual_seed(1234)
    img = torch.randint(0, 256, (B, 3) + HW, dtype=torch.uint8, generator=g).cuda()
    iout = torch.empty_like(img)
    out["patches"] = timed(lambda: ops.paste_patches_batch(img, plans, bank_patch, iout), iters)
    out["patches"].update(shape=[B, 3] + list(HW), records=[len(p["patches"]) for p in plans], painted_bytes=int((iout != img).sum()))
    icfg = T.parse_image_augment_config({"augment_image": dict(enabled=True, seed=1, zoom=[0.8, 1.25], shift=[0.1, 0.1], flip_prob=0.5, brightness=[0.8, 1.2],
                                                               contrast=[0.8, 1.2], channel_gain=[0.9, 1.1])})
    ip = [AI.draw(icfg, 1, 0, 0, b, HW[1], HW[0]) for b in range(B)]
    out["patches_yardstick_augment_image"] = timed(lambda: ops.augment_image_batch(img, ip, iout), iters)
    return out


def sampler_host(bank, cfg, iters):
    import numpy as np
    P, D, calib = (importlib.import_module(PKG + "." + m) for m in ("paste", "data_import_carla", "calib"))
    crt = calib.kitti_like_crt()
    labels = [D.synthetic_boxes(cfg, 1234 + b) for b in range(2)]
    boxes = [l[0].numpy() for l in labels]
    ms, accepted = [], 0
    for call in range(iters):
        t0 = time.perf_counter()
        plans = [P.draw(PASTE, 1, 0, call, b, bank, boxes[b], labels[b][1], N_SCENE, crt, cfg) for b in range(2)]
        ms.append((time.perf_counter() - t0) * 1e3)
        accepted += sum(len(p["rows"]) for p in plans)
    ms.sort()
    return {"frames_per_step": 2, "labels_per_frame": [int(l[1]) for l in labels], "median_ms_per_step": statistics.median(ms), "p90_ms_per_step": ms[len(ms) * 9 // 10],
            "accepted_per_frame": accepted / (2.0 * iters)}


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
        raise SystemExit("paste_bench.py measures on the GPU; none is visible")
    bench = importlib.import_module("bench")
    T, FL, det, objbank = (importlib.import_module(PKG + "." + m) for m in ("train", "frame_loader", "detfill", "objbank"))
    bank = make_bank(64, 5)
    B = 2
    cfg = bench.kitti_config(B)
    out = {"launch": launches_alone(bank, args.iters), "sampler": sampler_host(bank, cfg, args.iters)}

    pool = bench.FramePool(cfg, 4, N_SCENE, 1234)
    trainers = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bank.npz")
        objbank.save(path, bank)
        for side in ("off", "on"):
            c = dict(cfg)
            if side == "on":
                c["augment_paste"] = dict(PASTE, bank=path)
            trainers[side] = T.Train(c)
            det.fill_state_dict(trainers[side].model)

    def batch(step):
        ids = pool.batch(step, B)
        b = FL.Batch(bboxes=torch.stack([pool.boxes[i] for i in ids], 0), num_bboxes=torch.tensor([pool.nb[i] for i in ids]), crt=None)
        b["points"], b["image"] = [pool.pts[i] for i in ids], pool.image_batch(ids)
        return b

    pasted = {"n": 0, "frames": 0}

    def run(side, steps):
        tr = trainers[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            tr.one_step_raw(pool.geometry, batch(s))
            if side == "on":
                pasted["n"] += sum(len(r) for r in tr.last_paste)
                pasted["frames"] += len(tr.last_paste)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    np.random.seed(0)
    for side in trainers:
        run(side, args.warmup)
    series = {side: [] for side in trainers}
    for _ in range(args.rounds):
        for side in trainers:
            series[side].append(run(side, args.steps))
    out["step"] = {"batch": B, "dtype": cfg["dtype"], "points_per_frame": N_SCENE, "steps_per_round": args.steps, "augment_paste": PASTE, "ms_per_step": series,
                   "median_ms": {side: statistics.median(v) for side, v in series.items()},
                   "pasted_objects_per_frame": pasted["n"] / max(pasted["frames"], 1),
                   "loss": {side: float(tr.loss_value.item()) for side, tr in trainers.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of `loss_sampling: anchor` at the cfg2 head shape (B = 2, 176 x 200 cells) against `focal`: the two entries alone, and the cfg2
batch-2 train step.

  python tools/loss_anchor_bench.py [--iters 200] [--rounds 4] [--boxes 12] [--deterministic] [--no-step] [--steps 40] [--warmup 15]

Entries: dcf_assign_anchors_iou and dcf_loss_anchor_fwd_bwd are each timed alone between HIP events (median over --iters calls) on
fixed random head outputs (softmax pairs of N(0, 2) logits) and --boxes labels per sample of random yaw; then LossTotal.forward of
`anchor` and of `focal` take turns, in alternating order, --rounds times: the median time of the whole forward between events (launches
plus torch's zero fills of the gradient maps) and the per-kernel times the library records in its dcf_prof_enable brackets.

Step: two trainers in this one process, one per mode, the same weights and the same frames resident in HBM; they take turns, in
alternating order, --rounds times, --steps steps each; per mode and round the median step-to-step interval between events."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
MODES = ("focal", "anchor")


def _median_us(torch, fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev)


def launch_legs(a):
    import torch
    bench = importlib.import_module("bench")
    Hl = importlib.import_module(PKG + "._hip")
    Lm = importlib.import_module(PKG + ".loss")
    ops = importlib.import_module(PKG + ".ops")
    cfg = bench.kitti_config(2)
    rs = cfg["anchor_bbox_feature"]["reduced_scale"]
    H, W = int(cfg["voxel_length"] / rs), int(cfg["voxel_width"] / rs)
    B = a.batch
    g = torch.Generator().manual_seed(0)
    boxes = torch.zeros(B, cfg["max_num_bbox"], 9)
    n = min(a.boxes, cfg["max_num_bbox"])
    for b in range(B):
        for k in range(n):
            x = cfg["lidar_x_min"] + (0.05 + 0.9 * torch.rand(1, generator=g).item()) * (cfg["lidar_x_max"] - cfg["lidar_x_min"])
            y = cfg["lidar_y_min"] + (0.05 + 0.9 * torch.rand(1, generator=g).item()) * (cfg["lidar_y_max"] - cfg["lidar_y_min"])
            yaw = (2.0 * torch.rand(1, generator=g).item() - 1.0) * 3.0
            boxes[b, k] = torch.tensor([x, y, -1.0, 4.0, 1.8, 1.5, yaw if k % 2 else 0.05 * k, 6, 1])
    nb = torch.tensor([n] * B)
    head = torch.randn(B, 32, H, W, generator=g) * 2.0
    head[:, :4] = torch.softmax(head[:, :4].reshape(B, 2, 2, H, W), 2).reshape(B, 4, H, W)
    head = head.cuda()
    cls, reg = head[:, :4], head[:, 4:18]
    losses = {m: Lm.LossTotal(dict(cfg, loss_sampling=m, loss_reduction="mean", deterministic=a.deterministic)).cuda() for m in MODES}
    out = {"B": B, "H": H, "W": W, "boxes": n, "deterministic": a.deterministic, "rounds": []}
    for m in MODES:                                   # every shape warm before anything is timed
        for _ in range(20):
            losses[m](boxes, nb, cls, reg)
    # ---- the two entries alone
    L = losses["anchor"]
    dev = cls.device
    anc = L._anc_dev
    bx, nbd = boxes.cuda(), nb.to(torch.int32).cuda()
    aws, target, counts, _ = ops.assign_anchors_workspace(B, H, W, boxes.shape[1], dev)
    lws, terms = ops.loss_anchor_workspace(B, H, W, dev)
    gbuf, loss = torch.zeros_like(head), torch.zeros(1, device=dev)
    alpha, gamma, eps = L.focal
    assign = lambda: ops.assign_anchors_iou(anc, bx, nbd, H, W, L.assign_iou[0], L.assign_iou[1], target, counts, aws)
    terms_call = lambda: ops.loss_anchor(cls, reg, anc, bx, target, counts, alpha, gamma, eps, float(cfg["regress_loss_gain"]), 2, loss, gbuf,
                                         gbuf[:, 4:], terms, lws)
    for _ in range(20):
        assign(); terms_call()
    out["entries_us"] = {"dcf_assign_anchors_iou": _median_us(torch, assign, a.iters), "dcf_loss_anchor_fwd_bwd": _median_us(torch, terms_call, a.iters)}
    out["counts"] = counts.cpu().tolist()
    print("entries alone: assign %.1f us, terms %.1f us (medians of %d); counts %s" % (out["entries_us"]["dcf_assign_anchors_iou"],
                                                                                       out["entries_us"]["dcf_loss_anchor_fwd_bwd"], a.iters, out["counts"]))
    # ---- the whole forward, the modes taking turns
    for rnd in range(a.rounds):
        res = {}
        for mode in (MODES if rnd % 2 == 0 else MODES[::-1]):
            Lr = losses[mode]
            fwd_us = _median_us(torch, lambda: Lr(boxes, nb, cls, reg), a.iters)
            Hl.lib().dcf_prof_reset()
            Hl.lib().dcf_prof_enable(1)
            for _ in range(a.iters):
                Lr(boxes, nb, cls, reg)
            torch.cuda.synchronize()
            prof = Hl.prof_read()
            Hl.lib().dcf_prof_enable(0)
            kern = {k: {"us_per_launch": 1e3 * v[0] / max(v[1], 1), "launches_per_call": v[1] / a.iters} for k, v in prof.items()
                    if k.startswith(("loss_", "assign_"))}
            tot = sum(v["us_per_launch"] * v["launches_per_call"] for v in kern.values())
            res[mode] = {"forward_us": fwd_us, "kernels_us": tot, "kernels": kern}
            print("round %d %-6s forward %.1f us between events; kernels %.1f us per call:" % (rnd, mode, fwd_us, tot))
            for k, v in sorted(kern.items()):
                print("    %-24s %6.2f us x %g" % (k, v["us_per_launch"], v["launches_per_call"]))
        out["rounds"].append(res)
    return out


def step_legs(a):
    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    train = importlib.import_module(PKG + ".train")
    detfill = importlib.import_module(PKG + ".detfill")
    torch.cuda.set_device(0)
    trainers, pool = {}, None
    for m in MODES:
        cfg = bench.kitti_config(a.batch)
        cfg.update(bn_mode="eval", loss_sampling=m, hip_graphs="auto", deterministic=a.deterministic)
        torch.manual_seed(0)
        np.random.seed(1234)
        trainers[m] = train.Train(cfg)
        detfill.fill_state_dict(trainers[m].model)
        if pool is None:
            pool = bench.FramePool(cfg, n_frames=max(2 * a.batch, 4), n_points=cfg["max_num_pc"], seed0=0)
    for m in MODES:
        for s in range(a.warmup):
            bench.train_step(trainers[m], pool, pool.batch(s, a.batch))
    torch.cuda.synchronize()
    out = []
    for rnd in range(a.rounds):
        res = {}
        for mode in (MODES if rnd % 2 == 0 else MODES[::-1]):
            tr = trainers[mode]
            for s in range(3):                                     # back in steady state after the other trainer's turn
                bench.train_step(tr, pool, pool.batch(s, a.batch))
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            for mk in marks:
                mk.record()
            torch.cuda.synchronize()
            marks[0].record()
            for s in range(a.steps):
                bench.train_step(tr, pool, pool.batch(a.warmup + s, a.batch))
                marks[s + 1].record()
            torch.cuda.synchronize()
            ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps))
            loss = float(tr.loss_value.item())
            res[mode] = {"ms_per_step_median": statistics.median(ms), "ms_per_step_mean": sum(ms) / len(ms), "ms_min": ms[0], "loss": loss,
                         "terms": tr.loss_terms().cpu().tolist()}
            print("round %d step %-6s median %.3f ms, mean %.3f ms, min %.3f ms; loss %.4f" % (rnd, mode, res[mode]["ms_per_step_median"],
                                                                                             res[mode]["ms_per_step_mean"], ms[0], loss))
            if not math.isfinite(loss):
                raise SystemExit("non-finite loss in mode %s" % mode)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=12)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--no-step", action="store_true", help="the entries and the forward only")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {"launch": launch_legs(a)}
    out["step"] = None if a.no_step else step_legs(a)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the loss launch alone at the cfg2 head shape (B = 2, 176 x 200 cells): `loss_sampling: device` against `hard`.

  python tools/loss_hard_bench.py [--iters 200] [--boxes 12] [--deterministic]

Each mode runs LossTotal.forward on fixed random head outputs.  Two numbers per mode: the median time of the whole forward
between HIP events (the launches plus torch's zero-fills of the gradient maps), and the per-kernel times the library records in
its dcf_prof_enable brackets (loss_hard_keys / loss_hard_pass x 3 / loss_hard_compact / loss_hard_fwd_bwd for `hard`,
loss_sample_fwd_bwd for `device`).  Head outputs are N(0, 2) logits: the keys spread over many digits of every radix pass;
--constant uses one score everywhere instead (every cell in one histogram bin, the worst case for the LDS atomics)."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=12)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--constant", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    bench = importlib.import_module("bench")
    Hl = importlib.import_module(PKG + "._hip")
    Lm = importlib.import_module(PKG + ".loss")
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
            boxes[b, k] = torch.tensor([x, y, -1.0, 4.0, 1.8, 1.5, 0.3 * k, 6, 1])
    nb = torch.tensor([n] * B)
    head = torch.randn(B, 32, H, W, generator=g) * 2.0
    if a.constant:
        head[:, :4] = 0.25
    head = head.cuda()
    out = {"B": B, "H": H, "W": W, "boxes": n, "deterministic": a.deterministic, "constant": a.constant}
    for mode in ("device", "hard"):
        L = Lm.LossTotal(dict(cfg, loss_sampling=mode, loss_reduction="mean", deterministic=a.deterministic)).cuda()
        cls, reg = head[:, :4], head[:, 4:18]

        def run():
            return L(boxes, nb, cls, reg)
        for _ in range(20):
            run()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for s, e in ev:
            s.record()
            run()
            e.record()
        torch.cuda.synchronize()
        fwd_us = statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev)
        Hl.lib().dcf_prof_reset()
        Hl.lib().dcf_prof_enable(1)
        for _ in range(a.iters):
            run()
        torch.cuda.synchronize()
        prof = Hl.prof_read()
        Hl.lib().dcf_prof_enable(0)
        kern = {k: {"us_per_launch": 1e3 * v[0] / max(v[1], 1), "launches_per_call": v[1] / a.iters} for k, v in prof.items() if k.startswith("loss_")}
        tot = sum(v["us_per_launch"] * v["launches_per_call"] for v in kern.values())
        out[mode] = {"forward_us": fwd_us, "kernels_us": tot, "kernels": kern}
        print("%-6s forward %.1f us between events; kernels %.1f us per call:" % (mode, fwd_us, tot))
        for k, v in sorted(kern.items()):
            print("    %-24s %6.2f us x %g" % (k, v["us_per_launch"], v["launches_per_call"]))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the loss launch alone at the cfg2 head shape (B = 2, 176 x 200 cells): `loss_sampling: device`, `hard` and `focal`, and of
the cfg2 train step with `focal` against `device`.

  python tools/loss_focal_bench.py [--iters 200] [--rounds 2] [--boxes 12] [--deterministic] [--step] [--steps 60] [--warmup 15]

Launch: each mode runs LossTotal.forward on fixed random head outputs (softmax pairs of N(0, 2) logits, the head's output format).  The
modes take turns, in alternating order, --rounds times in one process; per mode and round two numbers: the median time of the whole
forward between HIP events (the launches plus torch's zero-fills of the gradient maps), and the per-kernel times the library records
in its dcf_prof_enable brackets (loss_focal_fwd_bwd + loss_focal_fold for `focal`, loss_hard_* for `hard`, loss_sample_fwd_bwd for
`device`).

--step: `python bench.py --gpus 1 --loss-sampling focal` against `--loss-sampling device`, one child process per leg, the legs
alternating, --rounds times; frames/s from each leg's JSON line."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
MODES = ("device", "hard", "focal")


def launch_legs(a):
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
    head[:, :4] = torch.softmax(head[:, :4].reshape(B, 2, 2, H, W), 2).reshape(B, 4, H, W)
    head = head.cuda()
    cls, reg = head[:, :4], head[:, 4:18]
    losses = {m: Lm.LossTotal(dict(cfg, loss_sampling=m, loss_reduction="mean", deterministic=a.deterministic)).cuda() for m in MODES}
    out = {"B": B, "H": H, "W": W, "boxes": n, "deterministic": a.deterministic, "rounds": []}
    for m in MODES:                                   # every shape warm before anything is timed
        for _ in range(20):
            losses[m](boxes, nb, cls, reg)
    for rnd in range(a.rounds):
        res = {}
        for mode in (MODES if rnd % 2 == 0 else MODES[::-1]):
            L = losses[mode]
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for s, e in ev:
                s.record()
                L(boxes, nb, cls, reg)
                e.record()
            torch.cuda.synchronize()
            fwd_us = statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev)
            Hl.lib().dcf_prof_reset()
            Hl.lib().dcf_prof_enable(1)
            for _ in range(a.iters):
                L(boxes, nb, cls, reg)
            torch.cuda.synchronize()
            prof = Hl.prof_read()
            Hl.lib().dcf_prof_enable(0)
            kern = {k: {"us_per_launch": 1e3 * v[0] / max(v[1], 1), "launches_per_call": v[1] / a.iters} for k, v in prof.items() if k.startswith("loss_")}
            tot = sum(v["us_per_launch"] * v["launches_per_call"] for v in kern.values())
            res[mode] = {"forward_us": fwd_us, "kernels_us": tot, "kernels": kern}
            print("round %d %-6s forward %.1f us between events; kernels %.1f us per call:" % (rnd, mode, fwd_us, tot))
            for k, v in sorted(kern.items()):
                print("    %-24s %6.2f us x %g" % (k, v["us_per_launch"], v["launches_per_call"]))
        out["rounds"].append(res)
    return out


def step_legs(a):
    out = []
    for rnd in range(a.rounds):
        res = {}
        for mode in (("focal", "device") if rnd % 2 == 0 else ("device", "focal")):
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--loss-sampling", mode]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
            if p.returncode != 0:
                raise SystemExit("bench.py --loss-sampling %s failed (%d):\n%s" % (mode, p.returncode, (p.stdout + p.stderr)[-3000:]))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            r = json.loads(line)
            res[mode] = {k: r.get(k) for k in ("value", "unit", "ms_per_step", "ms_per_step_median", "steps", "warmup")}
            res[mode]["final_loss"] = r["config"]["final_loss"]
            print("round %d step %-6s %.2f frames/s, %.3f ms per step (median %.3f), final loss %.4f"
                  % (rnd, mode, r["value"], r["ms_per_step"], r["ms_per_step_median"], r["config"]["final_loss"]))
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--boxes", type=int, default=12)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--step", action="store_true", help="also run bench.py with focal against device (child processes)")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {"step": step_legs(a) if a.step else None}     # (the children run before this process opens the GPU)
    out["launch"] = launch_legs(a)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

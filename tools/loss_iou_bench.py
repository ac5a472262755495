#!/usr/bin/env python3
"""Cost of the rotated-IoU regression term (`iou_loss_gain`) at the cfg2 head shape (B = 2, 176 x 200 cells, 12 labels
per sample): the entry alone, and the forward of `loss_sampling: anchor` with the term on against off.

  python tools/loss_iou_bench.py [--iters 200] [--rounds 4] [--boxes 12] [--kind 3d] [--deterministic]

Entry: dcf_loss_anchor_iou_fwd_bwd (and, for scale, dcf_assign_anchors_iou and dcf_loss_anchor_fwd_bwd) timed alone between HIP events,
median over --iters calls, on the targets the assignment gives for --boxes labels per sample of random yaw.  The offsets are N(0, 0.1): the
decoded box of a positive anchor stays near its anchor and so overlaps its label, which is the case where every edge is clipped.

Forward: two LossTotal modules in this one process, the term on and off, take turns in alternating order --rounds times: the median time of
the whole forward between events, and the per-kernel times the library records in its dcf_prof_enable brackets."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
LEGS = ("off", "on")


def _median_us(torch, fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=12)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--kind", default="3d", choices=("3d", "bev"))
    ap.add_argument("--gain", type=float, default=2.0)
    ap.add_argument("--deterministic", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
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
    anchor0 = Lm.LossTotal(dict(cfg, loss_sampling="anchor")).anchor_set[0, :, 0, 0]
    az, ah = float(anchor0[2]), float(anchor0[5])         # labels at the anchors' height: the 3-D IoU of a positive anchor is not 0
    n = min(a.boxes, cfg["max_num_bbox"])
    for b in range(B):
        for k in range(n):
            x = cfg["lidar_x_min"] + (0.05 + 0.9 * torch.rand(1, generator=g).item()) * (cfg["lidar_x_max"] - cfg["lidar_x_min"])
            y = cfg["lidar_y_min"] + (0.05 + 0.9 * torch.rand(1, generator=g).item()) * (cfg["lidar_y_max"] - cfg["lidar_y_min"])
            yaw = (2.0 * torch.rand(1, generator=g).item() - 1.0) * 3.0
            boxes[b, k] = torch.tensor([x, y, az, 4.0, 1.8, ah, yaw if k % 2 else 0.05 * k, 6, 1])
    nb = torch.tensor([n] * B)
    head = torch.randn(B, 32, H, W, generator=g) * 2.0
    head[:, :4] = torch.softmax(head[:, :4].reshape(B, 2, 2, H, W), 2).reshape(B, 4, H, W)
    head[:, 4:18] *= 0.05
    head = head.cuda()
    cls, reg = head[:, :4], head[:, 4:18]
    base = dict(cfg, loss_sampling="anchor", loss_reduction="mean", deterministic=a.deterministic)
    losses = {"off": Lm.LossTotal(base).cuda(), "on": Lm.LossTotal(dict(base, iou_loss_gain=a.gain, iou_loss_kind=a.kind)).cuda()}
    out = {"B": B, "H": H, "W": W, "boxes": n, "kind": a.kind, "deterministic": a.deterministic, "rounds": []}
    for leg in LEGS:                                  # every shape warm before anything is timed
        for _ in range(20):
            losses[leg](boxes, nb, cls, reg)
    # ---- the entries alone
    L = losses["on"]
    dev = cls.device
    anc = L._anc_dev
    bx, nbd = boxes.cuda(), nb.to(torch.int32).cuda()
    aws, target, counts, _ = ops.assign_anchors_workspace(B, H, W, boxes.shape[1], dev)
    lws, terms = ops.loss_anchor_workspace(B, H, W, dev)
    iws, iou_terms, _ = ops.loss_anchor_iou_workspace(B, H, W, dev)
    gbuf, loss = torch.zeros_like(head), torch.zeros(1, device=dev)
    alpha, gamma, eps = L.focal
    assign = lambda: ops.assign_anchors_iou(anc, bx, nbd, H, W, L.assign_iou[0], L.assign_iou[1], target, counts, aws)
    terms_call = lambda: ops.loss_anchor(cls, reg, anc, bx, target, counts, alpha, gamma, eps, float(cfg["regress_loss_gain"]), 2, loss, gbuf,
                                         gbuf[:, 4:], terms, lws)
    iou_call = lambda: ops.loss_anchor_iou(reg, anc, bx, target, counts, Lm.IOU_KIND[a.kind], a.gain, 2, loss, gbuf[:, 4:], iou_terms, iws)
    for _ in range(20):
        assign(); terms_call(); iou_call()
    out["entries_us"] = {"dcf_assign_anchors_iou": _median_us(torch, assign, a.iters), "dcf_loss_anchor_fwd_bwd": _median_us(torch, terms_call, a.iters),
                         "dcf_loss_anchor_iou_fwd_bwd": _median_us(torch, iou_call, a.iters)}
    out["counts"], out["iou_terms"] = counts.cpu().tolist(), iou_terms.cpu().tolist()
    print("entries alone (medians of %d, us): %s; counts %s; (mean IoU, N) %s" % (a.iters, out["entries_us"], out["counts"], out["iou_terms"]))
    # ---- the whole forward, the term off and on taking turns
    for rnd in range(a.rounds):
        res = {}
        for leg in (LEGS if rnd % 2 == 0 else LEGS[::-1]):
            Lr = losses[leg]
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
            res[leg] = {"forward_us": fwd_us, "kernels_us": tot, "kernels": kern}
            print("round %d term %-3s forward %.1f us between events; kernels %.1f us per call:" % (rnd, leg, fwd_us, tot))
            for k, v in sorted(kern.items()):
                print("    %-24s %6.2f us x %g" % (k, v["us_per_launch"], v["launches_per_call"]))
        out["rounds"].append(res)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the KITTI-style protocol (`eval_protocol: kitti`) against the plain ranked evaluation (section 13) at
the cfg2 head size (B = 2, 176 x 200 cells).

  python tools/eval_kitti_bench.py [--budget 0.3]

Device-event times (median, after warm-up, over enough repetitions to fill --budget seconds each) of
  * RankedTest.accumulate on one batch at a score threshold that leaves about 500 candidates per sample, with the protocol on (levels,
    16 DontCare rectangles and a per-frame matrix handed in) and plain, alternating in the same process on the same pred;
  * RankedTest.summary() with 2^12 and with 2^17 accumulated detections, protocol on and plain.
The head output is synthetic (that of tools/eval_rank_bench.py): uniform scores, boxes spread over the 70 m x 80 m range, 12 labelled
boxes per sample with levels 0 .. 3."""
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
    ap.add_argument("--budget", type=float, default=0.3, help="seconds of repetitions per measurement")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    Tm = importlib.import_module(PKG + ".test")
    det = importlib.import_module(PKG + ".detfill")
    B, H, W = 2, 176, 200
    hw = H * W
    u = det.uniform((B, 32, H, W), 5100, 0.0, 1.0)
    pred = u.copy()
    for an in range(2):
        o = 18 + 7 * an
        pred[:, o + 0] = 70.0 * u[:, o + 0]
        pred[:, o + 1] = -40.0 + 80.0 * u[:, o + 1]
        pred[:, o + 2] = -1.0 + 0.2 * u[:, o + 2]
        pred[:, o + 3] = 3.5 + 1.3 * u[:, o + 3]
        pred[:, o + 4] = 1.6 + 0.5 * u[:, o + 4]
        pred[:, o + 5] = 1.4 + 0.4 * u[:, o + 5]
        pred[:, o + 6] = 3.14159 * u[:, o + 6]
    pred = torch.from_numpy(pred).cuda()
    refs = torch.zeros(B, 20, 9)
    lab = det.uniform((B, 12, 7), 5200, 0.0, 1.0)
    for b in range(B):
        for k in range(12):
            v = lab[b, k]
            refs[b, k] = torch.tensor([70.0 * v[0], -40.0 + 80.0 * v[1], -1.0, 3.5 + 1.3 * v[3], 1.6 + 0.5 * v[4], 1.5, 3.14159 * v[6], 6.0, 1.0])
    levels = (torch.arange(B * 20).reshape(B, 20) % 4).to(torch.int32)
    rc = det.uniform((B, 16, 4), 5400, 0.0, 1.0)
    dontcare = torch.from_numpy(np.stack([1000.0 * rc[..., 0], 250.0 * rc[..., 1], 1000.0 * rc[..., 0] + 40.0 + 200.0 * rc[..., 2],
                                          250.0 * rc[..., 1] + 30.0 + 90.0 * rc[..., 3]], -1).astype(np.float32))
    f, cx, cy = 700.0, 621.0, 187.0                                       # a pinhole 2 m behind the range, looking along +x
    crt = [np.array([[cx, cy, 1.0], [-f, 0.0, 0.0], [0.0, -f, 0.0], [2.0 * cx, 2.0 * cy - f, 2.0]], np.float32)] * B
    thr500 = 1.0 - 500.0 / (2 * hw)

    def harness(**cfg):
        T = Tm.RankedTest.__new__(Tm.RankedTest)
        torch.nn.Module.__init__(T)
        T.config = dict({"score_threshold": thr500, "eval_metric": "ranked", "image_height": 375, "image_width": 1242}, **cfg)
        T.initialize_ap()
        return T

    def timed(fn, before=None):
        """Median device-event time (ms) of fn over repetitions filling the budget, after warm-up."""
        def once():
            if before:
                before()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            return s.elapsed_time(e)
        for _ in range(3):
            first = once()
        reps = int(min(200, max(5, a.budget * 1e3 / max(first, 1e-3))))
        return statistics.median(once() for _ in range(reps)), reps

    K = harness(eval_protocol="kitti")
    P = harness()
    refs_dev, lv_dev, dc_dev = refs.cuda(), levels.cuda(), dontcare.cuda()
    out = {"B": B, "H": H, "W": W, "threshold_500": thr500}
    for rnd in range(2):                                                  # alternately in one process: kitti, plain, kitti, plain
        out["kitti_accumulate_ms_%d" % rnd], out["kitti_accumulate_reps"] = timed(
            lambda: K.accumulate(pred, refs_dev, levels=lv_dev, dontcare=dc_dev, crt=crt), K.initialize_ap)
        out["plain_accumulate_ms_%d" % rnd], out["plain_accumulate_reps"] = timed(lambda: P.accumulate(pred, refs_dev), P.initialize_ap)
    K.initialize_ap()
    K.accumulate(pred, refs_dev, levels=lv_dev, dontcare=dc_dev, crt=crt)
    s = K.summary()
    out["candidates"] = [int(c) for c in K._last[2].cpu().tolist()]
    out["survivors"] = s["num_P"]
    out["ignored_bev_moderate_0.7"] = s["bev"]["moderate"]["num_ignored"][0.7]
    for n in (1 << 12, 1 << 17):
        for name, S in (("kitti", harness(eval_protocol="kitti")), ("plain", harness())):
            acc = S._accumulators(pred.device)
            acc["scores"][:n] = torch.from_numpy(np.round(det.uniform((n,), 5300, 0.5, 1.0) * 1024.0) / 1024.0).cuda()
            bitsrc = torch.from_numpy((det.uniform((n,), 5301, 0.0, 1.0) * 1024.0).astype(np.int32)).cuda()
            if name == "kitti":
                acc["tpmask"][:, :n] = bitsrc | (bitsrc << 10) | (bitsrc << 20)
                acc["igmask"][:, :n] = (~bitsrc & 0x155) * 0x100401
                acc["state"][0], acc["state"][1], acc["state"][2], acc["state"][3] = n, n // 4, n // 3, n // 2
            else:
                acc["tpmask"][:n] = bitsrc
                acc["state"][0], acc["state"][1] = n, n // 2

            def summ():
                S._summary = None
                S.summary()
            for rnd in range(2):
                out["%s_summary_%d_ms_%d" % (name, n, rnd)], _ = timed(summ)
    for k in sorted(out):
        print("%-32s %s" % (k, out[k]))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

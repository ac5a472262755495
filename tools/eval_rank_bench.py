#!/usr/bin/env python3
"""Cost of the ranked evaluation (`eval_metric: ranked`) at the cfg2 head size (B = 2, 176 x 200 cells).

  python tools/eval_rank_bench.py [--budget 0.3]

Device-event times (median, after warm-up, over enough repetitions to fill --budget seconds each) of
  * RankedTest.accumulate on one batch at a score threshold that leaves about 500 candidates per sample, alternating in the same
    process with the compat post-processing of Test.get_eval_value_onestep (get_bboxes_device, NMS_SAT,
    precision_recall_singleshot) on the same pred -- the compat path waits for the device inside, so its events span those waits;
  * the same accumulate with all 70 400 candidates of a sample above the threshold (the 4096 highest-ranked stay);
  * RankedTest.summary() with 2^12 and with 2^17 accumulated detections.
The head output is synthetic: uniform scores, boxes spread over the 70 m x 80 m range, 12 labelled boxes per sample."""
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
    thr500 = 1.0 - 500.0 / (2 * hw)

    def harness(cls, **cfg):
        T = cls.__new__(cls)
        torch.nn.Module.__init__(T)
        T.config = dict({"score_threshold": thr500}, **cfg)
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

    R = harness(Tm.RankedTest)
    C = harness(Tm.Test)
    refs_dev = refs.cuda()

    def compat():
        C.initialize_ap()
        boxes = C.get_bboxes_device(pred)
        C.refined_bbox = C.NMS_SAT(boxes)
        C.precision_recall_singleshot(C.refined_bbox, refs)

    out = {"B": B, "H": H, "W": W, "threshold_500": thr500}
    # alternately in one process: ranked, compat, ranked, compat
    for rnd in range(2):
        out["accumulate_500_ms_%d" % rnd], out["accumulate_500_reps"] = timed(lambda: R.accumulate(pred, refs_dev), R.initialize_ap)
        out["compat_500_ms_%d" % rnd], out["compat_500_reps"] = timed(compat)
    R.initialize_ap()
    R.accumulate(pred, refs_dev)
    s = R.summary()
    out["candidates_500"] = [int(c) for c in R._last[2].cpu().tolist()]
    out["survivors_500"] = s["num_P"]
    Rall = harness(Tm.RankedTest, eval_score_threshold=-1.0)
    out["accumulate_all_ms"], out["accumulate_all_reps"] = timed(lambda: Rall.accumulate(pred, refs_dev), Rall.initialize_ap)
    Rall.initialize_ap()
    Rall.accumulate(pred, refs_dev)
    s = Rall.summary()
    out["survivors_all"], out["truncated_all"] = s["num_P"], s["truncated_candidates"]
    for n in (1 << 12, 1 << 17):
        S = harness(Tm.RankedTest)
        acc = S._accumulators(pred.device)
        acc["scores"][:n] = torch.from_numpy(np.round(det.uniform((n,), 5300, 0.5, 1.0) * 1024.0) / 1024.0).cuda()
        acc["tpmask"][:n] = torch.from_numpy((det.uniform((n,), 5301, 0.0, 1.0) * 1024.0).astype(np.int32)).cuda()
        acc["state"][0], acc["state"][1] = n, n // 2

        def summ():
            S._summary = None
            S.summary()
        out["summary_%d_ms" % n], out["summary_%d_reps" % n] = timed(summ)
        out["summary_%d_map" % n] = S.summary()["map"]
    for k in sorted(out):
        print("%-24s %s" % (k, out[k]))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

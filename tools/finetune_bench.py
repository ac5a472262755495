#!/usr/bin/env python3
"""Cost of fine-tuning the camera stream at the cfg2 shapes.

  python tools/finetune_bench.py [--iters 200] [--rounds 5] [--steps 30] [--warmup 10] [--step-rounds 3] [--no-step] [--out FILE]

One process, one GPU.
1. dcf_adamw_ema_step_groups against dcf_adamw_ema_step on fp32 arenas of the cfg2 trainer's flat_params.numel(): blocks of --iters
   launches, HIP events around every launch, the block's median; the variants take turns for --rounds rounds, a variant's figure is
   the median of its blocks' medians (minimum and maximum beside it).  Variants, each without and with decay + average:
       base_a / base_b   dcf_adamw_ema_step twice: the spread between two blocks of the SAME kernel, the margin of every comparison
       unit              the new entry, mu = 1 everywhere (n/4 more bytes)
       slow_trunk        the camera trunk in a 0.1 group
       frozen_trunk      the camera trunk frozen (its elements are not streamed)
2. dcf_image_to_nhwc4_norm against dcf_image_to_nhwc4 at 2 x 3 x 375 x 1242, bf16, the same way.
3. The whole cfg2 train step (Train.one_step_raw, batch 2, bf16, frames resident in HBM, bn_mode eval) for three trainers in this process --
   no groups, stem + layer1 frozen (the rest of the trunk at 0.1), the whole trunk frozen -- alternating for --step-rounds rounds of
   --steps steps, a host clock around steps that end in a device synchronise; and the launches of one step of each from the library's
   profile.
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
LR, B1, B2, EPS, WD = 1e-4, 0.9, 0.999, 1e-8, 0.01
STEM = ["image_backbone.conv1", "image_backbone.bn1"]
GROUPS = {"unfrozen": None,
          "stem_layer1": [{"match": STEM + ["image_backbone.layer1."], "frozen": True}, {"match": ["image_backbone."], "lr_mult": 0.1}],
          "trunk": [{"match": ["image_backbone."], "frozen": True}]}


def _block(fn, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)          # us


def _rounds(variants, iters, rounds):
    series = {name: [] for name, _ in variants}
    for name, fn in variants:
        _block(fn, 20)
    for _ in range(rounds):
        for name, fn in variants:
            series[name].append(_block(fn, iters))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in series.items()}


def optimiser(model, iters, rounds):
    import numpy as np
    import torch
    ops, O = (importlib.import_module(PKG + "." + m) for m in ("ops", "optim"))
    n = model.flat_params.numel()
    entries = model._table.entries
    bits = torch.from_numpy(O.decay_bits(entries, n).view(np.int64)).cuda()
    g = torch.randn(n, device="cuda") * 1e-3
    p, m, v = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    e = p.clone()
    dev = p.device
    slow = O.parse_param_groups([{"match": ["image_backbone."], "lr_mult": 0.1}])
    froz = O.parse_param_groups([{"match": ["image_backbone."], "frozen": True}])
    sides = {"unit": (ops.AdamGroups(O.group_ids(entries, n, None), 1, dev), O.group_table(None, LR, WD)),
             "slow_trunk": (ops.AdamGroups(O.group_ids(entries, n, slow), 2, dev), O.group_table(slow, LR, WD)),
             "frozen_trunk": (ops.AdamGroups(O.group_ids(entries, n, froz), 2, dev), O.group_table(froz, LR, WD))}
    trunk = sum((k[3] + 3) // 4 * 4 for k in entries if k[0].startswith("image_backbone."))
    dm = 1.0 - LR * WD
    out = {"n": n, "trunk_elements": trunk}
    for tag, full in (("plain", False), ("decay_ema", True)):
        def base():
            ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 1, 0.5, dm if full else 1.0, bits if full else None, e if full else None,
                               1e-3 if full else 0.0)

        def new(side):
            gr, tab = sides[side]
            if not full:
                tab = [(mu, 1.0, fz) for mu, _, fz in tab]

            def f():
                ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, EPS, 1, gr, tab, 0.5, bits if full else None, e if full else None,
                                          1e-3 if full else 0.0)
            return f
        res = _rounds([("base_a", base), ("base_b", base)] + [(s, new(s)) for s in sides], iters, rounds)
        a, b = res["base_a"], res["base_b"]
        spread = max(abs(a["median_us"] - b["median_us"]), a["max_us"] - a["min_us"], b["max_us"] - b["min_us"])
        base_us = min(a["median_us"], b["median_us"])
        bpe = 36.0 + 1 / 32 if full else 28.0
        res["spread_us"] = spread
        res["bytes_per_element"] = bpe
        res["allowance_us"] = base_us * (0.25 / bpe) + spread              # n/4 more bytes + the yardstick's own spread
        res["unit_extra_us"] = res["unit"]["median_us"] - base_us
        res["slow_trunk_extra_us"] = res["slow_trunk"]["median_us"] - base_us
        res["frozen_trunk_extra_us"] = res["frozen_trunk"]["median_us"] - base_us
        res["within_allowance"] = {s: res[s]["median_us"] - base_us <= res["allowance_us"] for s in ("unit", "slow_trunk")}
        out[tag] = res
    return out


def image_norm(iters, rounds):
    import torch
    H, ops = (importlib.import_module(PKG + "." + m) for m in ("_hip", "ops"))
    img = torch.randint(0, 256, (2, 3, 375, 1242), dtype=torch.uint8, device="cuda")
    mean, std = H.host_f32([0.406, 0.456, 0.485]), H.host_f32([0.225, 0.224, 0.229])
    y = torch.empty((2, 381, 1250, 4), dtype=torch.bfloat16, device="cuda")

    # an 8 us launch: whatever the host does between the first event and the enqueue is inside the interval while the device waits
    # for it, so both sides hand over ready-made addresses through the bound functions (marshalling two numpy arrays per call
    # showed up as 3 us of "kernel time")
    f_plain, f_norm = H.fn("dcf_image_to_nhwc4"), H.fn("dcf_image_to_nhwc4_norm")
    pi, py, pm, ps, st = img.data_ptr(), y.data_ptr(), mean.ctypes.data, std.ctypes.data, H.stream_ptr()

    def plain():
        f_plain(H.BF16, pi, py, 2, 375, 1242, st)

    def norm():
        f_norm(H.BF16, pi, py, 2, 375, 1242, pm, ps, st)
    res = _rounds([("plain_a", plain), ("plain_b", plain), ("norm", norm)], iters, rounds)
    a, b = res["plain_a"], res["plain_b"]
    res["spread_us"] = max(abs(a["median_us"] - b["median_us"]), a["max_us"] - a["min_us"], b["max_us"] - b["min_us"])
    res["norm_extra_us"] = res["norm"]["median_us"] - min(a["median_us"], b["median_us"])
    res["within_spread"] = res["norm_extra_us"] <= res["spread_us"]
    return res


def steps(bench, cfg, rounds, nsteps, warmup):
    import numpy as np
    import torch
    H, T, FL, det = (importlib.import_module(PKG + "." + m) for m in ("_hip", "train", "frame_loader", "detfill"))
    B = 2
    pool = bench.FramePool(cfg, 4, 100000, 1234)
    trainers = {}
    for side, groups in GROUPS.items():
        c = dict(cfg, bn_mode="eval")
        if groups is not None:
            c["param_groups"] = groups
        trainers[side] = T.Train(c)
        det.fill_state_dict(trainers[side].model)

    def batch(step):
        ids = pool.batch(step, B)
        b = FL.Batch(bboxes=torch.stack([pool.boxes[i] for i in ids], 0), num_bboxes=torch.tensor([pool.nb[i] for i in ids]), crt=None)
        b["points"], b["image"] = [pool.pts[i] for i in ids], pool.image_batch(ids)
        return b

    def run(side, k):
        tr = trainers[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(k):
            tr.one_step_raw(pool.geometry, batch(s))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    np.random.seed(0)
    for side in trainers:
        run(side, warmup)
    series = {side: [] for side in trainers}
    for _ in range(rounds):
        for side in trainers:
            series[side].append(run(side, nsteps))
    launches = {}
    for side in trainers:
        H.call("dcf_prof_reset")
        H.call("dcf_prof_enable", 1)
        try:
            run(side, 1)
        finally:
            H.call("dcf_prof_enable", 0)
        prof = H.prof_read(512)
        H.call("dcf_prof_reset")
        launches[side] = {"total": sum(int(x[1]) for x in prof.values()),
                          "stem_wgrad": sum(int(x[1]) for k, x in prof.items() if k.startswith("stem_wgrad")),
                          "maxpool_bwd": sum(int(x[1]) for k, x in prof.items() if k.startswith("maxpool_bwd"))}
    med = {side: statistics.median(v) for side, v in series.items()}
    spread = max(max(v) - min(v) for v in series.values())
    return {"batch": B, "dtype": cfg["dtype"], "steps_per_round": nsteps, "ms_per_step": series, "median_ms": med, "spread_ms": spread,
            "gain_ms": {side: med["unfrozen"] - med[side] for side in med if side != "unfrozen"},
            "not_slower": {side: med[side] <= med["unfrozen"] + spread for side in med if side != "unfrozen"},
            "launches_per_step": launches, "loss": {side: float(tr.loss_value.item()) for side, tr in trainers.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench.py measures on the GPU; none is visible")
    bench = importlib.import_module("bench")
    M = importlib.import_module(PKG + ".model")
    cfg = bench.kitti_config(2)
    out = {"device": torch.cuda.get_device_name(0), "optimiser": optimiser(M.ObjectDetection_DCF(cfg), args.iters, args.rounds),
           "image_norm": image_norm(args.iters, args.rounds)}
    torch.cuda.empty_cache()
    if not args.no_step:
        out["step"] = steps(bench, cfg, args.step_rounds, args.steps, args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

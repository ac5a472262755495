#!/usr/bin/env python3
"""Cost of gradient accumulation (csrc/optim.hip dcf_grad_accumulate) at the cfg2 arena size.

  python tools/accum_bench.py [--iters 200] [--rounds 5] [--step] [--steps 40] [--warmup 8] [--out FILE]

One process, one GPU.  Kernel timings: on fp32 arenas of the cfg2 trainer's flat_params.numel() (96 MB each), blocks of --iters
launches, HIP events around every launch, the block's median; the variants take turns for --rounds rounds, and a variant's figure
is the median of its blocks' medians (minimum and maximum beside it):
    adam_a / adam_b          dcf_adam_step twice (28 B per element): the project's yardstick for a streaming pass, and the spread
                             between two blocks of the SAME kernel, the margin of every comparison
    copy                     dcf_grad_accumulate mode 0, dst = src (8 B per element)
    add                      dcf_grad_accumulate mode 1, dst += src (12 B per element)
    add_range                mode 1 on a range that starts 4 bytes past a 16-byte boundary in both arenas (the scalar head + float4 body)
    add_scalar               mode 1 with dst and src 4 bytes apart modulo 16 (the one-float-per-lane path no trainer call takes)
--step: the whole cfg2 train step (bench.py's frames resident in HBM, batch 2, bf16) with grad_accum_steps 2 and 4 against the
plain step, three trainers in this process taking turns for --rounds rounds of --steps one_step calls (a multiple of 4: whole
windows), a host clock around calls that end in a device synchronise: mean time per micro-step.  Prints one JSON line (and writes
it to --out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8


def _block(fn, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)          # us


def kernels(n, iters, rounds):
    import torch
    ops = importlib.import_module(PKG + ".ops")
    g = torch.randn(n + 8, device="cuda") * 1e-3
    acc = torch.zeros(n + 8, device="cuda")
    p, m, v = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")

    def adam():
        ops.adam_step(p, g[:n], m, v, LR, B1, B2, EPS, 1, 0.5)

    def accumulate(mode, doff, soff):
        dst, src = acc[doff:doff + n], g[soff:soff + n]

        def f():
            ops.grad_accumulate(dst, src, mode)
        return f

    variants = [("adam_a", adam, 28.0), ("adam_b", adam, 28.0), ("copy", accumulate(0, 0, 0), 8.0), ("add", accumulate(1, 0, 0), 12.0),
                ("add_range", accumulate(1, 1, 1), 12.0), ("add_scalar", accumulate(1, 0, 1), 12.0)]
    series = {name: [] for name, _, _ in variants}
    for name, fn, _ in variants:                             # warm-up: every variant once
        _block(fn, 20)
    for _ in range(rounds):
        for name, fn, _ in variants:
            series[name].append(_block(fn, iters))
    res = {}
    for name, _, bpe in variants:
        med = statistics.median(series[name])
        res[name] = {"median_us": med, "min_us": min(series[name]), "max_us": max(series[name]), "bytes_per_element": bpe,
                     "tbytes_per_s": n * bpe / med / 1e6}
    a, b = res["adam_a"], res["adam_b"]
    spread = max(abs(a["median_us"] - b["median_us"]), a["max_us"] - a["min_us"], b["max_us"] - b["min_us"])
    adam_bw = max(a["tbytes_per_s"], b["tbytes_per_s"])
    return {"n": n, "iters": iters, "rounds": rounds, "variants": res, "spread_us": spread, "adam_tbytes_per_s": adam_bw,
            "relative_to_adam": {k: res[k]["tbytes_per_s"] / adam_bw for k in ("copy", "add", "add_range", "add_scalar")}}


def steps(bench, cfg, rounds, nsteps, warmup):
    import numpy as np
    import torch
    T, det = importlib.import_module(PKG + ".train"), importlib.import_module(PKG + ".detfill")
    pool = bench.FramePool(cfg, 4, 100000, 1000)
    trainers = {}
    for side, k in (("plain", 1), ("k2", 2), ("k4", 4)):
        c = dict(cfg)
        if k > 1:
            c["grad_accum_steps"] = k
        trainers[side] = T.Train(c)
        det.fill_state_dict(trainers[side].model)

    def run(side, count):
        tr = trainers[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(count):
            bench.train_step(tr, pool, pool.batch(s, 2))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / count

    np.random.seed(0)
    for side in trainers:
        run(side, warmup)
    series = {side: [] for side in trainers}
    for _ in range(rounds):
        for side in trainers:
            series[side].append(run(side, nsteps))
    med = {side: statistics.median(v) for side, v in series.items()}
    spread = {side: max(v) - min(v) for side, v in series.items()}
    return {"batch": 2, "dtype": cfg["dtype"], "micro_steps_per_round": nsteps, "ms_per_micro_step": series, "median_ms": med,
            "spread_ms": spread, "cost_ms": {side: med[side] - med["plain"] for side in ("k2", "k4")},
            "open_window": {side: tr.accum_index() for side, tr in trainers.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps % 4 or args.warmup % 4:
        raise SystemExit("--steps and --warmup must be multiples of 4 (whole windows of 2 and of 4)")
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench.py measures on the GPU; none is visible")
    bench = importlib.import_module("bench")
    M = importlib.import_module(PKG + ".model")
    cfg = bench.kitti_config(2)
    n = M.ObjectDetection_DCF(cfg).flat_params.numel()
    out = {"kernels": kernels(n, args.iters, args.rounds)}
    torch.cuda.empty_cache()
    if args.step:
        out["step"] = steps(bench, cfg, args.rounds, args.steps, args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the training recipe's optimiser step (csrc/optim.hip) at the cfg2 arena size.

  python tools/optim_bench.py [--iters 200] [--rounds 5] [--step] [--steps 40] [--warmup 10] [--out FILE]

One process, one GPU.  Kernel timings: on fp32 arenas of the cfg2 trainer's flat_params.numel() (five arenas of 96 MB: nothing
stays in the 256 MB Infinity Cache from one launch to the next), blocks of --iters launches, HIP events around every launch,
the block's median; the variants take turns for --rounds rounds, and a variant's figure is the median of its blocks' medians
(minimum and maximum beside it):
    adam_a / adam_b          dcf_adam_step twice: the spread between two blocks of the SAME kernel, the margin of every comparison
    <shape>/off              dcf_adamw_ema_step with decay_mul 1, no mask, no average (28 B per element)
    <shape>/decay            decoupled decay under the cfg2 model's real mask (28 B + 1/32 B per element)
    <shape>/decay_ema        decay and the weight average (36 B per element)
    adam_guarded             dcf_adam_step_guarded with a clean state
    adam_skew, flat/decay_ema_skew    the same launches on arenas that start 4352 bytes further into their allocation each (torch
                             hands out the five 96 MB arenas at the same offset within the memory channels' interleave; the
                             skew tells whether the streams of one wave meeting on one channel costs anything)
    <shape>/guarded_off, <shape>/guarded_decay_ema      the new entry with that state
for both launch shapes (option ADAMW_SHAPE: flat = one float4 group per lane; stride = capped grid, grid-stride, two groups in
flight per lane).  --step: the whole cfg2 train step (bench.py's frames resident in HBM, batch 2, bf16) with the recipe on
(cosine schedule + weight_decay + ema_decay) against off, two trainers in this process alternating for --rounds rounds of --steps
steps, a host clock around steps that end in a device synchronise.  Prints one JSON line (and writes it to --out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
SHAPES = ("flat", "stride")
RECIPE = dict(lr_schedule=dict(kind="cosine", warmup_steps=100, total_steps=100000, min_lr=1e-6), weight_decay=0.01, ema_decay=0.999)
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


def kernels(model, iters, rounds):
    import numpy as np
    import torch
    H, ops, O = (importlib.import_module(PKG + "." + m) for m in ("_hip", "ops", "optim"))
    n = model.flat_params.numel()
    words = O.decay_bits(model._table.entries, n)
    bits = torch.from_numpy(words.view(np.int64)).cuda()
    g = torch.randn(n, device="cuda") * 1e-3
    p, m, v = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    e = p.clone()
    st = ops.AmpState(g.device, 1.0)
    ops.grad_stats(g, st)
    ops.amp_update(st, 0.5, False, 2.0, 0.5, 2000, None, LR, B1, B2)
    assert int(st.found_inf.item()) == 0
    dm = 1.0 - LR * 0.01
    SKEW = 1088                                             # floats: 4352 bytes = 17 x 256, a multiple of 16
    ps, gs, ms, vs, es = (torch.empty(n + 5 * SKEW, device="cuda")[k * SKEW:k * SKEW + n].copy_(t) for k, t in enumerate((p, g, m, v, e)))

    def adam():
        ops.adam_step(p, g, m, v, LR, B1, B2, EPS, 1, 0.5)

    def adam_skew():
        ops.adam_step(ps, gs, ms, vs, LR, B1, B2, EPS, 1, 0.5)

    def ema_skew():
        ops.adamw_ema_step(ps, gs, ms, vs, LR, B1, B2, EPS, 1, 0.5, dm, bits, es, 1e-3)

    def adam_guarded():
        ops.adam_step_guarded(p, g, m, v, B1, B2, EPS, st)

    def new(decay, ema, state):
        def f():
            ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 1, 0.5, dm if decay else 1.0, bits if decay else None, e if ema else None,
                               1e-3 if ema else 0.0, state)
        return f

    variants = [("adam_a", None, adam, 28.0), ("adam_b", None, adam, 28.0), ("adam_guarded", None, adam_guarded, 28.0),
                ("adam_skew", None, adam_skew, 28.0), ("flat/decay_ema_skew", "flat", ema_skew, 36.0 + 1 / 32)]
    for s in SHAPES:
        variants += [(s + "/off", s, new(False, False, None), 28.0), (s + "/decay", s, new(True, False, None), 28.0 + 1 / 32),
                     (s + "/decay_ema", s, new(True, True, None), 36.0 + 1 / 32), (s + "/guarded_off", s, new(False, False, st), 28.0),
                     (s + "/guarded_decay_ema", s, new(True, True, st), 36.0 + 1 / 32)]
    series = {name: [] for name, _, _, _ in variants}
    try:
        for name, shape, fn, _ in variants:                  # warm-up: every variant once
            H.set_option("ADAMW_SHAPE", shape)
            _block(fn, 20)
        for _ in range(rounds):
            for name, shape, fn, _ in variants:
                H.set_option("ADAMW_SHAPE", shape)
                series[name].append(_block(fn, iters))
    finally:
        H.set_option("ADAMW_SHAPE", None)
    res = {}
    for name, _, _, bpe in variants:
        med = statistics.median(series[name])
        res[name] = {"median_us": med, "min_us": min(series[name]), "max_us": max(series[name]), "bytes_per_element": bpe,
                     "tbytes_per_s": n * bpe / med / 1e6}
    a, b = res["adam_a"]["median_us"], res["adam_b"]["median_us"]
    spread = max(abs(a - b), res["adam_a"]["max_us"] - res["adam_a"]["min_us"], res["adam_b"]["max_us"] - res["adam_b"]["min_us"])
    adam_us, adam_bw = min(a, b), max(res["adam_a"]["tbytes_per_s"], res["adam_b"]["tbytes_per_s"])
    checks = {}
    for s in SHAPES:
        d, de = res[s + "/decay"], res[s + "/decay_ema"]
        checks[s] = {"decay_no_slower_than_adam": d["median_us"] <= max(a, b) + spread,
                     "decay_ema_reaches_adam_bandwidth": n * de["bytes_per_element"] / (de["median_us"] - spread) / 1e6 >= min(res["adam_a"]["tbytes_per_s"], res["adam_b"]["tbytes_per_s"])}
    return {"n": n, "mask_words": int(len(words)), "decayed_groups": int(sum(bin(int(w)).count("1") for w in words)), "iters": iters,
            "rounds": rounds, "variants": res, "spread_us": spread, "adam_us": adam_us, "adam_tbytes_per_s": adam_bw, "expectations": checks}


def steps(bench, cfg, rounds, nsteps, warmup):
    import numpy as np
    import torch
    T, det = importlib.import_module(PKG + ".train"), importlib.import_module(PKG + ".detfill")
    pool = bench.FramePool(cfg, 4, 100000, 1000)
    trainers = {}
    for side, over in (("off", {}), ("on", RECIPE)):
        c = dict(cfg)
        c.update(over)
        trainers[side] = T.Train(c)
        det.fill_state_dict(trainers[side].model)

    def run(side, k):
        tr = trainers[side]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(k):
            bench.train_step(tr, pool, pool.batch(s, 2))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    np.random.seed(0)
    for side in trainers:
        run(side, warmup)
    series = {side: [] for side in trainers}
    for _ in range(rounds):
        for side in trainers:
            series[side].append(run(side, nsteps))
    med = {side: statistics.median(v) for side, v in series.items()}
    return {"batch": 2, "dtype": cfg["dtype"], "steps_per_round": nsteps, "recipe": RECIPE, "ms_per_step": series, "median_ms": med,
            "recipe_cost_ms": med["on"] - med["off"], "derived_ms": 0.04,
            "loss": {side: float(tr.loss_value.item()) for side, tr in trainers.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py measures on the GPU; none is visible")
    bench = importlib.import_module("bench")
    M = importlib.import_module(PKG + ".model")
    cfg = bench.kitti_config(2)
    out = {"kernels": kernels(M.ObjectDetection_DCF(cfg), args.iters, args.rounds)}
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

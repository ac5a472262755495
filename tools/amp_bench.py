#!/usr/bin/env python3
"""Cost of the guarded optimiser step (csrc/amp.hip) at the cfg2 arena size.

  python tools/amp_bench.py --parent-lib PATH [--iters 300] [--rounds 3] [--step]

Times, with HIP events after a warm-up, the three guarded launches (dcf_grad_stats + dcf_amp_update + dcf_adam_step_guarded, one
bracket, and each on its own) on an fp32 arena of the cfg2 model's size, against dcf_adam_step of PATH -- the library built from
another tree (the parent commit), loaded with DCF_HIP_LIB -- on the same arena in the same job.  Each side runs in a fresh child
process; the children alternate for --rounds rounds and each reports the median of --iters launches.  --step: also the whole cfg2
train step (bench.py's frames, batch 2, bf16) with loss_scale dynamic against none, as information."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"


def _arena_size():
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    model = importlib.import_module(PKG + ".model")
    return model.ObjectDetection_DCF(bench.kitti_config(2)).flat_params.numel()


def _events(fn, iters, warmup=50):
    import torch
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)          # us


def child(side, n, iters):
    import torch
    sys.path.insert(0, ROOT)
    import importlib
    H = importlib.import_module(PKG + "._hip")
    g = torch.randn(n, device="cuda") * 1e-3
    p, m, v = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    if side == "plain":
        # the other tree's library exports only its own entry points: bind dcf_adam_step alone, not the whole binding table
        import ctypes
        L = ctypes.CDLL(H.LIB_PATH)
        L.dcf_adam_step.restype, L.dcf_adam_step.argtypes = H.SIGNATURES["dcf_adam_step"]
        out = {"side": side, "n": n, "lib": H.LIB_PATH, "version": L.dcf_version()}

        def adam():
            rc = L.dcf_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-4, 0.9, 0.999, 1e-8, 1, 0.5, H.stream_ptr())
            assert rc == 0
        out["adam_us"] = _events(adam, iters)
        print("RESULT " + json.dumps(out), flush=True)
        return
    out = {"side": side, "n": n, "lib": H.LIB_PATH, "version": H.lib().dcf_version()}
    ops =importlib.import_module(PKG + ".ops")
    st = ops.AmpState(g.device, 2.0)

    def stats():
        ops.grad_stats(g, st)

    def update():
        ops.amp_update(st, 1.0, True, 2.0, 0.5, 2000, 1e6, 1e-4, 0.9, 0.999)

    def adam():
        ops.adam_step_guarded(p, g, m, v, 0.9, 0.999, 1e-8, st)

    def guarded():
        stats()
        update()
        adam()
    out["guarded_us"] = _events(guarded, iters)
    out["grad_stats_us"] = _events(stats, iters)
    out["amp_update_us"] = _events(update, iters)
    out["adam_guarded_us"] = _events(adam, iters)
    assert int(st.found_inf.item()) == 0
    print("RESULT " + json.dumps(out), flush=True)


def step_child(mode, steps, warmup):
    import time
    import torch
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    T, det = importlib.import_module(PKG + ".train"), importlib.import_module(PKG + ".detfill")
    cfg = bench.kitti_config(2)
    if mode == "dynamic":
        cfg["loss_scale"] = "dynamic"
    tr = T.Train(cfg)
    det.fill_state_dict(tr.model)
    pool = bench.FramePool(cfg, 4, 100000, 1000)
    for s in range(warmup):
        bench.train_step(tr, pool, pool.batch(s, 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        bench.train_step(tr, pool, pool.batch(s, 2))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {"mode": mode, "step_ms": ms}
    if mode == "dynamic":
        out["skipped"] = int(tr.skipped_steps().item())
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, env=None, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=env, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit("child %s failed (%d):\n%s\n%s" % (args, p.returncode, p.stdout[-2000:], p.stderr[-3000:]))
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libdcf_hip.so built from the tree to compare against")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--child", choices=["plain", "guarded"])
    ap.add_argument("--step-child", choices=["none", "dynamic"])
    ap.add_argument("--n", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, a.iters)
    if a.step_child:
        return step_child(a.step_child, a.steps, 10)
    n = _arena_size()
    print("arena: %d fp32 elements (cfg2 model, flat_params)" % n)
    res = {"plain": [], "guarded": []}
    if a.parent_lib:
        penv = dict(os.environ, DCF_HIP_LIB=os.path.abspath(a.parent_lib))
    for r in range(a.rounds):
        if a.parent_lib:
            res["plain"].append(run_child(["--child", "plain", "--n", str(n), "--iters", str(a.iters)], env=penv))
        res["guarded"].append(run_child(["--child", "guarded", "--n", str(n), "--iters", str(a.iters)]))
    print("median of %d launches per child, %d rounds alternating (us):" % (a.iters, a.rounds))
    for r in range(a.rounds):
        g = res["guarded"][r]
        line = "  round %d: guarded %.1f (grad_stats %.1f + amp_update %.1f + adam_guarded %.1f)" % (
            r, g["guarded_us"], g["grad_stats_us"], g["amp_update_us"], g["adam_guarded_us"])
        if res["plain"]:
            line += " | parent dcf_adam_step %.1f (lib version %d)" % (res["plain"][r]["adam_us"], res["plain"][r]["version"])
        print(line)
    gm = statistics.median(x["guarded_us"] for x in res["guarded"])
    summary = {"n": n, "guarded_us": gm, "grad_stats_us": statistics.median(x["grad_stats_us"] for x in res["guarded"]),
               "amp_update_us": statistics.median(x["amp_update_us"] for x in res["guarded"]),
               "adam_guarded_us": statistics.median(x["adam_guarded_us"] for x in res["guarded"])}
    if res["plain"]:
        pm = statistics.median(x["adam_us"] for x in res["plain"])
        summary.update(parent_adam_us=pm, ratio=gm / pm)
        print("guarded / parent Adam: %.1f / %.1f us = %.3fx (gate 1.35x)" % (gm, pm, gm / pm))
    if a.step:
        st = {"none": [], "dynamic": []}
        for r in range(a.rounds):
            for mode in ("none", "dynamic"):
                st[mode].append(run_child(["--step-child", mode, "--steps", str(a.steps)], timeout=900)["step_ms"])
        for mode in ("none", "dynamic"):
            print("cfg2 step (batch 2, bf16), loss_scale %-7s: %s ms" % (mode, " ".join("%.3f" % x for x in st[mode])))
        sn, sd = statistics.median(st["none"]), statistics.median(st["dynamic"])
        summary.update(step_none_ms=sn, step_dynamic_ms=sd, step_delta_pct=100.0 * (sd - sn) / sn)
        print("whole step: dynamic vs none %+.2f %% (information, not a gate)" % summary["step_delta_pct"])
    print("SUMMARY " + json.dumps(summary))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Grouped launches of independent convolutions (dcf_conv2d_fwd_group / dcf_conv2d_dgrad_group) against the same layers back to
back in launches of their own (option IGEMM_GROUP=0), at the cfg2 sites.
Usage (GPU box): python tools/conv_group_bench.py [--dtype bf16] [--batch 2]"""
import argparse, ctypes, importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd"
H = importlib.import_module(PKG + "._hip")

# site -> (kind, [(H, W, Cin, Cout, k, stride)]); H x W = the size of x (fwd) / of gx (dgrad)
SITES = [("lidar head 2", "fwd", [(704, 800, 32, 64, 3, 2), (704, 800, 32, 64, 1, 2)]),
         ("lidar head 3", "fwd", [(352, 400, 64, 128, 3, 2), (352, 400, 64, 128, 1, 2)]),
         ("lidar head 4", "fwd", [(176, 200, 128, 192, 3, 2), (176, 200, 128, 192, 1, 2)]),
         ("lidar head 5", "fwd", [(88, 100, 192, 256, 3, 2), (88, 100, 192, 256, 1, 2)]),
         ("camera head 2", "fwd", [(94, 311, 64, 128, 3, 2), (94, 311, 64, 128, 1, 2)]),
         ("camera head 3", "fwd", [(47, 156, 128, 256, 3, 2), (47, 156, 128, 256, 1, 2)]),
         ("camera head 4", "fwd", [(24, 78, 256, 512, 3, 2), (24, 78, 256, 512, 1, 2)]),
         ("lidar FPN", "fwd", [(88, 100, 192, 192, 1, 1), (44, 50, 256, 192, 1, 1), (176, 200, 128, 192, 1, 1)]),
         ("camera FPN", "fwd", [(12, 39, 512, 64, 1, 1), (24, 78, 256, 64, 1, 1), (47, 156, 128, 64, 1, 1), (94, 311, 64, 64, 1, 1)]),
         ("fc1_feat (34 k rows)", "fwd", [(34048, 1, 64, c, 1, 1) for c in (64, 128, 192, 256)]),
         ("lidar FPN bwd", "dgrad", [(176, 200, 128, 192, 1, 1), (88, 100, 192, 192, 1, 1), (44, 50, 256, 192, 1, 1)]),
         ("camera FPN bwd", "dgrad", [(94, 311, 64, 64, 1, 1), (47, 156, 128, 64, 1, 1), (24, 78, 256, 64, 1, 1), (12, 39, 512, 64, 1, 1)])]


def timeit(fn, iters=50):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=2)
    args = ap.parse_args()
    dt = H.dtype_code(args.dtype)
    td, B = H.torch_dtype(dt), args.batch
    rnd = lambda shape, s=1.0: ((torch.rand(shape, device="cuda") - 0.5) * s).to(td)
    print("%-22s %3s | single us | grouped us | launches" % ("site", "n"))
    for name, kind, layers in SITES:
        n = len(layers)
        keep, items = [], (H.ConvFwdItem * n)() if kind == "fwd" else (H.ConvDgradItem * n)()
        for i, (Hh, W, Ci, Co, k, s) in enumerate(layers):
            pad = k // 2
            Ho, Wo = (Hh + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
            if kind == "fwd":
                x, w, y = rnd((B, Hh, W, Ci)), rnd((Co, k, k, Ci), 0.1), torch.empty((B, Ho, Wo, Co), device="cuda", dtype=td)
                items[i] = H.ConvFwdItem(dt, 0, x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), B, Hh, W, Ci, Ho, Wo, Co, k, k, s, pad, 0)
            else:
                x, w, y = rnd((B, Ho, Wo, Co)), rnd((Ci, k, k, Co), 0.1), torch.empty((B, Hh, W, Ci), device="cuda", dtype=td)
                items[i] = H.ConvDgradItem(dt, 0, x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), B, Hh, W, Ci, Ho, Wo, Co, k, k, s, pad, 0)
            keep.append((x, w, y))
        entry = "dcf_conv2d_fwd_group" if kind == "fwd" else "dcf_conv2d_dgrad_group"
        st = H.stream_ptr()
        run = lambda: H.call(entry, ctypes.addressof(items), n, st)
        H.set_option("IGEMM_GROUP", 0)
        t0 = timeit(run)
        H.set_option("IGEMM_GROUP", None)
        t1 = timeit(run)
        H.call("dcf_prof_reset"); H.call("dcf_prof_enable", 1)
        run(); torch.cuda.synchronize()
        H.call("dcf_prof_enable", 0)
        names = ", ".join("%s x%d" % (k_, v[1]) for k_, v in sorted(H.prof_read().items()))
        H.call("dcf_prof_reset")
        print("%-22s %3d | %9.1f | %10.1f | %s" % (name, n, t0, t1, names))


if __name__ == "__main__":
    main()

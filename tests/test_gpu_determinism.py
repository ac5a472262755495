"""`deterministic: true` on the GPU: the canonical inverse maps integer for integer, the fixed-order
kernels against the default (atomic) kernels within the tolerances the default kernels' own tests use, bitwise repeatability of
every new kernel and of the whole train step while a second stream hogs the memory system, checkpoint resume with fusion on.
No test here asserts that the DEFAULT mode differs from run to run."""
import os

import numpy as np
import pytest
import torch

from _fusion_ref import _sorted_pairs, cam_map_statement, fusion_bwd_statement, tap_weights, taps_statement   # noqa: F401
from _util import pkg

pytestmark = pytest.mark.gpu

AFF = (10.0, 0.0, 10.0, 400.0)


class Hog(object):
    """The bandwidth hog of tests/stress_child.py: a second stream of this process moves 512 MB back and forth."""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.a = torch.empty(128 << 20, dtype=torch.float32, device="cuda")
        self.b = torch.empty_like(self.a)

    def kick(self, rounds=2):
        with torch.cuda.stream(self.stream):
            for _ in range(rounds):
                self.b.copy_(self.a, non_blocking=True)
                self.a.copy_(self.b, non_blocking=True)


def _knn_case(case, K, h, w, stride, n_max, seed=7):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(seed)
    n = {"random": 200, "one_point": 1, "no_points": 0, "few": 8}[case]
    xyz = torch.zeros(n_max, 3)
    xyz[:n, 0] = torch.rand(n, generator=g) * (h * stride / AFF[0])
    xyz[:n, 1] = torch.rand(n, generator=g) * (w * stride / AFF[2]) - AFF[3] / AFF[2]
    xyz[:n, 2] = torch.rand(n, generator=g) * 2 - 1
    xyz = xyz.cuda()
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    idx = ops.knn_bev(xyz, cnt, K, h, w, stride, AFF)
    return xyz, cnt, idx, n, g


def _uv_case(B, n_max, Hf, Wf, seed, crowd=False):
    g = torch.Generator().manual_seed(seed)
    uv = torch.rand(B, n_max, 2, generator=g)
    uv[..., 0] = uv[..., 0] * (Wf * 4 + 8) - 4                # a few points beyond every border: the clamp folds taps
    uv[..., 1] = uv[..., 1] * (Hf * 4 + 8) - 4
    if crowd:                                                  # many points inside one camera pixel: a list longer than a wave
        uv[0, :150, 0] = 41.0 + torch.rand(150, generator=g)
        uv[0, :150, 1] = 21.0 + torch.rand(150, generator=g)
    cnt = torch.tensor([n_max - 7 * b for b in range(B)], dtype=torch.int32)
    return uv, cnt


# ------------------------------------------------------------------------------------------------ 1. canonical maps, exact
@pytest.mark.parametrize("K,h,w,case", [(3, 24, 40, "random"), (5, 24, 40, "random"), (1, 24, 40, "random"), (3, 24, 40, "one_point"),
                                        (3, 24, 40, "no_points"), (1, 80, 64, "one_point"), (1, 96, 64, "few")])
def test_canonical_inverse_maps_exact(K, h, w, case):
    """dcf_fusion_invert + dcf_inv_sort_segments: start as the unsorted call leaves it, every segment of ent_pix / ent_pt equal to a
    numpy sort of the KNN map.  (1, 80, 64, one_point): one segment of 5120 pairs (beyond the LDS path); (1, 96, 64, few): segments of
    some hundred to a few thousand pairs (the LDS path); random: the in-wave path."""
    ops = pkg("ops")
    n_max = 300
    xyz, cnt, idx, n, _ = _knn_case(case, K, h, w, 4, n_max)
    idx2 = torch.flip(idx, dims=[1]).contiguous()              # a second map in the same call: segments of two maps side by side
    parent = ops.fusion_invert([idx, idx2], n_max)
    start0 = parent[0].clone()
    start, ent = ops.fusion_invert_sorted([idx, idx2], n_max)
    assert torch.equal(start, start0)
    st, px, pt = start.cpu().numpy(), ent[0].cpu().numpy(), ent[1].cpu().numpy()
    longest, off, lds_path = 0, 0, 0
    for m, t in enumerate((idx, idx2)):
        ws, wpx, wpt = _sorted_pairs(t.cpu().numpy(), n_max)
        seg = st[m * (n_max + 1):(m + 1) * (n_max + 1)]
        assert np.array_equal(seg - off, ws)
        assert np.array_equal(px[off:off + len(wpx)], wpx) and np.array_equal(pt[off:off + len(wpt)], wpt)
        lens = np.diff(np.append(ws, len(wpx)))
        longest = max(longest, int(lens.max()))
        lds_path += int(((lens > 64) & (lens <= 4096)).sum())
        off += len(wpx)
    if (K, h, w, case) == (1, 80, 64, "one_point"):
        assert longest > 4096
    if case == "few":
        assert lds_path >= 2


@pytest.mark.parametrize("B,n_max,Hf,Wf,crowd", [(1, 300, 24, 32, False), (2, 1000, 24, 32, True), (1, 0, 8, 8, False)])
def test_camera_pixel_map_exact(B, n_max, Hf, Wf, crowd):
    ops = pkg("ops")
    uv, cnt = _uv_case(B, max(n_max, 1), Hf, Wf, 11, crowd and n_max >= 150)
    if n_max == 0:
        cnt = torch.zeros(B, dtype=torch.int32)
    start, ent, _ = ops.cam_invert(uv.cuda(), cnt.cuda(), n_max, Hf, Wf)
    ws, we = cam_map_statement(uv.numpy(), cnt.numpy(), n_max, Hf, Wf)
    assert np.array_equal(start.cpu().numpy(), ws)
    assert np.array_equal(ent.cpu().numpy()[:len(we)], we)
    if crowd:
        assert int(np.diff(ws).max()) > 64


# ------------------------------------------------------------------------------------------------ 2. kernel parity
@pytest.mark.parametrize("Cb,K,case", [(64, 3, "random"), (128, 5, "random"), (192, 1, "random"), (256, 3, "random"), (256, 1, "random"),
                                       (64, 5, "random"), (64, 3, "one_point"), (128, 3, "no_points")])
def test_fusion_backward_det_matches_pixel_run_kernel(Cb, K, case):
    """The harness of tests/test_gpu_fusion.py::test_fusion_backward_by_point_matches_pixel_run_kernel with the deterministic kernel
    in the place of the by-point ones: dP (compute dtype, buffer starts as NaN), dW1d, db1 against dcf_fusion_gather_bwd; same
    tolerances.  The pixel-run kernel used as the reference here is itself pinned to the fp64 statement in tests/test_gpu_fusion_edges.py."""
    ops, H = pkg("ops"), pkg("_hip")
    h, w, stride, n_max = 24, 40, 4, 300
    xyz, cnt, idx, n, g = _knn_case(case, K, h, w, stride, n_max)
    assert int((idx >= 0).sum()) == (min(K, n) * h * w)
    P = (torch.rand(n_max, Cb, generator=g) - 0.5).cuda()
    ghs = (torch.rand(h, w, Cb, generator=g) - 0.5).cuda()
    w1d = ((torch.rand(Cb, 3, generator=g) - 0.5) * 0.2).cuda().reshape(-1)
    b1 = ((torch.rand(Cb, generator=g) - 0.5) * 0.2).cuda()
    inv = ops.fusion_invert_sorted([idx], n_max)
    ws = ops.fusion_bwd_det_workspace("cuda", K * h * w, Cb, 1)
    ws.fill_(float("nan"))
    for dtype, tol in ((H.F32, 2e-5), (H.BF16, 2e-5)):
        Pd = P.to(H.torch_dtype(dtype))
        gd = ghs.to(H.torch_dtype(dtype))
        ref = [torch.zeros(n_max, Cb, device="cuda"), torch.zeros(Cb * 3, device="cuda"), torch.zeros(Cb, device="cuda")]
        ops.fusion_gather_bwd(dtype, Pd, xyz, idx, stride, AFF, w1d, b1, gd, *ref)
        for rows in (n_max, 256):
            gp = torch.full((1, rows, Cb), float("nan"), device="cuda").to(H.torch_dtype(dtype))
            gw, gb = torch.zeros(Cb * 3, device="cuda"), torch.zeros(Cb, device="cuda")
            ops.fusion_gather_bwd_det(dtype, Pd[:rows].contiguous().unsqueeze(0), xyz.unsqueeze(0), inv, n_max, 0, (K, h, w), stride, AFF, w1d, b1,
                                      gd.unsqueeze(0), gp, gw, gb, ws)
            gp = gp[0]
            want = ref[0][:rows].to(H.torch_dtype(dtype)).float() if dtype != H.F32 else ref[0][:rows]
            assert torch.isfinite(gp.float()).all()
            rtol = tol if dtype == H.F32 else 2.0 ** -7
            err = float((gp.float() - want).abs().max())
            print("Cb %d K %d %s dtype %d rows %d: dP err %.3g of %.3g" % (Cb, K, case, dtype, rows, err, float(want.abs().max())))
            assert err <= rtol * max(float(want.abs().max()), 1e-6) * max(1.0, (h * w) ** 0.5 if dtype == H.F32 else 1.0)
            for a, b in ((gw, ref[1]), (gb, ref[2])):
                scale = max(float(b.abs().max()), 1e-6)
                assert float((a - b).abs().max()) <= tol * scale * max(1.0, (h * w) ** 0.5)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("K", [3, 5])
def test_fusion_backward_det_at_cfg2_size(K, dtype):
    """tests/test_gpu_benchsize.py::test_fusion_backward_by_point_at_cfg2_size's harness (its cloud, its fp64 statement with the
    slack for ambiguous ReLU decisions, its tolerances) around the deterministic kernel, all four sites."""
    from test_gpu_benchsize import _cfg2_frame
    ops, H = pkg("ops"), pkg("_hip")
    g, pc, uv, n = _cfg2_frame()
    n_max = pc.shape[0]
    xyz = torch.from_numpy(pc)
    xyz_d = xyz.cuda()
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    sites = [(2, 64), (4, 128), (8, 192), (16, 256)]
    maps = [ops.knn_bev(xyz_d, cnt, K, 704 // s, 800 // s, s, g.aff) for s, _ in sites]
    inv = ops.fusion_invert_sorted(maps, n_max)
    rows = (n + 255) // 256 * 256
    code = H.dtype_code(dtype)
    tdt = H.torch_dtype(code)
    gen = torch.Generator().manual_seed(100 + K)
    for si, (stride, Cb) in enumerate(sites):
        h, w = 704 // stride, 800 // stride
        idx = maps[si].cpu()
        P = (torch.rand(rows, Cb, generator=gen) - 0.5).to(tdt)
        ghs = (torch.rand(h, w, Cb, generator=gen) - 0.5).to(tdt)
        w1d = (torch.rand(Cb, 3, generator=gen) - 0.5) * 0.2
        b1 = (torch.rand(Cb, generator=gen) - 0.5) * 0.2
        gp = torch.full((1, rows, Cb), float("nan"), device="cuda").to(tdt)
        got = [gp, torch.zeros(Cb * 3, device="cuda"), torch.zeros(Cb, device="cuda")]
        ws = ops.fusion_bwd_det_workspace("cuda", K * h * w, Cb, 1)
        ops.fusion_gather_bwd_det(code, P.cuda().unsqueeze(0), xyz_d.unsqueeze(0), inv, n_max, si, (K, h, w), stride, g.aff, w1d.reshape(-1).cuda(),
                                  b1.cuda(), ghs.cuda().unsqueeze(0), *got, ws)
        want, slack = fusion_bwd_statement(P.float(), xyz, idx, stride, g.aff, w1d, b1, ghs.float())
        assert torch.isfinite(gp.float()).all()
        got = [got[0][0].float().cpu().double(), got[1].cpu().double().view(Cb, 3), got[2].cpu().double()]
        # dP comes out in the compute dtype here (the default kernel's accumulator is fp32): 2^-7 on bf16 rows, as the small-shape test has it
        for name, a, b, s_, tol in (("dP", got[0], want[0], slack[0], 2e-5 if dtype == "f32" else 2.0 ** -7), ("dW1d", got[1], want[1], slack[1], 3e-4), ("db1", got[2], want[2], slack[2], 3e-4)):
            scale = float(b.abs().max())
            assert scale > 0
            over = (a - b).abs() - (tol * scale + 1.01 * s_)
            print("site %d K %d %s %s: off by %.3g of max %.3g" % (si, K, dtype, name, float((a - b).abs().max()), scale))
            assert float(over.max()) <= 0, "site %d (stride %d, Cb %d, K %d, %s) %s: off by %g of max %g" % (
                si, stride, Cb, K, dtype, name, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("Cf", [64, 256])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_point_sample_backward_det_matches_atomic_kernel(Cf, dtype):
    """Small maps, two frames, borders and a crowded pixel: every row stored (buffer starts as NaN), 2e-5 of the maximum against
    dcf_point_sample_bwd_batch (the bound of test_point_sample_backward_at_cfg2_size)."""
    ops, H = pkg("ops"), pkg("_hip")
    B, n_max, Hf, Wf = 2, 1000, 24, 32
    code = H.dtype_code(dtype)
    uv, cnt = _uv_case(B, n_max, Hf, Wf, 13, True)
    uv, cnt = uv.cuda(), cnt.cuda()
    gen = torch.Generator().manual_seed(4)
    for rows in (n_max, 1024):
        gfp = (torch.rand(B, rows, Cf, generator=gen) - 0.5).to(H.torch_dtype(code)).cuda()
        ref = torch.zeros(B, Hf, Wf, Cf, device="cuda")
        for b in range(B):
            ops.point_sample_bwd(code, gfp[b], uv[b], cnt[b:b + 1], min(rows, n_max), ref[b])
        got = torch.full((B, Hf, Wf, Cf), float("nan"), device="cuda")
        ops.point_sample_bwd_det(code, gfp, uv, ops.cam_invert(uv, cnt, n_max, Hf, Wf), got)
        assert torch.isfinite(got).all()
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
        assert float((got == 0).all(dim=-1).sum()) > 0          # pixels nobody touches exist and were written as zeros


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_point_sample_backward_det_at_cfg2_size(dtype):
    """tests/test_gpu_benchsize.py::test_point_sample_backward_at_cfg2_size's harness around the gather kernel."""
    from test_gpu_benchsize import _cfg2_frame
    ops, H = pkg("ops"), pkg("_hip")
    g, pc, uv, n = _cfg2_frame(seed=6)
    Hf, Wf, Cf = 94, 311, 64
    rows = (n + 255) // 256 * 256
    code = H.dtype_code(dtype)
    gen = torch.Generator().manual_seed(3)
    gfp = (torch.rand(rows, Cf, generator=gen) - 0.5).to(H.torch_dtype(code))
    uvt = torch.from_numpy(uv)
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    gF = torch.full((1, Hf, Wf, Cf), float("nan"), device="cuda")
    cam = ops.cam_invert(uvt.cuda().unsqueeze(0), cnt, uvt.shape[0], Hf, Wf)
    ops.point_sample_bwd_det(code, gfp.cuda().unsqueeze(0), uvt.cuda().unsqueeze(0), cam, gF)
    pix, wts = tap_weights(uv[:n], Hf, Wf)
    want = torch.zeros(Hf * Wf, Cf, dtype=torch.float64)
    g64 = gfp[:n].double()
    for t in range(4):
        want.index_add_(0, pix[:, t], g64 * wts[:, t, None])
    got = gF.cpu().double().reshape(Hf * Wf, Cf)
    print("point-sample backward (gather) at cfg2 size, %s: off by %.3g of %.3g" % (dtype, float((got - want).abs().max()), float(want.abs().max())))
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
    assert float(gF.abs().sum()) > 0


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("C,npix", [(64, 70000), (36, 9001), (256, 17600), (128, 300), (192, 2 * 88 * 100)])
def test_rowscale_bias_bwd_det(C, npix, dtype):
    """fc2's bias gradient in fixed order: the bound of tests/test_gpu_elementwise.py::test_relu_mask_rowscale_bwd against fp64 sums,
    for the bias-only form and the one-pass form (whose masked gradient equals the default kernel's bit for bit)."""
    ops, H = pkg("ops"), pkg("_hip")
    gen = torch.Generator().manual_seed(6)
    tdt = H.torch_dtype(dtype)
    cnt = torch.randint(0, 4, (npix,), generator=gen).float()
    gy = (torch.rand(npix, C, generator=gen) - 0.5).to(tdt)
    y = torch.relu(torch.rand(npix, C, generator=gen) - 0.5).to(tdt)
    gd, yd = gy.cuda(), y.cuda()
    ref = (cnt[:, None].double() * gy.double()).sum(0) + 0.25
    bound = 1e-5 * float((cnt[:, None].double() * gy.double().abs()).sum(0).max()) + 1e-6
    ws = ops.rowscale_bias_det_workspace("cuda", C)
    ws.fill_(float("nan"))
    gb = torch.full((C,), 0.25, device="cuda")
    assert ops.rowscale_bias_bwd_det(dtype, gd, cnt.cuda(), gb, ws) is None
    assert float((gb.cpu().double() - ref).abs().max()) <= bound
    gb2 = torch.full((C,), 0.25, device="cuda")
    gout = ops.rowscale_bias_bwd_det(dtype, gd, cnt.cuda(), gb2, ws, y=yd)
    assert torch.equal(gb2, gb)
    dflt = torch.full((C,), 0.25, device="cuda")
    assert torch.equal(gout, ops.relu_mask_rowscale_bwd(dtype, gd, yd, cnt.cuda(), dflt))
    assert float((gb2 - dflt).abs().max()) <= 2 * bound


def _loss_case(sampling, n_boxes=20):
    from test_gpu_loss_sampling import _setup
    cfg, boxes, nb, cls, reg, Hh, W = _setup(n_boxes, far=True)
    return dict(cfg, loss_sampling=sampling), boxes, nb, cls, reg


@pytest.mark.parametrize("sampling", ["device", "compat"])
def test_loss_det_matches_atomic_kernels(sampling):
    """Both device entries of the loss with and without `deterministic`, same lists (device: the stateless sampler; compat: numpy's
    generator seeded alike): loss within 2e-6, gradients within rtol 1e-5 / atol 1e-7 -- the bounds of
    tests/test_gpu_loss_sampling.py::test_device_sampler_lists_properties_and_loss between the two default kernels."""
    Lm = pkg("loss")
    cfg, boxes, nb, cls, reg = _loss_case(sampling)
    out = []
    for det in (False, True):
        L = Lm.LossTotal(dict(cfg, deterministic=det)).cuda()
        c = cls.cuda().requires_grad_(True)
        r = reg.cuda().requires_grad_(True)
        np.random.seed(3)
        loss = L(boxes, nb, c, r)
        loss.backward()
        out.append((loss.item(), c.grad.clone(), r.grad.clone()))
    (l0, c0, r0), (l1, c1, r1) = out
    print("loss %s: default %.9g deterministic %.9g; grad diff cls %.3g reg %.3g" % (sampling, l0, l1, float((c0 - c1).abs().max()), float((r0 - r1).abs().max())))
    assert abs(l0 - l1) <= 2e-6 * max(1.0, abs(l0))
    assert torch.allclose(c0, c1, rtol=1e-5, atol=1e-7) and torch.allclose(r0, r1, rtol=1e-5, atol=1e-7)
    assert float(c1.abs().sum()) > 0 and float(r1.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ 3. bitwise repeatability of the kernels
def test_kernels_repeat_bitwise_under_a_bandwidth_hog():
    """Every new kernel 20 times on fixed inputs while a second stream copies 512 MB back and forth: torch.equal with run 0."""
    ops, H = pkg("ops"), pkg("_hip")
    Lm = pkg("loss")
    hog = Hog()
    K, h, w, stride, n_max, Cb = 3, 96, 64, 4, 300, 128
    xyz, cnt, idx, n, g = _knn_case("few", K, h, w, stride, n_max)
    P = (torch.rand(1, n_max, Cb, generator=g) - 0.5).cuda()
    ghs = (torch.rand(1, h, w, Cb, generator=g) - 0.5).cuda()
    w1d = ((torch.rand(Cb, 3, generator=g) - 0.5) * 0.2).cuda().reshape(-1)
    b1 = ((torch.rand(Cb, generator=g) - 0.5) * 0.2).cuda()
    B, pm, Hf, Wf, Cf = 2, 1000, 24, 32, 64
    uv, ucnt = _uv_case(B, pm, Hf, Wf, 13, True)
    uv, ucnt = uv.cuda(), ucnt.cuda()
    gfp = (torch.rand(B, pm, Cf, generator=g) - 0.5).cuda()
    npix, C = 70000, 64
    gy = (torch.rand(npix, C, generator=g) - 0.5).cuda()
    rcnt = torch.randint(0, 4, (npix,), generator=g).float().cuda()
    lcfg, boxes, nb, cls, reg = _loss_case("device")
    losses = {s: Lm.LossTotal(dict(lcfg, loss_sampling=s, deterministic=True)).cuda() for s in ("device", "compat")}
    ws = ops.fusion_bwd_det_workspace("cuda", K * h * w, Cb, 1)
    rws = ops.rowscale_bias_det_workspace("cuda", C)
    first = None
    for run in range(20):
        hog.kick()
        inv = ops.fusion_invert_sorted([idx], n_max)
        cam = ops.cam_invert(uv, ucnt, pm, Hf, Wf)
        gp = torch.full((1, n_max, Cb), float("nan"), device="cuda")
        gw, gb = torch.zeros(Cb * 3, device="cuda"), torch.zeros(Cb, device="cuda")
        ops.fusion_gather_bwd_det(H.F32, P, xyz.unsqueeze(0), inv, n_max, 0, (K, h, w), stride, AFF, w1d, b1, ghs, gp, gw, gb, ws)
        gF = torch.full((B, Hf, Wf, Cf), float("nan"), device="cuda")
        ops.point_sample_bwd_det(H.F32, gfp, uv, cam, gF)
        gb2 = torch.zeros(C, device="cuda")
        ops.rowscale_bias_bwd_det(H.F32, gy, rcnt, gb2, rws)
        lout = []
        for s in ("device", "compat"):
            L = losses[s]
            L.calls = 0
            c = cls.cuda().requires_grad_(True)
            r = reg.cuda().requires_grad_(True)
            np.random.seed(3)
            lv = L(boxes, nb, c, r)
            lv.backward()
            lout += [lv.detach().clone(), c.grad.clone(), r.grad.clone()]
        torch.cuda.synchronize()
        used = int(cam[0][-1])                                  # entries beyond the frames' point counts are never written
        res = [inv[0].clone(), inv[1].clone(), cam[0].clone(), cam[1][:used].clone(), gp, gw, gb, gF, gb2] + lout
        if first is None:
            first = res
            # preconditions: the sums really have three or more terms and cross a wave's range
            seg = np.diff(inv[0].cpu().numpy()[:n_max + 1])
            lists = np.diff(cam[0].cpu().numpy())
            assert seg.max() >= 3 and lists.max() >= 3
            assert seg.max() > 128                              # a point's run spans more than one wave's slice of 16..128 pairs
            assert lists.max() > 64
            continue
        for i, (a, b) in enumerate(zip(res, first)):
            assert torch.equal(a, b), "run %d: output %d differs from run 0" % (run, i)


# ------------------------------------------------------------------------------------------------ 4. bitwise repeatability of the step
def _cfg2_trainer(dtype, sampling, batch, graphs=False, deterministic=True):
    from test_gpu_benchsize import _cfg2_config
    det, T = pkg("detfill"), pkg("train")
    cfg = _cfg2_config(dtype, batch=batch)
    cfg.update(hip_graphs=graphs, loss_sampling=sampling, loss_reduction="mean", deterministic=deterministic)
    tr = T.Train(cfg)
    det.fill_state_dict(tr.model)
    return cfg, tr


def _cfg2_inputs(cfg, batch):
    det, calib, D = pkg("detfill"), pkg("calib"), pkg("data_import_carla")
    lim6 = (0.0, 70.4, -40.0, 40.0, -2.4, 0.8)
    pts = [torch.from_numpy(det.synthetic_points(100000, lim6, 41 + b)).cuda() for b in range(batch)]
    img = torch.stack([torch.from_numpy(det.synthetic_image(375, 1242, 41 + b)) for b in range(batch)], 0).cuda()
    bx = [D.synthetic_boxes(cfg, 7 + b, n=6) for b in range(batch)]
    boxes = torch.stack([t[0] for t in bx], 0).cuda()
    nb = torch.tensor([t[1] for t in bx])
    return D.FrameGeometry(cfg, calib.kitti_like_crt()), pts, img, boxes, nb


def _snapshot(tr):
    return [tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone(), tr.optimizer.m.clone(), tr.optimizer.v.clone()]


def _run_steps(tr, geo, pts, img, boxes, nb, steps, hog=None):
    """`steps` one_steps (numpy's generator seeded per step: the compat sampler draws from it); the snapshots after every step."""
    out = []
    for s in range(steps):
        if hog is not None:
            hog.kick(6)
        np.random.seed(100 + s)
        x_lidar, geom = tr.geometry_async(geo, pts)
        tr.one_step(x_lidar, img, boxes, nb, geom=geom)
        torch.cuda.synchronize()
        out.append(_snapshot(tr))
    return out


def _save_state(tr):
    return dict(p=tr.model.flat_params.clone(), b=tr.model._bufflat.clone(), m=tr.optimizer.m.clone(), v=tr.optimizer.v.clone(),
                n=tr.optimizer.step_count, calls=tr.loss_total.calls)


def _restore_state(tr, st):
    tr.model.flat_params.copy_(st["p"]); tr.model._bufflat.copy_(st["b"]); tr.optimizer.m.copy_(st["m"]); tr.optimizer.v.copy_(st["v"])
    tr.optimizer.step_count = st["n"]
    tr.loss_total.calls = st["calls"]


@pytest.mark.parametrize("dtype,sampling,batch,graphs", [("f32", "device", 2, False), ("f32", "compat", 2, False), ("bf16", "device", 2, False),
                                                         ("bf16", "compat", 2, False), ("bf16", "device", 1, True)])
def test_step_repeats_bitwise(dtype, sampling, batch, graphs):
    """cfg2 shapes, deterministic: true: three one_steps from the seeded state, twice, the second time under the hog -- loss, gradient
    arena, parameters and Adam's moments bit for bit."""
    cfg, tr = _cfg2_trainer(dtype, sampling, batch, graphs)
    geo, pts, img, boxes, nb = _cfg2_inputs(cfg, batch)
    st = _save_state(tr)
    hog = Hog()
    runs = []
    for rep in range(2):
        _restore_state(tr, st)
        runs.append(_run_steps(tr, geo, pts, img, boxes, nb, 3, hog if rep else None))
    names = ("loss", "flat_grads", "flat_params", "adam_m", "adam_v")
    for s, (a, b) in enumerate(zip(*runs)):
        for nme, x, y in zip(names, a, b):
            assert torch.equal(x, y), "step %d: %s differs between the two executions (max diff %g)" % (s, nme, float((x.float() - y.float()).abs().max()))
    assert not torch.equal(runs[0][0][2], runs[0][2][2]) and np.isfinite(float(runs[0][2][0]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deterministic_gradients_tie_to_default_mode(dtype):
    """One forward + backward at cfg2 size from the seeded state in both modes: prediction and LiDAR part of the arena bit-equal,
    camera / fusion part per parameter tensor within relative L2 3e-3 and 1.5e-2 of the tensor's maximum (what
    test_cfg2_size_fp32_backward_matches_cpu_statement allows these gradients against the CPU statement).  The figures are printed."""
    det = pkg("detfill")
    res = {}
    for mode in (False, True):
        cfg, tr = _cfg2_trainer(dtype, "device", 2, deterministic=mode)
        geo, pts, img, boxes, nb = _cfg2_inputs(cfg, 2)
        x_lidar, geom = tr.geometry_async(geo, pts)
        pred = tr.model(x_lidar, img, geom=geom)
        R = torch.from_numpy(det.uniform(tuple(pred.shape), 99, -1.0, 1.0)).cuda()
        R[:, 18:] = 0
        tr.optimizer.zero_grad()
        (pred * R).sum().backward()
        torch.cuda.synchronize()
        layers = tr.model._plan.layers
        lidar_end = min(L.w_off for L in layers if L.name.startswith("image_"))
        res[mode] = (pred.detach().clone(), tr.model.flat_grads.clone(), {k: p.grad.detach().clone() for k, p in tr.model.named_parameters()}, lidar_end)
        del tr
        torch.cuda.empty_cache()
    (p0, g0, n0, le), (p1, g1, n1, _) = res[False], res[True]
    assert torch.equal(p0, p1)
    assert torch.equal(g0[:le], g1[:le])
    rel = float((g0[le:] - g1[le:]).abs().max() / g0[le:].abs().max())
    worst = []
    for k in n0:
        a, b = n0[k].float(), n1[k].float()
        scale = float(a.abs().max())
        e = float((a - b).abs().max()) / (scale + 1e-20)
        l2 = float((a - b).norm() / (a.norm() + 1e-20))
        worst.append((e, l2, k, scale))
    worst.sort(reverse=True)
    print("deterministic vs default, %s: camera/fusion arena max diff %.3g of the maximum; worst tensors (max-rel, L2): %s" % (dtype, rel, worst[:3]))
    bad = [t for t in worst if (t[0] > 1.5e-2 or t[1] > 3e-3) and t[0] * t[3] > 1e-6]
    assert not bad, bad[:5]


# ------------------------------------------------------------------------------------------------ 5. checkpoint resume with fusion on
def test_checkpoint_resume_bitwise_with_fusion(tmp_path):
    """The fused counterpart of tests/test_gpu_model.py's resume test: save after step 2, run steps 3 and 4; a fresh trainer loads the
    checkpoint and runs steps 3 and 4: parameters bit-identical."""
    cfg, tr = _cfg2_trainer("bf16", "device", 1)
    geo, pts, img, boxes, nb = _cfg2_inputs(cfg, 1)

    def step(t, s):
        np.random.seed(100 + s)
        x_lidar, geom = t.geometry_async(geo, pts)
        t.one_step(x_lidar, img, boxes, nb, geom=geom)

    for s in range(2):
        step(tr, s)
    path = os.path.join(str(tmp_path), "ckpt.pt")
    tr.save_checkpoint(path)
    for s in range(2, 4):
        step(tr, s)
    torch.cuda.synchronize()
    want = tr.model.flat_params.clone()
    del tr
    torch.cuda.empty_cache()
    _, tr2 = _cfg2_trainer("bf16", "device", 1)
    tr2.load_checkpoint(path)
    for s in range(2, 4):
        step(tr2, s)
    torch.cuda.synchronize()
    assert torch.equal(tr2.model.flat_params, want)

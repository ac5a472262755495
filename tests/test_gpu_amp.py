"""GPU suite: the guarded optimiser step (csrc/amp.hip; config keys loss_scale / grad_clip_norm) -- exact skip of a non-finite
step, scaling that changes nothing where it is exact, GradScaler's schedule on the device, the non-finite flag and the global
norm against torch, no new host synchronisation, checkpoints, captured graphs, the bucketed all-reduce path and the cfg2 size.
The LiDAR-only configs are used where a check is bitwise: their backward is deterministic from run to run."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from _amp_ref import fp16_landing_scale, scale_schedule
from _util import PKG, ROOT, golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu


def tiny_input():
    """The tiny golden config's voxel input (the same frames as tests/test_gpu_model.py builds)."""
    det = pkg("detfill")
    u = det.uniform((2, 32, 64, 32), 4242, 0.0, 1.0)
    m = det.uniform((2, 32, 64, 32), 4242 + 17, 0.0, 1.0) < 0.12
    return torch.from_numpy((u * m).astype(np.float32))


def tiny_cfg(dtype, **over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg["dtype"] = dtype
    cfg.update(over)
    return cfg


class Tiny(object):
    """A Train on the tiny golden config, batch B, with the golden boxes; step(s, bad) = one one_step with np.random.seed(100 + s),
    bad = None / "nan" / "inf" written into one voxel of the input."""

    def __init__(self, dtype, B=1, **over):
        self.T = pkg("train")
        lz = load_golden("loss.npz")
        self.cfg = tiny_cfg(dtype, **over)
        self.tr = self.T.Train(self.cfg)
        pkg("detfill").fill_state_dict(self.tr.model)
        self.x = tiny_input()[:B].cuda()
        self.img = torch.zeros(B, 3, 8, 8, dtype=torch.uint8, device="cuda")
        self.boxes, self.nb = torch.from_numpy(lz["bboxes"])[:B], torch.from_numpy(lz["nbox"])[:B]

    def step(self, s, bad=None, seed=None):
        x = self.x
        if bad is not None:
            x = x.clone()
            x[0, 3, 17, 9] = float("nan") if bad == "nan" else float("inf")
        np.random.seed(100 + s if seed is None else seed)
        self.tr.one_step(x, self.img, self.boxes, self.nb)
        torch.cuda.synchronize()

    def state(self):
        o = self.tr.optimizer
        return o.model.flat_params.clone(), o.m.clone(), o.v.clone()

    def amp(self):
        a = self.tr.optimizer.amp
        return {"scale": float(a.scale_next.item()), "tracker": int(a.growth_tracker.item()), "found": int(a.found_inf.item()),
                "applied": int(a.applied_steps.item()), "skipped": int(a.skipped_steps.item())}


def _equal3(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_nonfinite_step_is_skipped_exactly(dtype, bad):
    """Step 0 clean, step 1 with a NaN (or +inf) in the voxel input, step 2 clean, loss_scale dynamic.  After step 1 the gradient
    arena holds a non-finite value and parameters / moments are bitwise those after step 0; the scale is halved, one step skipped,
    one applied.  f32 / bf16: after step 2 the parameters equal a loss_scale none run of steps 0 and 2 (power-of-two scaling is
    exact in these types).  (On the plain path the NaN reaches the parameters.)"""
    t = Tiny(dtype, loss_scale="dynamic")
    t.step(0)
    after0 = t.state()
    a0 = t.amp()
    assert a0["found"] == 0 and a0["applied"] == 1 and a0["scale"] == 65536.0
    t.step(1, bad)
    assert not bool(torch.isfinite(t.tr.model.flat_grads).all()), "the bad frame did not reach the gradient"
    assert _equal3(t.state(), after0)
    a1 = t.amp()
    assert a1["found"] == 1 and a1["scale"] == 32768.0 and a1["skipped"] == 1 and a1["applied"] == 1 and a1["tracker"] == 0
    assert int(t.tr.skipped_steps().item()) == 1 and float(t.tr.loss_scale().item()) == 32768.0
    assert t.tr.optimizer.step_count == 1
    t.step(2)
    p2 = t.state()[0]
    assert bool(torch.isfinite(p2).all())
    a2 = t.amp()
    assert a2["applied"] == 2 and a2["skipped"] == 1 and a2["found"] == 0
    if dtype in ("f32", "bf16"):
        ref = Tiny(dtype)
        ref.step(0)
        ref.step(2)
        assert torch.equal(p2, ref.state()[0])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_static_power_of_two_scale_equals_no_scale(dtype):
    a, b = Tiny(dtype, loss_scale=1024), Tiny(dtype)
    la, lb = [], []
    for s in range(3):
        a.step(s)
        b.step(s)
        la.append(a.tr.loss_value.detach().clone())
        lb.append(b.tr.loss_value.detach().clone())
        assert _equal3(a.state(), b.state()), "step %d" % s
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert a.amp()["scale"] == 1024.0 and a.amp()["applied"] == 3


def test_fp16_overflow_backs_off_to_a_working_scale():
    """f16, dynamic from 2**30, the same frame and seed every step: the device skips until its scale is within one power of two of
    the largest power of two at which the quantisation-aware CPU statement's fp16 gradients are finite (oracle/model_quant_ref.py +
    oracle/loss_ref.py; the one power of two is fp32 summation order moving a value across fp16's overflow boundary).  Scale and
    growth tracker follow torch._amp_update_scale_ fed with the device's own found_inf sequence; the first applied step equals a
    fresh run with that scale as a static one, bit for bit."""
    t = Tiny("f16", loss_scale="dynamic", loss_scale_init=2.0 ** 30)
    e_star = fp16_landing_scale(t.cfg, tiny_input()[:1], t.boxes, t.nb, 100)
    assert e_star is not None
    print("oracle landing scale 2**%d" % e_star)
    found, scales = [], []
    before = t.state()
    landing = None
    for s in range(32):
        used = t.amp()["scale"]
        t.step(s, seed=100)
        a = t.amp()
        found.append(bool(a["found"]))
        want = scale_schedule(found, 2.0 ** 30)[-1]
        assert (a["scale"], a["tracker"]) == want, (s, a, want)
        if not a["found"]:
            landing = used
            break
        assert _equal3(t.state(), before)
    assert landing is not None, "no step was applied"
    e = math.log2(landing)
    print("device: %d skips, landing scale 2**%g" % (sum(found), e))
    assert e == int(e) and abs(e - e_star) <= 1
    ref = Tiny("f16", loss_scale=landing)
    ref.step(0, seed=100)
    assert ref.amp()["found"] == 0
    assert _equal3(t.state(), ref.state())


def test_dynamic_scale_growth_follows_torch():
    t = Tiny("f32", loss_scale="dynamic", loss_scale_growth_interval=2)
    found = []
    for s in range(6):
        t.step(s, "nan" if s == 3 else None)
        a = t.amp()
        found.append(bool(a["found"]))
        assert (a["scale"], a["tracker"]) == scale_schedule(found, 65536.0, growth_interval=2)[-1], (s, a)
    assert found == [False, False, False, True, False, False]
    assert t.amp()["scale"] == 131072.0            # grown at step 1, halved at 3, grown at 5


def _direct_state(scale=1.0):
    return pkg("ops").AmpState(torch.device("cuda"), scale)


@pytest.mark.parametrize("val", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_nonfinite_flag_matches_torch(val, where):
    ops = pkg("ops")
    n = 1_000_003
    g = torch.randn(n, generator=torch.Generator().manual_seed(7))
    g[{"first": 0, "last": n - 1, "middle": 523_459}[where]] = val
    ref = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_([g.clone()], ref, torch.ones(1))
    st = _direct_state()
    ops.grad_stats(g.cuda(), st)
    ops.amp_update(st, 1.0, True, 2.0, 0.5, 2000, None, 1e-4, 0.9, 0.999)
    assert int(st.found_inf.item()) == int(ref.item()) == 1
    # finite values up to 1e30 (their squares overflow fp32): no flag while clipping is off
    big = torch.randn(n, generator=torch.Generator().manual_seed(8)) * 1e29
    big[n - 1] = 1e30
    st = _direct_state()
    ops.grad_stats(big.cuda(), st)
    ops.amp_update(st, 1.0, True, 2.0, 0.5, 2000, None, 1e-4, 0.9, 0.999)
    ref = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_([big.clone()], ref, torch.ones(1))
    assert int(st.found_inf.item()) == int(ref.item()) == 0


def _cfg2_config(dtype, batch=1, fusion=True, n_points=100000):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")))
    cfg.update(dict(voxel_length=704, voxel_width=800, voxel_channel=32, lidar_x_min=0.0, lidar_x_max=70.4, lidar_y_min=-40.0,
                    lidar_y_max=40.0, lidar_z_min=-2.4, lidar_z_max=0.8, image_height=375, image_width=1242, max_num_pc=n_points,
                    batch_size=batch, dtype=dtype, projection_mode="correct", voxel_mode="compat"))
    cfg["fusion"] = dict(enabled=fusion, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    return cfg


def test_clipping_norm_matches_torch():
    """Random arena of the cfg2 model's size.  grad_norm within 1e-5 relative of torch.linalg.vector_norm in float64 (fp32 partial
    sums in a tree of depth ~log2(n) = 25: at most ~25 * 2**-24 = 1.5e-6, so 1e-5 leaves ~6x).  max_norm a tenth of the norm:
    m = (1 - b1) * g * coef_ref to 1e-5 of max|m|.  max_norm above the norm: bitwise the unclipped step."""
    ops = pkg("ops")
    n = pkg("model").ObjectDetection_DCF(_cfg2_config("bf16", batch=2)).flat_params.numel()
    print("cfg2 arena: %d elements" % n)
    assert 24_000_000 < n < 24_100_000
    g = torch.randn(n, generator=torch.Generator().manual_seed(11)) * 1e-3
    norm_ref = float(torch.linalg.vector_norm(g.double()))
    gd = g.cuda()
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 1e-4
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(12)).cuda()
    # clipped
    st = _direct_state()
    p, m, v = p0.clone(), torch.zeros_like(gd), torch.zeros_like(gd)
    max_norm = norm_ref / 10
    ops.grad_stats(gd, st)
    ops.amp_update(st, 1.0, False, 2.0, 0.5, 2000, max_norm, lr, b1, b2)
    ops.adam_step_guarded(p, gd, m, v, b1, b2, eps, st)
    got = float(st.grad_norm.item())
    print("grad_norm %r, float64 reference %r, rel %g" % (got, norm_ref, abs(got - norm_ref) / norm_ref))
    assert abs(got - norm_ref) <= 1e-5 * norm_ref
    coef_ref = max_norm / (norm_ref + 1e-6)
    want = (1 - b1) * g.double() * coef_ref
    err = float((m.cpu().double() - want).abs().max() / want.abs().max())
    print("clipped m: rel err %g (coef %r, reference %r)" % (err, float(st.clip_coef.item()), coef_ref))
    assert err <= 1e-5
    assert int(st.found_inf.item()) == 0 and int(st.applied_steps.item()) == 1
    # not clipped: the plain Adam step, bitwise
    st = _direct_state()
    p, m, v = p0.clone(), torch.zeros_like(gd), torch.zeros_like(gd)
    ops.grad_stats(gd, st)
    ops.amp_update(st, 1.0, False, 2.0, 0.5, 2000, norm_ref * 2, lr, b1, b2)
    ops.adam_step_guarded(p, gd, m, v, b1, b2, eps, st)
    assert float(st.clip_coef.item()) == 1.0
    pr, mr, vr = p0.clone(), torch.zeros_like(gd), torch.zeros_like(gd)
    ops.adam_step(pr, gd, mr, vr, lr, b1, b2, eps, 1, 1.0)
    assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr)


def test_no_new_host_synchronisation(monkeypatch):
    """Three one_step calls with loss_scale dynamic + grad_clip_norm make exactly as many host-synchronising calls as with none."""
    counts = {}

    def counting(name, fn):
        def wrapped(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **k)
        return wrapped

    runs = {}
    for mode, over in (("none", {}), ("guarded", dict(loss_scale="dynamic", grad_clip_norm=1e3))):
        t = Tiny("f32", **over)
        t.step(0)                                   # first step: lazy set-up on both paths, not counted
        counts.clear()
        with monkeypatch.context() as mp:
            for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
                                (torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize")):
                mp.setattr(owner, name, counting(owner.__name__ + "." + name, getattr(owner, name)))
            for s in range(1, 4):
                np.random.seed(100 + s)
                t.tr.one_step(t.x, t.img, t.boxes, t.nb)
        runs[mode] = dict(counts)
        torch.cuda.synchronize()
    print(runs)
    assert runs["guarded"] == runs["none"]


def test_checkpoint_carries_the_guard_state(tmp_path):
    over = dict(loss_scale="dynamic", loss_scale_growth_interval=3)
    a = Tiny("f32", **over)
    a.step(0)
    a.step(1, "nan")
    a.tr.save_checkpoint(str(tmp_path / "ck.pt"), epoch=3)
    a.step(2)
    b = Tiny("f32", **over)
    assert b.tr.load_checkpoint(str(tmp_path / "ck.pt")) == 3
    b.step(2)
    assert torch.equal(a.tr.model.flat_params, b.tr.model.flat_params)
    assert a.amp() == b.amp()
    assert b.amp()["skipped"] == 1 and b.amp()["applied"] == 2 and b.amp()["scale"] == 32768.0
    # a checkpoint of the plain path loads: step count from it, the configured initial scale
    c = Tiny("f32")
    c.step(0)
    c.step(1)
    c.tr.save_checkpoint(str(tmp_path / "plain.pt"))
    d = Tiny("f32", **over)
    d.tr.load_checkpoint(str(tmp_path / "plain.pt"))
    assert d.tr.optimizer.step_count == 2 and d.amp()["scale"] == 65536.0 and d.amp()["skipped"] == 0
    assert torch.equal(d.tr.model.flat_params, c.tr.model.flat_params)
    d.step(2)
    c.step(2)
    assert torch.equal(d.tr.model.flat_params, c.tr.model.flat_params)


def test_batch1_hip_graphs_skip_and_match_eager():
    """The batch-1 default (captured graphs) with loss_scale dynamic: the NaN frame is skipped, and the clean steps match the eager
    guarded run within the bounds of test_hip_graph_replay_matches_eager (rtol 1e-5, atol 1e-6)."""
    runs = {}
    for graphs in ("auto", False):
        t = Tiny("f32", loss_scale="dynamic", hip_graphs=graphs)
        assert t.tr.model.graphs_wanted(1) == (graphs == "auto")
        out = []
        for s, bad in ((0, None), (1, "nan"), (2, None), (3, None)):
            t.step(s, bad)
            out.append((t.tr.model.flat_grads.clone(), t.state(), t.amp()))
        runs[graphs] = out
        assert _equal3(out[1][1], out[0][1]) and out[1][2]["skipped"] == 1
        assert out[3][2]["applied"] == 3 and out[3][2]["skipped"] == 1
    for s in (0, 2, 3):
        (gg, sg, _), (ge, se, _) = runs["auto"][s], runs[False][s]
        assert torch.allclose(gg, ge, rtol=1e-5, atol=1e-6), s
        for a, b in zip(sg, se):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), s


def test_bucketed_allreduce_path_scans_the_reduced_arena(tmp_path):
    """A one-rank gloo group in this process, batch 2, overlap_allreduce force, bf16 gradient buckets: the gradient goes through
    the bucket hook, is rounded to bf16, "summed" and widened back before the scan; a NaN frame is skipped there."""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        t = Tiny("f32", B=2, loss_scale="dynamic", overlap_allreduce="force", grad_bucket_dtype="bf16")
        t.step(0)
        assert t.tr._widen, "the bucketed path was not taken"
        s0 = t.state()
        t.step(1, "nan")
        assert t.tr._widen and t.tr._reduced == t.tr.model.flat_grads.numel()
        assert not bool(torch.isfinite(t.tr.model.flat_grads).all())
        assert _equal3(t.state(), s0)
        a = t.amp()
        assert a["skipped"] == 1 and a["applied"] == 1 and a["scale"] == 32768.0
        t.step(2)
        assert t.amp()["applied"] == 2 and bool(torch.isfinite(t.state()[0]).all())
    finally:
        dist.destroy_process_group()


def test_cfg2_size_guarded_step_matches_plain_step():
    """cfg2 size, bf16 with fusion, batch 2: loss_scale dynamic at 2**16 with grad_clip_norm above the norm against none, one step.
    LiDAR-stream ranges of params, m, v bitwise; camera + fusion ranges (float atomics in the fusion backward) within the stress
    test's bf16 bound of 3e-4 of the maximum for m, twice that for v (quadratic in g), and parameters bitwise-close (one ulp plus
    1e-3 lr) wherever the gradient is further from zero than that noise -- an Adam step's sign can flip only below it."""
    det, calib, D, T = pkg("detfill"), pkg("calib"), pkg("data_import_carla"), pkg("train")
    lim6 = (0.0, 70.4, -40.0, 40.0, -2.4, 0.8)
    crt = calib.kitti_like_crt()
    pts = [torch.from_numpy(det.synthetic_points(100000, lim6, 31 + b)).cuda() for b in range(2)]
    img = torch.stack([torch.from_numpy(det.synthetic_image(375, 1242, 31 + b)) for b in range(2)], 0).cuda()
    boxes, nb = D.synthetic_boxes(_cfg2_config("bf16", batch=2), 31, n=3)
    boxes, nb = torch.stack([boxes, boxes], 0), torch.tensor([nb, nb])
    res = {}
    clip = None
    for mode in ("none", "guarded"):
        cfg = _cfg2_config("bf16", batch=2)
        if mode == "guarded":
            cfg.update(loss_scale="dynamic", loss_scale_init=2.0 ** 16, grad_clip_norm=clip)
        tr = T.Train(cfg)
        det.fill_state_dict(tr.model)
        geo = D.FrameGeometry(cfg, crt)
        x_lidar, geom = tr.geometry_async(geo, pts)
        np.random.seed(100)
        tr.one_step(x_lidar, img, boxes, nb, geom=geom)
        torch.cuda.synchronize()
        o = tr.optimizer
        res[mode] = (o.model.flat_params.clone(), o.m.clone(), o.v.clone(), tr.model.flat_grads.clone())
        if mode == "none":
            clip = 10.0 * float(torch.linalg.vector_norm(tr.model.flat_grads.double()))
        else:
            assert int(o.amp.found_inf.item()) == 0 and float(o.amp.clip_coef.item()) == 1.0
            print("grad_norm %g (clip at %g)" % (float(tr.grad_norm().item()), clip))
            lidar_end = min(L.w_off for L in tr.model._plan.layers if L.name.startswith("image_"))
            lr = cfg["learning_rate"]
        del tr
        torch.cuda.empty_cache()
    (pn, mn, vn, gn), (pg, mg, vg, gg) = res["none"], res["guarded"]
    assert 0 < lidar_end < pn.numel()
    L = slice(0, lidar_end)
    assert torch.equal(pg[L], pn[L]) and torch.equal(mg[L], mn[L]) and torch.equal(vg[L], vn[L])
    C = slice(lidar_end, pn.numel())
    bound = 3e-4
    em = float((mg[C] - mn[C]).abs().max() / mn[C].abs().max())
    ev = float((vg[C] - vn[C]).abs().max() / vn[C].abs().max())
    print("camera + fusion: m rel %g, v rel %g" % (em, ev))
    assert em <= bound and ev <= 2 * bound
    clear = mn[C].abs() > 2 * bound * mn[C].abs().max()
    ulp = torch.nextafter(pn[C].abs(), torch.full_like(pn[C], float("inf"))) - pn[C].abs()
    dp = (pg[C] - pn[C]).abs()
    assert bool((dp[clear] <= ulp[clear] + 1e-3 * lr).all()), float(dp[clear].max())

"""The execution plan with grouped launches (engine.conv_fwd_group / conv_dgrad_group sites, option IGEMM_GROUP) against the same
plan with every convolution in a launch of its own (IGEMM_GROUP=0), on one seeded input at a small size: a 32x64x96 grid, a 64x160
image, batch 2, bf16.  Grouping only changes which grid a layer's workgroups belong to, so everything that does not pass through
the fusion backward's float atomics must be equal bit for bit: predictions, the camera map, and the gradient arena of the LiDAR
stream alone; of the fused model, the forward and the LiDAR stream's and fc2's weight gradients -- and with `deterministic: true`
(no float atomics anywhere) the whole arena, camera stream and fusion layers included.  The profile names must show that the
grouped launches ran (and that none ran with the option off)."""
import numpy as np
import pytest
import torch

from _util import pkg

pytestmark = pytest.mark.gpu

LIM6 = (0.0, 16.0, -12.0, 12.0, -2.4, 0.8)


def _config(fusion, deterministic=False):
    import os
    import yaml
    from _util import PKG, ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")))
    cfg.update(dict(voxel_length=64, voxel_width=96, voxel_channel=32, lidar_x_min=0.0, lidar_x_max=16.0, lidar_y_min=-12.0, lidar_y_max=12.0,
                    lidar_z_min=-2.4, lidar_z_max=0.8, image_height=64, image_width=160, max_num_pc=4096, batch_size=2, dtype="bf16",
                    projection_mode="correct", voxel_mode="compat", deterministic=deterministic))
    cfg["lidar_module"] = dict(out_feature1=32, out_feature2=64, out_feature3=128, out_feature4=192, out_feature5=256,
                               num_res_block1=1, num_res_block2=1, num_res_block3=2, num_res_block4=1, num_res_block5=1)
    cfg["fusion"] = dict(enabled=fusion, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    return cfg


def _both_ways(cfg):
    """-> {grouped?: (pred, gradient arena, camera map or None, launch names)} and the model."""
    det, calib, D, T, H = pkg("detfill"), pkg("calib"), pkg("data_import_carla"), pkg("train"), pkg("_hip")
    Kc = np.array([[80.0, 0.0, 80.0], [0.0, 80.0, 32.0], [0.0, 0.0, 1.0]])
    crt = calib.crt_from(Kc, calib.R_LIDAR_TO_CAM)
    pts = [torch.from_numpy(det.synthetic_points(4000, LIM6, 71 + b)).cuda() for b in range(2)]
    img = torch.stack([torch.from_numpy(det.synthetic_image(64, 160, 71 + b)) for b in range(2)], 0).cuda()
    tr = T.Train(cfg)
    det.fill_state_dict(tr.model)
    geo = D.FrameGeometry(cfg, crt)
    R, out = None, {}
    try:
        for grouped in (False, True):
            H.set_option("IGEMM_GROUP", None if grouped else 0)
            x_lidar, geom = tr.geometry_async(geo, pts)
            torch.cuda.synchronize()
            K = tr.model._ensure_backend(x_lidar.device)
            H.call("dcf_prof_reset")
            H.call("dcf_prof_enable", 1)
            try:
                pred = tr.model(x_lidar, img, geom=geom)
                if R is None:
                    R = torch.from_numpy(det.uniform(tuple(pred.shape), 99, -1.0, 1.0)).cuda()
                    R[:, 18:] = 0
                (pred * R).sum().backward()
                fmap = tr.model._plan.forward_image(K, img, save=False).clone() if cfg["fusion"]["enabled"] else None
                torch.cuda.synchronize()
            finally:
                H.call("dcf_prof_enable", 0)
            names = {n: v[1] for n, v in H.prof_read().items()}
            H.call("dcf_prof_reset")
            out[grouped] = (pred.detach().clone(), tr.model.flat_grads.clone(), fmap, names)
    finally:
        H.set_option("IGEMM_GROUP", None)
    return out, tr.model


def _assert_names(out, fwd_min, dgrad_min):
    off, on = out[False][3], out[True][3]
    assert not [n for n in off if "_grp_" in n and n.startswith(("conv_fwd", "conv_dgrad"))], sorted(off)
    nf = sum(c for n, c in on.items() if n.startswith("conv_fwd_grp_bf16<"))
    nd = sum(c for n, c in on.items() if n.startswith("conv_dgrad_grp_bf16<"))
    assert nf >= fwd_min and nd >= dgrad_min, "grouped launches: %d forward, %d input-gradient; %s" % (nf, nd, sorted(on.items()))
    # every grouped launch replaces at least two single ones
    count = lambda d: sum(c for n, c in d.items() if n.startswith(("conv_fwd", "conv_dgrad")))
    assert count(on) <= count(off) - (nf + nd), (count(on), count(off), nf, nd)


def test_lidar_stream_grouped_equals_single_launches():
    out, _ = _both_ways(_config(fusion=False))
    (p0, g0, _, _), (p1, g1, _, _) = out[False], out[True]
    # the four stage heads and the three FPN laterals forward; the FPN laterals' input gradients
    _assert_names(out, 5, 1)
    assert torch.equal(p0, p1), "predictions differ: max abs %g" % float((p0 - p1).abs().max())
    assert float(g0.abs().max()) > 0
    assert torch.equal(g0, g1), "gradient arena differs: max abs %g of %g" % (float((g0 - g1).abs().max()), float(g0.abs().max()))


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "deterministic"])
def test_fused_model_grouped_equals_single_launches(deterministic):
    out, model = _both_ways(_config(fusion=True, deterministic=deterministic))
    (p0, g0, f0, _), (p1, g1, f1, _) = out[False], out[True]
    # + the camera stream's three stage heads and its laterals, the sites' fc1_feat products; the camera laterals' input gradients
    _assert_names(out, 10, 2)
    assert torch.equal(f0, f1), "camera map differs: max abs %g" % float((f0.float() - f1.float()).abs().max())
    assert torch.equal(p0, p1), "predictions differ: max abs %g" % float((p0 - p1).abs().max())
    assert float(g0.abs().max()) > 0
    if deterministic:
        assert torch.equal(g0, g1), "gradient arena differs: max abs %g of %g" % (float((g0 - g1).abs().max()), float(g0.abs().max()))
        return
    checked = 0
    for key, _, off, n, _ in model._plan.table.entries:
        if key.startswith("lidar_backbone.") or key.endswith(".fc2.weight"):
            assert torch.equal(g0[off:off + n], g1[off:off + n]), "%s: gradient differs, max abs %g" % (key, float((g0[off:off + n] - g1[off:off + n]).abs().max()))
            checked += n
    assert checked > 1000000           # the LiDAR stream's few million parameters

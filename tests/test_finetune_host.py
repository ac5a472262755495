"""CPU: the host side of fine-tuning the camera stream (finetune.py, optim.parse_param_groups / group_ids / group_table /
frozen_trunk_units) -- the normalisation statement against float64, the torchvision-layout import on synthesised
dictionaries, every refusal of the param_groups parser, the id array, decay_mul per group, the trunk-prefix derivation, and that absent
keys leave today's objects."""
import numpy as np
import pytest
import torch

import _finetune_ref as FR
import _optim_ref as R
from _util import golden_cfg, load_golden, pkg

F = np.float32


def _cfg(arch="resnet18", **fusion):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dtype="f32"))
    cfg["fusion"] = dict(dict(enabled=True, K=3, r_max=None, image_channels=64, image_stream=arch, zero_init_last=False), **fusion)
    return cfg


def _model(arch="resnet18", **fusion):
    net = pkg("model").ObjectDetection_DCF(_cfg(arch, **fusion))
    pkg("detfill").fill_state_dict(net)
    return net


def _bits(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- normalisation
def test_normalisation_statement_against_float64():
    """All 256 byte values x three tables (ImageNet in RGB and in BGR order, the [-1, 1] table), within 1 ulp of float64.  The bound
    is no theorem for every table: three roundings can add up to 1.5 of these units, and the hostile table of _finetune_ref (mean 1e-3
    under std 1e-2) measures 1.09 -- that table is part of the bit-for-bit kernel test, not of this comparison."""
    FT = pkg("finetune")
    img = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16).repeat(3, 1)
    for mean, std in FR.NORM_TABLES[1:4]:
        got = FT.normalize_image(img, mean, std)
        assert got.dtype == F and got.shape == img.shape
        for c in range(3):
            want = FR.norm_f64(np.arange(256), mean[c], std[c])
            # within 1 ulp of fp32: the ulp of the chain's largest value carried through the division, max(|s/255|, |mean|, |s/255 -
            # mean|) / std.  (Where the subtraction cancels, the quotient's half ulp is an error of many ulps of the small RESULT
            # for any evaluation that rounds three times; the kernel is pinned to the statement bit for bit, not to float64.)
            q = np.arange(256) / 255.0
            big = np.maximum(np.maximum(np.abs(q), abs(float(F(mean[c])))), np.abs(q - float(F(mean[c])))) / float(F(std[c]))
            tol = big * 2.0 ** -23                                        # one unit in the last place of a 24-bit significand
            err = np.abs(got[0, c].reshape(-1).astype(np.float64) - want)
            print("image_norm mean %r std %r plane %d: worst error %.3f ulp" % (mean, std, c, float((err / tol).max())))
            assert (err <= tol).all(), (mean, std, c, int(np.argmax(err - tol)))
    ident = FT.normalize_image(img, (0, 0, 0), (1, 1, 1))
    plain = img.astype(F) / F(255.0)
    assert np.array_equal(ident.view(np.uint32), plain.view(np.uint32))
    y = FT.image_to_nhwc4_ref(img, *FR.NORM_TABLES[1])
    assert y.shape == (1, 22, 24, 4) and not y[..., 3].any() and not y[:, :3].any() and not y[:, :, :3].any() and not y[:, :, 19:].any()
    assert np.array_equal(y[0, 3:19, 3:19, :3], FT.normalize_image(img, *FR.NORM_TABLES[1])[0].transpose(1, 2, 0))


def test_image_norm_config():
    FT = pkg("finetune")
    assert FT.parse_image_norm(None) is None
    m, s = FT.parse_image_norm({"mean": [0.1, 0.2, 0.3], "std": [1, 2, 3]})
    assert m.dtype == F and s.dtype == F and m.tolist() == [float(F(0.1)), float(F(0.2)), float(F(0.3))]
    for bad in ([1, 2, 3], {"mean": [0, 0, 0]}, {"mean": [0, 0], "std": [1, 1, 1]}, {"mean": [0, 0, 0], "std": [1, 0, 1]},
                {"mean": [0, 0, 0], "std": [1, -1, 1]}, {"mean": [0, float("nan"), 0], "std": [1, 1, 1]},
                {"mean": [0, 0, 0], "std": [1, float("inf"), 1]}, {"mean": [0, 0, 0], "std": [1, 1, 1], "scale": 2},
                {"mean": [0, 0, 0], "std": [1, 1e-60, 1]}, {"mean": [0, True, 0], "std": [1, 1, 1]}, {"mean": "0,0,0", "std": [1, 1, 1]}):
        with pytest.raises(ValueError):
            FT.parse_image_norm(bad)
    M = pkg("model")
    with pytest.raises(ValueError):                                       # when the model is built
        M.ObjectDetection_DCF(_cfg(image_norm={"mean": [0, 0, 0], "std": [0, 1, 1]}))
    with pytest.raises(ValueError):
        M.ObjectDetection_DCF(_cfg(image_input_order="grb"))
    assert M.ObjectDetection_DCF(_cfg())._plan.image_norm is None
    assert M.ObjectDetection_DCF(_cfg())._plan.img_frozen == 0
    got = M.ObjectDetection_DCF(_cfg(image_norm={"mean": [0.1, 0.2, 0.3], "std": [1, 2, 3]}))._plan.image_norm
    assert got[1].tolist() == [1.0, 2.0, 3.0]


# ---------------------------------------------------------------------------------------------------------------- the import
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_import_of_a_torchvision_layout_trunk(arch):
    FT = pkg("finetune")
    src = FR.tv_state_dict(arch, 1)
    assert "fc.weight" in src and "layer1.0.conv1.weight" in src
    for order, prefix in (("rgb", ""), ("bgr", ""), ("bgr", "module.")):
        net = _model(arch)
        before = _bits(net)
        sd = FR.tv_state_dict(arch, 1, prefix)
        loaded = FT.load_image_trunk(net, sd, order) if prefix else net.load_image_trunk(sd, order)
        assert not [k for k in loaded if k.startswith("fc.")]
        after = net.state_dict()
        seen = 0
        for k, v in after.items():
            if not k.startswith(FR.PFX):
                assert _same(v, before[k]), k                             # LiDAR, FPN, fusion: their bits
                continue
            want = src[k[len(FR.PFX):]]
            if k == FR.PFX + "conv1.weight" and order == "bgr":
                want = want[:, [2, 1, 0]]
            assert _same(v.detach(), want.to(v.dtype)), (k, order)
            assert not _same(v.detach(), before[k]) or v.numel() == 0
            seen += 1
        assert seen == len([k for k in src if not k.startswith("fc.")])
        assert int(after[FR.PFX + "bn1.num_batches_tracked"]) == 8 and _same(after[FR.PFX + "bn1.running_var"], src["bn1.running_var"])
        # the flat arena holds the stem in its padded physical layout: the padding stays zero
        off = [e for e in net._table.entries if e[0] == FR.PFX + "conv1.weight"][0]
        phys = net.flat_params[off[2]:off[2] + off[3]].view(off[1][0], 7, 8, 4)
        assert not phys[:, :, 7].any() and not phys[..., 3].any()
    # without num_batches_tracked: optional
    net = _model(arch)
    sd = {k: v for k, v in FR.tv_state_dict(arch, 1).items() if not k.endswith("num_batches_tracked")}
    FT.load_image_trunk(net, sd, "rgb")
    assert int(net.state_dict()[FR.PFX + "bn1.num_batches_tracked"]) == 0


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_import_refusals_write_nothing(arch):
    FT = pkg("finetune")
    net = _model(arch)
    before = _bits(net)
    good = FR.tv_state_dict(arch, 2)
    missing = {k: v for k, v in good.items() if k != "layer3.0.bn2.bias"}
    nobuf = {k: v for k, v in good.items() if k != "layer2.0.downsample.1.running_mean"}
    wrong = dict(good, **{"layer2.0.conv1.weight": torch.zeros(3, 3, 3, 3)})
    other = FR.tv_state_dict("resnet50" if arch == "resnet18" else "resnet18", 2)
    for bad, word in ((missing, "layer3.0.bn2.bias"), (nobuf, "layer2.0.downsample.1.running_mean"), (wrong, "layer2.0.conv1.weight"), (other, "layer1.0")):
        with pytest.raises(ValueError) as e:
            FT.load_image_trunk(net, bad, "bgr")
        assert word in str(e.value)
        for k, v in net.state_dict().items():
            assert _same(v, before[k]), k
    with pytest.raises(ValueError):
        FT.load_image_trunk(net, good, "gbr")
    with pytest.raises(ValueError):
        FT.load_image_trunk(net, [1, 2], "rgb")
    with pytest.raises(ValueError):
        FT.load_image_trunk_file(net, "/nonexistent/trunk.pth", "bgr")
    M = pkg("model")
    with pytest.raises((ValueError, NotImplementedError)):                # an unknown arch never gets as far as a model
        M.ObjectDetection_DCF(_cfg("resnet19"))
    lidar_only = golden_cfg(load_golden("model_tiny.npz"))
    with pytest.raises(ValueError):
        FT.load_image_trunk(M.ObjectDetection_DCF(lidar_only), good, "rgb")
    for k, v in net.state_dict().items():
        assert _same(v, before[k]), k


# ---------------------------------------------------------------------------------------------------------------- param_groups
KEYS = ["lidar_backbone.conv3.weight", "image_backbone.conv1.weight", "image_backbone.bn1.weight", "image_backbone.bn1.bias",
        "image_backbone.layer1.0.conv1.weight", "image_backbone.layer1.0.bn1.weight", "image_backbone.layer2.0.conv1.weight",
        "image_backbone.layer3.0.conv1.weight", "image_backbone.layer4.0.conv1.weight", "image_fpn.lat1.weight", "fusion.site1.fc2.bias"]


def test_parse_param_groups_refusals():
    O = pkg("optim")
    assert O.parse_param_groups(None) is None and O.parse_param_groups([]) is None
    ok = O.parse_param_groups([{"match": ["image_backbone.conv1", "image_backbone.bn1", "image_backbone.layer1."], "frozen": True},
                               {"match": ["image_backbone."], "lr_mult": 0.1}], KEYS)
    assert ok == [{"match": ("image_backbone.conv1", "image_backbone.bn1", "image_backbone.layer1."), "lr_mult": 1.0, "frozen": True},
                  {"match": ("image_backbone.",), "lr_mult": 0.1, "frozen": False}]
    assert O.parse_param_groups([{"match": ["x"], "lr_mult": 0}])[0]["lr_mult"] == 0.0
    assert len(O.parse_param_groups([{"match": ["a%d" % i]} for i in range(15)])) == 15
    bad = [{"match": ["a"]}, [{"match": ["a%d" % i]} for i in range(16)], ["image_backbone."], [{"lr_mult": 0.1}], [{"match": []}],
           [{"match": "image_backbone."}], [{"match": [""]}], [{"match": [3]}], [{"match": ["a"], "lr_mult": -0.1}],
           [{"match": ["a"], "lr_mult": float("nan")}], [{"match": ["a"], "lr_mult": float("inf")}], [{"match": ["a"], "lr_mult": "0.1"}],
           [{"match": ["a"], "lr_mult": True}], [{"match": ["a"], "frozen": 1}], [{"match": ["a"], "frozen": True, "lr_mult": 0.5}],
           [{"match": ["a"], "frozen": True, "lr_mult": 1.0}], [{"match": ["a"], "weight_decay": 0.1}]]
    for blk in bad:
        with pytest.raises(ValueError):
            O.parse_param_groups(blk)
    with pytest.raises(ValueError):                                       # matches no parameter
        O.parse_param_groups([{"match": ["image_backbone.layer5."], "lr_mult": 0.1}], KEYS)
    with pytest.raises(ValueError):                                       # ... because an earlier group wins all of its parameters
        O.parse_param_groups([{"match": ["image_backbone."], "lr_mult": 0.1}, {"match": ["image_backbone.layer1."], "frozen": True}], KEYS)


def test_group_ids_on_a_hand_made_table():
    O = pkg("optim")
    groups = O.parse_param_groups([{"match": ["stem", "first."], "frozen": True}, {"match": ["first.", "trunk."], "lr_mult": 0.1}, {"match": ["head"], "lr_mult": 3}])
    # (key, logical shape, offset, physical numel, layout): a padded stem, a 5-element tensor (its tail group), an unmatched one, ...
    entries = [("stem.weight", (2, 3, 7, 7), 0, 2 * 7 * 8 * 4, "stem"), ("first.bn.weight", (5,), 448, 5, "plain"), ("other.weight", (6,), 456, 6, "plain"),
               ("trunk.first.weight", (4, 1, 1, 1), 464, 4, "ohwi"), ("head.bias", (3,), 468, 3, "plain")]
    n = 471
    ids = O.group_ids(entries, n, groups)
    assert ids.dtype == np.uint8 and ids.shape == ((n + 3) // 4,)
    want = np.zeros(118, dtype=np.uint8)
    want[0:112] = 1                                                       # the stem's whole physical extent
    want[112:114] = 1                                                     # 5 elements: two float4 groups, the padding behind them included
    want[116:117] = 1                                                     # first match wins: "first." of group 1, not group 2's
    want[117:118] = 3                                                     # the ragged tail group of the arena
    assert np.array_equal(ids, want)
    assert not O.group_ids(entries, n, None).any()
    with pytest.raises(ValueError):                                       # ParamTable's 16-byte alignment is asserted
        O.group_ids([("a.weight", (3,), 2, 3, "plain")], 8, groups)
    with pytest.raises(ValueError):
        O.group_ids([("a.weight", (9,), 0, 9, "plain")], 8, groups)


def test_decay_mul_per_group_against_float64():
    O = pkg("optim")
    groups = O.parse_param_groups([{"match": ["a"], "frozen": True}, {"match": ["b"], "lr_mult": 0.1}, {"match": ["c"], "lr_mult": 3.0}, {"match": ["d"], "lr_mult": 0.0}])
    for lr, wd in ((1e-3, 0.01), (0.0123, 0.5), (2.5e-4, 0.0), (1.0, 1.0)):
        tab = O.group_table(groups, lr, wd)
        assert [t[2] for t in tab] == [False, True, False, False, False]
        assert [t[0] for t in tab] == [1.0, 0.0, 0.1, 3.0, 0.0]
        for (mu, dm, fz) in tab:
            want = 1.0 - lr * mu * wd
            assert dm == float(F(want)) and abs(dm - want) <= 2.0 ** -24
        assert tab[0][1] == float(F(1.0 - lr * wd))                       # group 0: today's single decay_mul
        assert O.group_rates(groups, lr) == [lr, 0.0, lr * 0.1, lr * 3.0, 0.0]
    assert O.group_table(None, 1e-3, 0.01) == [(1.0, float(F(1.0 - 1e-5)), False)]


def test_trunk_prefix_derivation():
    O = pkg("optim")
    P = lambda blk: O.parse_param_groups(blk)
    stem = ["image_backbone.conv1", "image_backbone.bn1"]
    assert O.frozen_trunk_units(KEYS, None) == 0
    assert O.frozen_trunk_units(KEYS, P([{"match": ["image_backbone."], "lr_mult": 0.1}])) == 0
    assert O.frozen_trunk_units(KEYS, P([{"match": stem, "frozen": True}])) == 1
    assert O.frozen_trunk_units(KEYS, P([{"match": stem + ["image_backbone.layer1."], "frozen": True}, {"match": ["image_backbone."], "lr_mult": 0.1}])) == 2
    assert O.frozen_trunk_units(KEYS, P([{"match": ["image_backbone.layer1."], "frozen": True}])) == 0          # the stem is live
    assert O.frozen_trunk_units(KEYS, P([{"match": ["image_backbone."], "frozen": True}])) == 5
    assert O.frozen_trunk_units(KEYS, P([{"match": ["image_"], "frozen": True}])) == 5                            # (+ the FPN: optimiser only)
    assert O.frozen_trunk_units(KEYS, P([{"match": ["image_backbone.conv1", "image_backbone.layer1."], "frozen": True}])) == 0   # bn1 is live
    assert O.frozen_trunk_units(KEYS, P([{"match": stem + ["image_backbone.layer2."], "frozen": True}])) == 1    # layer1 live: the prefix ends
    assert O.frozen_trunk_units(KEYS, P([{"match": ["image_backbone.bn1.bias"], "lr_mult": 0.5}, {"match": ["image_backbone."], "frozen": True}])) == 0
    assert O.frozen_trunk_units([k for k in KEYS if not k.startswith("image_")], P([{"match": ["lidar"], "frozen": True}])) == 0
    # on a real model's keys, both archs: the prefix is one run of layer rows and one arena range
    for arch in ("resnet18", "resnet50"):
        net = _model(arch)
        keys = [e[0] for e in net._table.entries]
        for n_units, extra in ((1, []), (2, ["image_backbone.layer1."]), (4, ["image_backbone.layer%d." % i for i in (1, 2, 3)]),
                               (5, ["image_backbone.layer%d." % i for i in (1, 2, 3, 4)])):
            groups = O.parse_param_groups([{"match": stem + extra, "frozen": True}], keys)
            assert O.frozen_trunk_units(keys, groups) == n_units
            rng = net.set_frozen_trunk(n_units)
            frozen_keys = [e for e in net._table.entries if O.group_of(e[0], groups)]
            assert rng[0] == min(e[2] for e in frozen_keys) and rng[1] == max(e[2] + (e[3] + 3) // 4 * 4 for e in frozen_keys)
            inside = [e[0] for e in net._table.entries if rng[0] <= e[2] < rng[1]]
            assert inside == [e[0] for e in frozen_keys]
        assert net.set_frozen_trunk(0) is None and net._plan.img_frozen == 0
    with pytest.raises(ValueError):                                       # a frozen BatchNorm that follows batch statistics is not built
        net = pkg("model").ObjectDetection_DCF(dict(_cfg(), bn_mode="train"))
        net.set_frozen_trunk(1)


def test_flat_adam_objects_without_the_keys():
    """All keys absent: no group table, no id array, the plan's defaults."""
    T = pkg("train")

    class Stub(object):
        flat_params = torch.zeros(8)
        flat_grads = torch.zeros(8)
    opt = T.FlatAdam(Stub(), 1e-3)
    assert opt.groups is None and opt.group_ids is None and opt.group_rates(0) == [1e-3]

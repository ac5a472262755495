"""Reference helpers of the fine-tuning tests (test infrastructure; CPU only): synthesised torchvision-layout trunks, the grouped
optimiser statement built from _optim_ref.adam_ref, and the torch-CPU restatement of the camera stream behind the input
normalisation (the body of oracle/model_ref.image_stream with another first line)."""
import numpy as np
import torch
import torch.nn.functional as TF

import _optim_ref as R
from oracle import model_ref

F = np.float32
PFX = "image_backbone."
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # RGB order (public ImageNet statistics)
# identity; ImageNet in RGB and in BGR plane order; the [-1, 1] table; a hostile one (a negative mean, a tiny mean under a tiny std) for
# the bit-for-bit kernel test only
NORM_TABLES = (((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (IMAGENET_MEAN, IMAGENET_STD), ((0.406, 0.456, 0.485), (0.225, 0.224, 0.229)),
               ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((-0.25, 0.5, 1e-3), (3.0, 0.0625, 1e-2)))


# ---------------------------------------------------------------------------------------------------------------- torchvision layout
def tv_state_dict(arch, seed=0, prefix="", fc=True):
    """A state dict in torchvision's layout for `arch`, values from a seeded generator (nothing like detfill's, so a load shows):
    the keys of model_ref.image_state_shapes under image_backbone. with that prefix removed, plus fc.* (1000 classes)."""
    shapes = model_ref.image_state_shapes(64, arch=arch)
    rng = np.random.RandomState(4242 + seed)
    sd = {}
    for k, s in shapes.items():
        if not k.startswith(PFX):
            continue
        kk = prefix + k[len(PFX):]
        if k.endswith("num_batches_tracked"):
            sd[kk] = torch.tensor(7 + seed, dtype=torch.long)
        elif k.endswith("running_var") or (len(s) == 1 and k.endswith(".weight")):
            sd[kk] = torch.from_numpy(rng.uniform(0.5, 1.5, s).astype(F))
        elif len(s) == 1:
            sd[kk] = torch.from_numpy(rng.uniform(-0.2, 0.2, s).astype(F))
        else:
            b = 1.0 / np.sqrt(float(np.prod(s[1:])))
            sd[kk] = torch.from_numpy(rng.uniform(-b, b, s).astype(F))
    if fc:
        width = 2048 if arch == "resnet50" else 512
        sd[prefix + "fc.weight"] = torch.from_numpy(rng.uniform(-0.01, 0.01, (1000, width)).astype(F))
        sd[prefix + "fc.bias"] = torch.zeros(1000)
    return sd


# ---------------------------------------------------------------------------------------------------------------- normalisation
def norm_f64(s, mean, std):
    """((s / 255) - mean) / std in float64 from the fp32 table values (what the fp32 statement is measured against)."""
    return (np.float64(s) / 255.0 - np.float64(F(mean))) / np.float64(F(std))


def all_bytes_image(B, Hh, W, seed=0):
    """uint8 [B,3,H,W]; where H*W >= 256 every plane holds all 256 values (a shuffled ramp), else a ramp from a per-plane offset."""
    rng = np.random.RandomState(90 + seed)
    img = np.empty((B, 3, Hh, W), dtype=np.uint8)
    for b in range(B):
        for c in range(3):
            ramp = (np.arange(Hh * W) + 37 * c + 11 * b) % 256
            rng.shuffle(ramp)
            img[b, c] = ramp.reshape(Hh, W).astype(np.uint8)
    return img


# ---------------------------------------------------------------------------------------------------------------- the grouped step
def element_ids(ids, n):
    """Per-element group id from the per-float4 ids."""
    return np.repeat(np.asarray(ids, dtype=np.uint8), 4)[:n]


def adam_groups_ref(p, g, m, v, e, ids, table, lr_over_bc1, inv_sqrt_bc2, gscale, b1, b2, eps, dec=None, omd=0.0):
    """The statement of dcf_adamw_ema_step_groups: _optim_ref.adam_ref per group on the elements of that group, at
    fl(lr_over_bc1 * mu_g) with decay_mul_g; a frozen group's elements keep their bits (its gradient is never looked at).
    table: [(mu, decay_mul, frozen)] per id.  Returns (p', m', v', e' or None)."""
    n = len(p)
    el = element_ids(ids, n)
    p1, m1, v1 = (np.array(x, dtype=F, copy=True) for x in (p, m, v))
    e1 = None if e is None else np.array(e, dtype=F, copy=True)
    for gid, (mu, dm, frozen) in enumerate(table):
        sel = el == gid
        if frozen or not sel.any():
            continue
        lr = F(lr_over_bc1) * F(mu)
        out = R.adam_ref(p[sel], g[sel], m[sel], v[sel], lr, inv_sqrt_bc2, gscale, b1, b2, eps, dm, None if dec is None else dec[sel],
                         None if e is None else e[sel], omd)
        p1[sel], m1[sel], v1[sel] = out[0], out[1], out[2]
        if e is not None:
            e1[sel] = out[3]
    return p1, m1, v1, e1


BOUNDS = (100, 256, 1024, 2048)           # inside a wave, a wave boundary, a flat-shape workgroup, a stride-shape chunk (elements)


def segment_ids(n, k):
    """uint8[ceil(n/4)]: the arena cut at BOUNDS (and every 4096 elements from 4096 on), segment s in group s % k."""
    groups = (n + 3) // 4
    bounds = np.array(sorted(set(BOUNDS) | set(range(4096, max(n, 4097), 4096))), dtype=np.int64)
    seg = np.searchsorted(bounds, 4 * np.arange(groups, dtype=np.int64), side="right")
    return (seg % k).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the camera stream
def image_stream_norm(sd, img_u8, mean_rgb, std_rgb, input_order, bn_mode="eval", pfx="image_backbone", fpn="image_fpn"):
    """oracle/model_ref.image_stream with the first line replaced: the dataset's planes are put in RGB order (input_order names the
    colour of plane 0), x = (img / 255 - mean) / std per RGB plane, then the same trunk and FPN.  sd holds the SOURCE (RGB) conv1."""
    x = img_u8.to(torch.float32)
    if input_order == "bgr":
        x = x.flip(1)
    mean = torch.tensor(mean_rgb, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(std_rgb, dtype=torch.float32).view(1, 3, 1, 1)
    x = (x / 255.0 - mean) / std
    _bn = model_ref._bn
    x = TF.relu(_bn(sd, pfx + ".bn1", TF.conv2d(x, sd[pfx + ".conv1.weight"], None, 2, 3), bn_mode))
    x = TF.max_pool2d(x, 3, 2, 1)
    feats = []
    for li in range(1, 5):
        bi = 0
        while ("%s.layer%d.%d.conv1.weight" % (pfx, li, bi)) in sd:
            p = "%s.layer%d.%d" % (pfx, li, bi)
            s = 2 if (p + ".downsample.0.weight") in sd and li > 1 else 1
            r = _bn(sd, p + ".downsample.1", TF.conv2d(x, sd[p + ".downsample.0.weight"], None, s), bn_mode) if (p + ".downsample.0.weight") in sd else x
            if (p + ".conv3.weight") in sd:
                y = TF.relu(_bn(sd, p + ".bn1", TF.conv2d(x, sd[p + ".conv1.weight"], None, 1, 0), bn_mode))
                y = TF.relu(_bn(sd, p + ".bn2", TF.conv2d(y, sd[p + ".conv2.weight"], None, s, 1), bn_mode))
                y = _bn(sd, p + ".bn3", TF.conv2d(y, sd[p + ".conv3.weight"], None, 1, 0), bn_mode)
            else:
                y = TF.relu(_bn(sd, p + ".bn1", TF.conv2d(x, sd[p + ".conv1.weight"], None, s, 1), bn_mode))
                y = _bn(sd, p + ".bn2", TF.conv2d(y, sd[p + ".conv2.weight"], None, 1, 1), bn_mode)
            x = TF.relu(y + r)
            bi += 1
        feats.append(x)
    c2, c3, c4, c5 = feats
    p5 = TF.conv2d(c5, sd[fpn + ".lat4.weight"])
    p4 = TF.conv2d(c4, sd[fpn + ".lat3.weight"]) + TF.interpolate(p5, size=c4.shape[-2:], mode="bilinear", align_corners=False)
    p3 = TF.conv2d(c3, sd[fpn + ".lat2.weight"]) + TF.interpolate(p4, size=c3.shape[-2:], mode="bilinear", align_corners=False)
    p2 = TF.conv2d(c2, sd[fpn + ".lat1.weight"]) + TF.interpolate(p3, size=c2.shape[-2:], mode="bilinear", align_corners=False)
    return TF.conv2d(p2, sd[fpn + ".smooth.weight"], None, 1, 1)

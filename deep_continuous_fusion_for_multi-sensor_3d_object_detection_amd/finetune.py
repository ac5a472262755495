"""Fine-tuning the camera stream: the host statement of the input normalisation and the import of a
torchvision-layout ResNet trunk.

Plain numpy / torch host code; nothing here imports torchvision or reads the device.  The normalisation kernel
(csrc/elementwise.hip, dcf_image_to_nhwc4_norm) is pinned to normalize_image bit for bit; the parameter groups that go with a loaded
trunk are optim.parse_param_groups / optim.group_ids.
"""
import numpy as np
import torch

from . import cfgcheck as C

NORM_KEYS = ("mean", "std")
INPUT_ORDERS = ("rgb", "bgr")
TRUNK = "image_backbone."


def parse_image_norm(blk):
    """The `fusion.image_norm` block, validated: None (absent) or (mean float32[3], std float32[3]) in the order of the image planes
    the dataset delivers.  Unknown keys, wrong lengths, a non-finite mean and a std that is not finite and > 0 raise ValueError."""
    if blk is None:
        return None
    C.block("fusion.image_norm", blk, NORM_KEYS)
    out = []
    for key in NORM_KEYS:
        v = blk.get(key, None)
        if not isinstance(v, (list, tuple)) or len(v) != 3:
            raise ValueError("fusion.image_norm.%s must be a list of three numbers (got %r)" % (key, v))
        a = np.asarray([C.number("fusion.image_norm." + key, x) for x in v], dtype=np.float32)
        if not np.isfinite(a).all() or (key == "std" and not (a > 0).all()):
            raise ValueError("fusion.image_norm.%s: %s (got %r)" % (key, "must be greater than 0 in fp32" if key == "std" else "overflows fp32", v))
        out.append(a)
    return out[0], out[1]


def normalize_image(img_u8, mean, std):
    """The statement of dcf_image_to_nhwc4_norm: uint8 [..., 3, H, W] -> float32 of the same shape,
        v_c = fl(fl(fl((float)s / 255) - mean_c) / std_c)
    per plane c of the input's own order: three correctly rounded fp32 operations (numpy float32 array arithmetic rounds each once)."""
    x = np.asarray(img_u8)
    if x.dtype != np.uint8 or x.ndim < 3 or x.shape[-3] != 3:
        raise ValueError("normalize_image: a uint8 array [..., 3, H, W] (got %s %s)" % (x.dtype, x.shape))
    mean = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    std = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    v = ((x.astype(np.float32) / np.float32(255.0)) - mean) / std
    assert v.dtype == np.float32
    return v


def image_to_nhwc4_ref(img_u8, mean, std):
    """normalize_image in the kernel's output layout: float32 [B, H+6, W+8, 4], a 3-pixel halo of +0, channel 3 = +0."""
    v = normalize_image(img_u8, mean, std)
    B, _, Hh, W = v.shape
    y = np.zeros((B, Hh + 6, W + 8, 4), dtype=np.float32)
    y[:, 3:3 + Hh, 3:3 + W, :3] = v.transpose(0, 2, 3, 1)
    return y


def trunk_keys(model):
    """{torchvision key: (model key, shape, required)} of the model's camera trunk: every parameter and BatchNorm buffer under
    `image_backbone.`; num_batches_tracked is optional."""
    t = model._table
    out = {}
    for key, shape, off, n, layout in t.entries:
        if key.startswith(TRUNK):
            out[key[len(TRUNK):]] = (key, tuple(shape), True)
    for key, shape, off, n in t.buffers:
        if key.startswith(TRUNK):
            out[key[len(TRUNK):]] = (key, tuple(shape), not key.endswith("num_batches_tracked"))
    return out


def load_image_trunk(model, state_dict, input_order="rgb"):
    """Load a torchvision-layout ResNet state dict (`conv1.weight`, `bn1.*`, `layerL.B.*` with `downsample.0/1.*`; an optional
    `module.` prefix; `fc.*` ignored) into the model's camera trunk (`image_backbone.<key>`), on host memory or on the device.
    input_order names the colour of the DATASET's plane 0: the source weights are RGB, and with "bgr" conv1.weight's input channels
    are reversed on load, so that the model sees the planes the weights were trained on.  Every trunk parameter and BatchNorm buffer of
    the model's arch must be present with the right shape (num_batches_tracked is optional); otherwise ValueError names the keys and
    NOTHING is written.  Everything outside the trunk keeps its bits.  Returns the sorted list of the torchvision keys loaded."""
    if input_order not in INPUT_ORDERS:
        raise ValueError("input_order must be one of %s (got %r)" % (list(INPUT_ORDERS), input_order))
    want = trunk_keys(model)
    if not want:
        raise ValueError("the model has no camera trunk (fusion.enabled is off)")
    if not hasattr(state_dict, "items"):
        raise ValueError("load_image_trunk needs a state dict (got %r)" % (type(state_dict),))
    src = {}
    for k, v in state_dict.items():
        k = k[7:] if k.startswith("module.") else k
        if k.startswith("fc."):
            continue
        src[k] = v
    missing = sorted(k for k, (_, _, req) in want.items() if req and k not in src)
    unknown = sorted(k for k in src if k not in want)
    wrong = sorted("%s %s (model: %s)" % (k, tuple(src[k].shape), want[k][1]) for k in src
                   if k in want and (not torch.is_tensor(src[k]) or tuple(src[k].shape) != want[k][1]))
    if missing or unknown or wrong:
        raise ValueError("load_image_trunk: the state dict does not fit the model's camera trunk -- missing %s; not of this arch %s; "
                         "wrong shape %s" % (missing, unknown, wrong))
    own = dict(model.named_parameters())
    own.update(dict(model.named_buffers()))
    with torch.no_grad():
        for k in sorted(src):
            v = src[k].detach()
            if k == "conv1.weight" and input_order == "bgr":
                v = v.flip(1)
            dst = own[want[k][0]]
            dst.copy_(v.to(device=dst.device, dtype=dst.dtype))
    return sorted(src)                        # (the weight images are re-folded from the arena every step: nothing else to refresh)


def load_image_trunk_file(model, path, input_order="bgr"):
    """`fusion.image_pretrained`: load_image_trunk from a torch.load-able file; an unreadable path raises ValueError."""
    try:
        sd = torch.load(path, map_location="cpu")
    except Exception as e:
        raise ValueError("fusion.image_pretrained: cannot read %r (%s)" % (path, e))
    if isinstance(sd, dict) and "state_dict" in sd and hasattr(sd["state_dict"], "items"):
        sd = sd["state_dict"]
    return load_image_trunk(model, sd, input_order)

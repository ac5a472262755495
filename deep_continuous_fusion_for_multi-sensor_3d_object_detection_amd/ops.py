"""Operator layer: one Python function per C-ABI entry point of libdcf_hip.so.

Each function takes torch CUDA tensors (NHWC activations, compute dtype f32 or bf16),
allocates the output with torch (device memory = plumbing) and enqueues the HIP kernel on
torch's current stream.  No arithmetic happens in torch here.
"""
import ctypes

import numpy as np
import torch

from . import _hip as H


def _chk(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
        raise H.DcfError("%s must be a contiguous CUDA tensor" % name)
    return t


def conv_out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ------------------------------------------------------------------ layout
def nchw_to_nhwc(x, dtype):
    B, C, Hh, W = x.shape
    _chk(x, "x")
    y = torch.empty((B, Hh, W, C), dtype=H.torch_dtype(dtype), device=x.device)
    H.call("dcf_nchw_to_nhwc", dtype, x, y, B, C, Hh, W, H.stream_ptr())
    return y


def nhwc_to_nchw(x, dtype):
    """NHWC tensor of the compute dtype -> NCHW fp32 (the reference's activation layout)."""
    B, Hh, W, C = x.shape
    _chk(x, "x")
    y = torch.empty((B, C, Hh, W), dtype=torch.float32, device=x.device)
    H.call("dcf_nhwc_to_nchw", dtype, x, y, B, C, Hh, W, H.stream_ptr())
    return y


def image_to_nhwc4(img_u8, dtype):
    B, C, Hh, W = img_u8.shape
    assert C == 3 and img_u8.dtype == torch.uint8
    _chk(img_u8, "image")
    y = torch.empty((B, Hh + 6, W + 8, 4), dtype=H.torch_dtype(dtype), device=img_u8.device)
    H.call("dcf_image_to_nhwc4", dtype, img_u8, y, B, Hh, W, H.stream_ptr())
    return y


def image_to_nhwc4_norm(img_u8, dtype, mean, std, out=None):
    """dcf_image_to_nhwc4_norm: image_to_nhwc4 with ((x / 255) - mean[c]) / std[c] per plane c of the image's own order (three
    rounded fp32 operations, finetune.normalize_image is the statement); mean, std: three host floats each."""
    B, C, Hh, W = img_u8.shape
    assert C == 3 and img_u8.dtype == torch.uint8
    _chk(img_u8, "image")
    mean, std = H.host_f32(mean).reshape(-1), H.host_f32(std).reshape(-1)
    if mean.size != 3 or std.size != 3:
        raise ValueError("image_to_nhwc4_norm: mean and std hold three values each (got %d, %d)" % (mean.size, std.size))
    y = torch.empty((B, Hh + 6, W + 8, 4), dtype=H.torch_dtype(dtype), device=img_u8.device) if out is None else out
    H.call("dcf_image_to_nhwc4_norm", dtype, img_u8, y, B, Hh, W, mean, std, H.stream_ptr())
    return y


# ------------------------------------------------------------------ convolution
def conv2d_fwd(dtype, x, w, shift, res, kh, kw, stride, pad, relu, cout):
    B, Hh, W, Cin = x.shape
    Ho, Wo = conv_out_size(Hh, kh, stride, pad), conv_out_size(W, kw, stride, pad)
    y = torch.empty((B, Ho, Wo, cout), dtype=x.dtype, device=x.device)
    H.call("dcf_conv2d_fwd", dtype, x, w, shift, res, y, B, Hh, W, Cin, Ho, Wo, cout, kh, kw, stride, pad, int(relu),
           H.stream_ptr())
    return y


def conv2d_fwd_rowscale(dtype, x, w, shift, rowscale, res, relu, cout):
    """1x1 conv2d_fwd whose shift is scaled per output pixel: y = act(conv + rowscale[m] * shift[c] + res); rowscale fp32 [B*H*W]."""
    B, Hh, W, Cin = x.shape
    if rowscale.numel() != B * Hh * W or rowscale.dtype != torch.float32:
        raise H.DcfError("conv2d_fwd_rowscale: rowscale must be fp32 with one entry per output pixel")
    y = torch.empty((B, Hh, W, cout), dtype=x.dtype, device=x.device)
    H.call("dcf_conv2d_fwd_rowscale", dtype, x, w, shift, _chk(rowscale, "rowscale"), res, y, B, Hh, W, Cin, Hh, W, cout, 1, 1, 1, 0, int(relu),
           H.stream_ptr())
    return y


def fp8_act_scale(amax):
    """The activation scale rule of the fp8 path (largest power of two s with amax*s <= 224)."""
    import ctypes
    out = ctypes.c_float(0.0)
    H.call("dcf_fp8_act_scale", float(amax), ctypes.addressof(out))
    return float(out.value)


def cast_fp8(dtype, x, amax_prev=None, amax_cur=None):
    """uint8 image (OCP e4m3 bits) of x * scale(amax_prev); amax_cur (device float[64]) collects partial maxima of |x|."""
    x8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    H.call("dcf_cast_fp8", dtype, x, x8, amax_prev, amax_cur, x.numel(), H.stream_ptr())
    return x8


def conv2d_fwd_fp8(out_dtype, x8, w8, wscale, xamax, shift, res, kh, kw, stride, pad, relu, cout, want_y8=False, y8amax=None, y8cur=None):
    """want_y8: also return the fp8 image of y (scale from y8amax, partial maxima into y8cur[64]) -> (y, y8)."""
    B, Hh, W, Cin = x8.shape
    Ho, Wo = conv_out_size(Hh, kh, stride, pad), conv_out_size(W, kw, stride, pad)
    y = torch.empty((B, Ho, Wo, cout), dtype=H.torch_dtype(out_dtype), device=x8.device)
    y8 = torch.empty((B, Ho, Wo, cout), dtype=torch.uint8, device=x8.device) if want_y8 else None
    H.call("dcf_conv2d_fwd_fp8", out_dtype, x8, w8, wscale, xamax, shift, res, y, y8, y8amax, y8cur, B, Hh, W, Cin, Ho, Wo, cout, kh, kw,
           stride, pad, int(relu), H.stream_ptr())
    return (y, y8) if want_y8 else y


def conv2d_dgrad(dtype, gy, wt, res, in_shape, kh, kw, stride, pad, mask=None):
    B, Hh, W, Cin = in_shape
    _, Ho, Wo, Cout = gy.shape
    gx = torch.empty((B, Hh, W, Cin), dtype=gy.dtype, device=gy.device)
    H.call("dcf_conv2d_dgrad", dtype, gy, wt, res, mask, gx, B, Hh, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, H.stream_ptr())
    return gx


def conv2d_dgrad_halfres(dtype, gy, wt, res, resq, in_shape, kh, kw, stride, pad, mask=None):
    """conv2d_dgrad of a stride-2 layer plus resq [B, ceil(H/2), ceil(W/2), Cin] added on the (2i, 2j) sub-grid of gx."""
    B, Hh, W, Cin = in_shape
    _, Ho, Wo, Cout = gy.shape
    if tuple(resq.shape) != (B, (Hh + 1) // 2, (W + 1) // 2, Cin):
        raise H.DcfError("conv2d_dgrad_halfres: resq %s does not sit on the even sub-grid of %s" % (tuple(resq.shape), tuple(in_shape)))
    gx = torch.empty((B, Hh, W, Cin), dtype=gy.dtype, device=gy.device)
    H.call("dcf_conv2d_dgrad_halfres", dtype, gy, wt, res, resq, mask, gx, B, Hh, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, H.stream_ptr())
    return gx


def conv3x3_chain_supported(dtype, B, Hh, W, C, nlayers):
    """Can dcf_conv3x3_chain run `nlayers` 3x3 / stride-1 layers of C channels on [B,Hh,W,C] in one launch?"""
    return bool(H.lib().dcf_conv3x3_chain_supported(dtype, B, Hh, W, C, nlayers))


def conv3x3_chain_workspace(dtype, B, Hh, W, C, nlayers, device):
    """Arrival counters of a chain launch, zeroed ONCE here (every launch leaves them zero); int32 tensor."""
    n = H.lib().dcf_conv3x3_chain_workspace_bytes(dtype, B, Hh, W, C, nlayers)
    if n == 0:
        raise H.DcfError("conv3x3_chain: unsupported shape %s x %d layers" % ((B, Hh, W, C), nlayers))
    return torch.zeros((n // 4,), dtype=torch.int32, device=device)


def conv3x3_chain(dtype, x, layers, flip, ws, table=None):
    """A chain of 3x3 / stride-1 / pad-1 layers with C channels in and out, each reading the one before it, in ONE launch
    (dcf_hip.h: dcf_conv3x3_chain).  x [B,H,W,C]; layers = list of (w, shift, res, mask, relu) where w / shift are tensors or
    raw device addresses and res / mask are tensors, None, or an int k = "the output of chain layer k" (k <= l - 2).
    flip = 1: input gradients (w = the [Cin][tap][Cout] images).  Returns the list of outputs (new tensors).
    table: a ctypes (H.ChainLayer * n) to reuse between calls (the caller keeps it alive)."""
    B, Hh, W, C = x.shape
    n = len(layers)
    outs = [torch.empty((B, Hh, W, C), dtype=x.dtype, device=x.device) for _ in range(n)]
    tab = table if table is not None else (H.ChainLayer * n)()
    cur = x.data_ptr()
    for l, (w, shift, res, mask, relu) in enumerate(layers):
        it = tab[l]
        it.x = cur
        it.w = H._ptr(w)
        it.shift = H._ptr(shift)
        it.res = outs[res].data_ptr() if type(res) is int else H._ptr(res)
        it.mask = outs[mask].data_ptr() if type(mask) is int else H._ptr(mask)
        cur = it.y = outs[l].data_ptr()
        it.relu = 1 if relu else 0
    import ctypes
    H.call("dcf_conv3x3_chain", dtype, ctypes.addressof(tab), n, B, Hh, W, C, int(flip), ws, H.stream_ptr())
    return outs


def conv3x3_chain_status(ws):
    """The give-up record of the last chain launches on workspace ws (0 = every wait was satisfied); synchronises."""
    return int(ws[1].item())


def conv2d_wgrad_splits(B, Ho, Wo, Cin, Cout, kh, kw, stride=1):
    return H.lib().dcf_conv2d_wgrad_splits(B, Ho, Wo, Cin, Cout, kh, kw, stride)


def conv2d_wgrad(dtype, x, gy, slabs, nsplit, kh, kw, stride, pad, gsum=None):
    B, Hh, W, Cin = x.shape
    _, Ho, Wo, Cout = gy.shape
    H.call("dcf_conv2d_wgrad", dtype, x, gy, slabs, gsum, nsplit, B, Hh, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, H.stream_ptr())
    return slabs


def stem7x7_fwd(dtype, img4, w, shift, relu, cout, Hh, W):
    B = img4.shape[0]
    Ho, Wo = conv_out_size(Hh, 7, 2, 3), conv_out_size(W, 7, 2, 3)
    y = torch.empty((B, Ho, Wo, cout), dtype=img4.dtype, device=img4.device)
    H.call("dcf_stem7x7_fwd", dtype, img4, w, shift, y, B, Hh, W, Ho, Wo, cout, int(relu), H.stream_ptr())
    return y


def stem7x7_wgrad(dtype, img4, gy, slabs, nsplit, Hh, W, gsum=None):
    B, Ho, Wo, Cout = gy.shape
    H.call("dcf_stem7x7_wgrad", dtype, img4, gy, slabs, gsum, nsplit, B, Hh, W, Ho, Wo, Cout, H.stream_ptr())
    return slabs


# ------------------------------------------------------------------ elementwise
def relu_bwd_chansum(dtype, gy, y, gsum, relu=True):
    C = gy.shape[-1]
    npix = gy.numel() // C
    H.call("dcf_relu_bwd_chansum", dtype, gy, y if relu else None, gsum, npix, C, int(relu), H.stream_ptr())
    return gy


def bn_workspace(C, device):
    return torch.empty((H.lib().dcf_bn_workspace_bytes(C),), dtype=torch.uint8, device=device)


def bn_train_fwd(dtype, x, gamma, beta, res, running_mean, running_var, relu, ws, eps=1e-5, momentum=0.1):
    """Returns (y, mean, invstd); running stats are updated in place when given."""
    C = x.shape[-1]
    npix = x.numel() // C
    y = torch.empty_like(x)
    mean = torch.empty((C,), dtype=torch.float32, device=x.device)
    invstd = torch.empty((C,), dtype=torch.float32, device=x.device)
    H.call("dcf_bn_train_fwd", dtype, x, gamma, beta, res, y, mean, invstd, running_mean, running_var, npix, C, eps, momentum,
           int(relu), ws, H.stream_ptr())
    return y, mean, invstd


def bn_train_bwd(dtype, g, x, mean, invstd, gamma, dgamma, dbeta, ws):
    C = x.shape[-1]
    dx = torch.empty_like(x)
    H.call("dcf_bn_train_bwd", dtype, g, x, mean, invstd, gamma, dgamma, dbeta, dx, x.numel() // C, C, ws, H.stream_ptr())
    return dx


def resize_bilinear_fwd(dtype, x, out_hw, align_corners, add=None):
    B, Hi, Wi, C = x.shape
    Ho, Wo = out_hw
    y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    H.call("dcf_resize_bilinear_fwd", dtype, x, add, y, B, Hi, Wi, Ho, Wo, C, int(align_corners), H.stream_ptr())
    return y


def resize_bilinear_bwd(dtype, gy, in_hw, align_corners):
    B, Ho, Wo, C = gy.shape
    Hi, Wi = in_hw
    gx = torch.empty((B, Hi, Wi, C), dtype=gy.dtype, device=gy.device)
    H.call("dcf_resize_bilinear_bwd", dtype, gy, gx, B, Hi, Wi, Ho, Wo, C, int(align_corners), H.stream_ptr())
    return gx


def maxpool_fwd(dtype, x):
    B, Hh, W, C = x.shape
    Ho, Wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    H.call("dcf_maxpool3x3s2_fwd", dtype, x, y, B, Hh, W, Ho, Wo, C, H.stream_ptr())
    return y


def maxpool_fwd_idx(dtype, x):
    """(y, idx): pooled output and the arg-max positions (uint32 [B,Ho,Wo,C/4], one byte per channel)."""
    B, Hh, W, C = x.shape
    Ho, Wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, Ho, Wo, C // 4), dtype=torch.int32, device=x.device)
    H.call("dcf_maxpool3x3s2_fwd_idx", dtype, x, y, idx, B, Hh, W, Ho, Wo, C, H.stream_ptr())
    return y, idx


def maxpool_bwd_idx(dtype, idx, gy, in_shape):
    B, Hh, W, C = in_shape
    _, Ho, Wo, _ = gy.shape
    gx = torch.empty(in_shape, dtype=gy.dtype, device=gy.device)
    H.call("dcf_maxpool3x3s2_bwd_idx", dtype, idx, gy, gx, B, Hh, W, Ho, Wo, C, H.stream_ptr())
    return gx


def maxpool_bwd(dtype, x, y, gy):
    B, Hh, W, C = x.shape
    _, Ho, Wo, _ = gy.shape
    gx = torch.empty_like(x)
    H.call("dcf_maxpool3x3s2_bwd", dtype, x, y, gy, gx, B, Hh, W, Ho, Wo, C, H.stream_ptr())
    return gx


def head_fwd(dtype, head, anchors):
    B, h, w, Cp = head.shape
    pred = torch.empty((B, 32, h, w), dtype=torch.float32, device=head.device)
    H.call("dcf_head_fwd", dtype, head, Cp, anchors, pred, B, h, w, H.stream_ptr())
    return pred


def head_bwd(dtype, head, anchors, pred, gpred):
    B, h, w, Cp = head.shape
    ghead = torch.empty_like(head)
    H.call("dcf_head_bwd", dtype, head, Cp, anchors, pred, _chk(gpred, "gpred"), ghead, B, h, w, H.stream_ptr())
    return ghead


def cast(src, dtype_dst):
    dst = torch.empty(src.shape, dtype=H.torch_dtype(dtype_dst), device=src.device)
    H.call("dcf_cast", H.dtype_code(src.dtype), src, dtype_dst, dst, src.numel(), H.stream_ptr())
    return dst


def adam_step(params, grads, m, v, lr, beta1, beta2, eps, step, gscale=1.0):
    H.call("dcf_adam_step", params, grads, m, v, params.numel(), lr, beta1, beta2, eps, step, gscale, H.stream_ptr())


# ------------------------------------------------------------------ guarded optimiser step (csrc/amp.hip)
class AmpState(object):
    """struct dcf_amp_state in one fp32 device tensor (`raw`), with 0-d views of its fields.  The views alias the device
    memory: reading one with .item() synchronises, using one in a torch expression does not."""

    WORDS = ctypes.sizeof(H.AmpState) // 4

    def __init__(self, device, scale=1.0):
        self.raw = torch.zeros(self.WORDS, dtype=torch.float32, device=device)
        f = {name: getattr(H.AmpState, name).offset // 4 for name, _ in H.AmpState._fields_}
        r = self.raw
        self.scale_in, self.scale_next = r[f["scale_in"]], r[f["scale_next"]]
        self.growth_tracker = r[f["growth_tracker"]:f["growth_tracker"] + 1].view(torch.int32)[0]
        self.found_inf = r[f["found_inf"]:f["found_inf"] + 1].view(torch.int32)[0]
        self.applied_steps = r[f["applied_steps"]:f["applied_steps"] + 2].view(torch.int64)[0]
        self.skipped_steps = r[f["skipped_steps"]:f["skipped_steps"] + 2].view(torch.int64)[0]
        self.grad_norm, self.clip_coef = r[f["grad_norm"]], r[f["clip_coef"]]
        self.gscale, self.lr_over_bc1, self.inv_sqrt_bc2 = r[f["gscale"]], r[f["lr_over_bc1"]], r[f["inv_sqrt_bc2"]]
        self.header = r[:f["part_sum"]]              # everything but the partials workspace: what a checkpoint carries
        self.scale_in.fill_(scale)
        self.scale_next.fill_(scale)


def grad_stats(grads, state):
    H.call("dcf_grad_stats", grads, grads.numel(), state.raw, H.stream_ptr())


def amp_update(state, gscale_host, dynamic, growth_factor, backoff_factor, growth_interval, max_norm, lr, beta1, beta2):
    """max_norm None = no clipping."""
    H.call("dcf_amp_update", state.raw, gscale_host, 1 if dynamic else 0, growth_factor, backoff_factor, growth_interval,
           0.0 if max_norm is None else max_norm, lr, beta1, beta2, H.stream_ptr())


def adam_step_guarded(params, grads, m, v, beta1, beta2, eps, state):
    H.call("dcf_adam_step_guarded", params, grads, m, v, params.numel(), beta1, beta2, eps, state.raw, H.stream_ptr())


def adamw_ema_step(params, grads, m, v, lr, beta1, beta2, eps, step, gscale=1.0, decay_mul=1.0, decay_bits=None, ema=None, ema_omd=0.0,
                   state=None):
    """dcf_adamw_ema_step (csrc/optim.hip): the Adam step with decoupled weight decay (decay_mul = 1 - lr * weight_decay on the
    float4 groups whose bit is set in the uint64 device tensor decay_bits; None = all) and the weight average ema += ema_omd *
    (p' - ema) in the same pass.  state (AmpState): the guarded step -- lr, step and gscale then come from the device."""
    H.call("dcf_adamw_ema_step", params, grads, m, v, ema, decay_bits, params.numel(), lr, beta1, beta2, eps, step, gscale, decay_mul,
           ema_omd, None if state is None else state.raw, H.stream_ptr())


class AdamGroups(object):
    """The side table of dcf_adamw_ema_step_groups: `ids`, one uint8 per float4 group of the arena (optim.group_ids), checked on the
    host HERE -- an id of `count` or more is refused -- and uploaded once; `count` groups."""

    def __init__(self, ids, count, device):
        ids = np.ascontiguousarray(np.asarray(ids))
        if ids.dtype != np.uint8 or ids.ndim != 1:
            raise ValueError("AdamGroups: ids must be a one-dimensional uint8 array (got %s, %d-d)" % (ids.dtype, ids.ndim))
        count = int(count)
        if not 1 <= count <= H.ADAM_MAX_GROUPS:
            raise ValueError("AdamGroups: 1 to %d groups (got %d)" % (H.ADAM_MAX_GROUPS, count))
        if ids.size and int(ids.max()) >= count:
            raise ValueError("AdamGroups: group id %d with %d groups" % (int(ids.max()), count))
        self.count = count
        self.n_ids = int(ids.size)
        self.ids = torch.from_numpy(ids.copy()).to(device) if ids.size else torch.zeros(1, dtype=torch.uint8, device=device)
        self.table = (H.AdamGroup * count)()


def adamw_ema_step_groups(params, grads, m, v, lr, beta1, beta2, eps, step, groups, table, gscale=1.0, decay_bits=None, ema=None,
                          ema_omd=0.0, state=None):
    """dcf_adamw_ema_step_groups (csrc/optim.hip): adamw_ema_step with parameter groups.  groups: AdamGroups (the per-float4 ids);
    table: [(mu, decay_mul, frozen)] per group id, by value into the launch.  A frozen group's p, m, v, ema keep their bits and its
    gradient is not read; the others run at lr * mu with their own decay_mul."""
    n = params.numel()
    if len(table) != groups.count:
        raise ValueError("adamw_ema_step_groups: %d table rows for %d groups" % (len(table), groups.count))
    if groups.n_ids != (n + 3) // 4:
        raise ValueError("adamw_ema_step_groups: %d group ids for %d elements (one per float4 group)" % (groups.n_ids, n))
    for k, (mu, dm, fz) in enumerate(table):
        groups.table[k] = H.AdamGroup(float(mu), float(dm), 1 if fz else 0)
    if n == 0:                                             # (an empty tensor has no address to pass)
        return
    H.call("dcf_adamw_ema_step_groups", params, grads, m, v, ema, decay_bits, groups.ids, groups.count, ctypes.addressof(groups.table), n,
           lr, beta1, beta2, eps, step, gscale, ema_omd, None if state is None else state.raw, H.stream_ptr())


def grad_accumulate(dst, src, mode):
    """dcf_grad_accumulate (csrc/optim.hip): dst = src (mode 0) or dst += src (mode 1) over two contiguous fp32 device tensors of one
    size -- the gradient arena or a range of it; they must not overlap."""
    if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.numel() != src.numel():
        raise ValueError("grad_accumulate: two fp32 tensors of one size (got %s[%d], %s[%d])" % (dst.dtype, dst.numel(), src.dtype, src.numel()))
    if not (dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("grad_accumulate: dst and src must be contiguous")
    if dst.numel() == 0:                                   # (an empty tensor has no address to pass)
        return
    H.call("dcf_grad_accumulate", dst, src, dst.numel(), int(mode), H.stream_ptr())


# ------------------------------------------------------------------ geometry
class GridSpec(object):
    """Grid constants of CarlaDataset.__init__ (data_import_carla.py:35-43) and the filter
    thresholds of :215-226 -- host-side integer arithmetic only."""

    def __init__(self, cfg):
        L, W, Cz = cfg["voxel_length"], cfg["voxel_width"], cfg["voxel_channel"]
        self.dims = (Cz, L, W)
        self.xs = int(L / (cfg["lidar_x_max"] - cfg["lidar_x_min"]))
        self.ys = int(W / (cfg["lidar_y_max"] - cfg["lidar_y_min"]))
        self.zs = int(Cz / (cfg["lidar_z_max"] - cfg["lidar_z_min"]))
        self.xo = int(-cfg["lidar_x_min"] * self.xs)
        self.yo = int(-cfg["lidar_y_min"] * self.ys)
        self.zo = int(-cfg["lidar_z_min"] * self.zs)
        d = cfg["delta"]
        self.lim = np.array([cfg["lidar_x_min"], cfg["lidar_x_max"] - d, cfg["lidar_y_min"], cfg["lidar_y_max"] - d,
                             cfg["lidar_z_min"], cfg["lidar_z_max"] - d], dtype=np.float64).astype(np.float32)
        self.aff = np.array([self.xs, self.xo, self.ys, self.yo, self.zs, self.zo], dtype=np.float32)
        self.image_height = cfg["image_height"]
        self.image_width = cfg["image_width"]


def range_filter(pts, lim):
    n = pts.shape[0]
    dev = pts.device
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    src = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((H.lib().dcf_compact_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    H.call("dcf_range_filter", _chk(pts, "pts"), n, H.host_f32(lim), out, src, cnt, ws, H.stream_ptr())
    return out, src, cnt


def voxelize(pts, lim, aff, dims, mode=H.VOXEL_COMPAT, owner_ws=None, out=None):
    Cz, L, W = dims
    dev = pts.device
    grid = torch.empty((Cz, L, W), dtype=torch.float32, device=dev) if out is None else _chk(out, "out")
    if mode in (H.VOXEL_COMPAT, H.VOXEL_COMPAT_ROUNDS) and owner_ws is None:
        owner_ws = torch.zeros((2, Cz * L * W), dtype=torch.int32, device=dev)
    H.call("dcf_voxelize", _chk(pts, "pts"), pts.shape[0], H.host_f32(lim), H.host_f32(aff), Cz, L, W, mode, grid, owner_ws,
           H.stream_ptr())
    return grid


def voxelize_batch(pts_list, lim, aff, dims, owner_ws, out):
    """Compat-mode grids of B frames (claim / gather / release, one launch each for all frames): out [B,Cz,L,W] fp32,
    owner_ws int32 [B,2,Cz*L*W] (zero on entry and on exit)."""
    Cz, L, W = dims
    B = len(pts_list)
    ptrs = (ctypes.c_void_p * B)(*[_chk(p, "pts").data_ptr() for p in pts_list])
    ns = (ctypes.c_int * B)(*[p.shape[0] for p in pts_list])
    H.call("dcf_voxelize_batch", ctypes.addressof(ptrs), ctypes.addressof(ns), B, H.host_f32(lim), H.host_f32(aff), Cz, L, W, _chk(out, "out"),
           owner_ws, H.stream_ptr())
    return out


def voxelize_batch_nhwc(dtype, pts_list, lim, aff, dims, owner_ws, out):
    """The same grids as the engine's input image: out [B,L,W,Cz] in the compute dtype (= nchw_to_nhwc of voxelize_batch)."""
    Cz, L, W = dims
    B = len(pts_list)
    ptrs = (ctypes.c_void_p * B)(*[_chk(p, "pts").data_ptr() for p in pts_list])
    ns = (ctypes.c_int * B)(*[p.shape[0] for p in pts_list])
    H.call("dcf_voxelize_batch_nhwc", dtype, ctypes.addressof(ptrs), ctypes.addressof(ns), B, H.host_f32(lim), H.host_f32(aff), Cz, L, W,
           _chk(out, "out"), owner_ws, H.stream_ptr())
    return out


def project_filter(pts, lim, crt, ulim, vlim, mode=H.PROJ_COMPAT, n_out=None, want_src=False, out=None):
    """Returns (uv [n_out,2], xyz [n_out,3], count int32[1] (device), src or None); rows past count are zero.
    out: optional (uv, xyz, count) to write into -- zero-filled, contiguous, at least as many rows as input points (a
    batch's frames then land side by side in one tensor without a stack copy)."""
    n = pts.shape[0]
    dev = pts.device
    n_out = n if n_out is None else n_out
    if n_out < n:
        raise H.DcfError("project_filter: output rows (%d) < input points (%d)" % (n_out, n))
    if out is not None:
        uv, xyz, cnt = out
        if uv.shape[0] < n or xyz.shape[0] < n or not (uv.is_contiguous() and xyz.is_contiguous()):
            raise H.DcfError("project_filter: out tensors must be contiguous with at least %d rows" % n)
    else:
        uv = torch.zeros((max(n_out, 1), 2), dtype=torch.float32, device=dev)
        xyz = torch.zeros((max(n_out, 1), 3), dtype=torch.float32, device=dev)
        cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    src = torch.empty((max(n, 1),), dtype=torch.int32, device=dev) if want_src else None
    ws = torch.empty((H.lib().dcf_compact_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    H.call("dcf_project_filter", _chk(pts, "pts"), n, H.host_f32(lim), H.host_f32(crt).reshape(-1), float(ulim), float(vlim), mode,
           uv, xyz, src, cnt, ws, H.stream_ptr())
    return uv, xyz, cnt, src


def project_filter_batch(pts_list, lim, crts, ulim, vlim, mode, uv_all, xyz_all, cnt_all, ws=None):
    """dcf_project_filter for the (<= 8) frames of a batch in one launch per phase: pts_list = B device tensors [n_b,3]; crts [B,4,3]
    (or [B,12]) host floats, one matrix per frame; uv_all [B,rows,2], xyz_all [B,rows,3] (zero-filled by the caller: rows past a
    frame's count are left untouched), cnt_all int32 [B].  Same values as one project_filter per frame."""
    import ctypes
    B = len(pts_list)
    rows = xyz_all.shape[1]
    ns = [int(p.shape[0]) for p in pts_list]
    if max(ns) > rows or uv_all.shape[1] != rows or not (uv_all.is_contiguous() and xyz_all.is_contiguous() and cnt_all.is_contiguous()):
        raise H.DcfError("project_filter_batch: contiguous outputs with at least %d rows per frame" % max(ns))
    ptrs = (ctypes.c_void_p * B)(*[_chk(p, "pts").data_ptr() if p.shape[0] else None for p in pts_list])
    cnts = (ctypes.c_int32 * B)(*ns)
    crt = np.ascontiguousarray(np.asarray(crts, dtype=np.float32).reshape(B, 12))
    need = B * H.lib().dcf_compact_workspace_bytes(max(max(ns), 1))
    if ws is None or ws.numel() < need:
        ws = torch.empty((need,), dtype=torch.uint8, device=xyz_all.device)
    H.call("dcf_project_filter_batch", ctypes.addressof(ptrs), ctypes.addressof(cnts), B, H.host_f32(lim), crt, float(ulim), float(vlim), int(mode),
           uv_all, xyz_all, rows, cnt_all, ws, H.stream_ptr())
    return ws


def _check_point_frames(op, pts_list, out_list, bank=None):
    """The frame checks of the point wrappers (augment, camera mask, paste): contiguous fp32 CUDA tensors, and an output holds at
    least its frame.  bank (paste): frames, outputs and the bank are [n,3]; the capacity of an output is the kernel's to check."""
    n3 = bank is not None
    for t in list(pts_list) + list(out_list) + ([bank] if n3 else []):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and (not n3 or (t.dim() == 2 and t.shape[1] == 3))):
            raise H.DcfError("%s: %s must be contiguous fp32 CUDA tensors%s" % (op, "frames, outputs and the bank" if n3 else "frames", " [n,3]" if n3 else ""))
    if not n3 and any(o.numel() < p.numel() for p, o in zip(pts_list, out_list)):
        raise H.DcfError("%s: output smaller than its frame" % op)


def _chunk_tables(pts, outs, null_by_output=False):
    """(k, ptrs, outs, ns): the pointer and row-count tables of one chunk of k <= 8 frames.  A frame without rows travels as a null
    pointer, and so does its output -- null_by_output (paste, whose outputs hold more rows than their frames): an output is null
    when it has no rows itself."""
    k = len(pts)
    ptrs = (ctypes.c_void_p * k)(*[p.data_ptr() if p.shape[0] else None for p in pts])
    optrs = (ctypes.c_void_p * k)(*[o.data_ptr() if (o if null_by_output else p).shape[0] else None for p, o in zip(pts, outs)])
    ns = (ctypes.c_int * k)(*[int(p.shape[0]) for p in pts])
    return k, ptrs, optrs, ns


def _check_image_pair(op, img_u8, out, count, what, also=(), out_optional=False):
    """The checks of a uint8 [B,3,H,W] image and the output beside it (DcfError), with the overlap test (ValueError: neither kernel works in
    place -- the augmentation gathers neighbouring pixels, the batch's image is a view of the loader's staging set).  count: how many
    per-frame `what` came with the image; also: further (name, tensor) byte buffers; out None where out_optional: a new tensor.
    Returns (out, B, H, W)."""
    for name, t in (("img_u8", img_u8), ("out", out)) + tuple(also):
        if t is None and name == "out" and out_optional:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise H.DcfError("%s: %s must be a contiguous uint8 CUDA tensor" % (op, name))
    if img_u8.dim() != 4 or img_u8.shape[1] != 3 or img_u8.numel() == 0:
        raise H.DcfError("%s: image must be [B,3,H,W] (got %s)" % (op, tuple(img_u8.shape)))
    B, _, Hh, Ww = (int(v) for v in img_u8.shape)
    if count != B:
        raise H.DcfError("%s: %d frames, %d %s" % (op, B, count, what))
    if out is None:
        out = torch.empty_like(img_u8)
    if tuple(out.shape) != tuple(img_u8.shape) or out.device != img_u8.device:
        raise H.DcfError("%s: out must be %s on the image's device" % (op, tuple(img_u8.shape)))
    nbytes = img_u8.numel()
    if img_u8.data_ptr() < out.data_ptr() + nbytes and out.data_ptr() < img_u8.data_ptr() + nbytes:
        raise ValueError("%s: out overlaps the input" % op)
    return out, B, Hh, Ww


def augment_points_batch(pts_list, params, out_list=None):
    """Train-time BEV augmentation (augment.py) of the frames of a batch: pts_list = B device tensors [n_b,3]
    fp32 (views at any point offset of a larger buffer included), params = B augment.draw results; out_list: B tensors to write
    into (None = in place).  Bit for bit augment.transform_points, dropped points (augment.keep_mask) as +inf rows.  One launch
    per 8 frames.  Returns out_list."""
    from . import augment
    B = len(pts_list)
    if len(params) != B or (out_list is not None and len(out_list) != B):
        raise H.DcfError("augment_points_batch: %d frames, %d parameter sets" % (B, len(params)))
    out_list = pts_list if out_list is None else out_list
    _check_point_frames("augment_points_batch", pts_list, out_list)
    for b0 in range(0, B, 8):
        sl = slice(b0, min(b0 + 8, B))
        k, ptrs, outs, ns = _chunk_tables(pts_list[sl], out_list[sl])
        mat = np.ascontiguousarray(np.stack([augment.matrix5(q) for q in params[sl]], 0), dtype=np.float32)
        keys = (ctypes.c_uint64 * k)(*[int(q["drop_key"]) for q in params[sl]])
        thr = (ctypes.c_uint32 * k)(*[augment.drop_threshold(q) for q in params[sl]])
        H.call("dcf_augment_points_batch", ctypes.addressof(ptrs), ctypes.addressof(ns), k, mat, ctypes.addressof(keys), ctypes.addressof(thr),
               ctypes.addressof(outs), H.stream_ptr())
    return out_list


def camera_mask_points_batch(pts_list, crts, lim, ulim, vlim, mode, fov, occ_list=None, out_list=None):
    """The camera visibility mask (visibility.py) of the frames of a batch: pts_list = B device tensors [n_b,3]
    fp32 (views at any point offset of a larger buffer included), crts [B,4,3] (or [B,12]) host floats, one matrix per frame; lim,
    ulim, vlim, mode as for project_filter_batch; fov: rows the projection would not keep become +inf rows; occ_list: per frame None
    or fp32 [m_b,5] = (x0, y0, x1, y1, D), m_b <= 16 (visibility.occluders); out_list: B tensors to write into (None = in place).
    Bit for bit visibility.mask_points per frame.  One launch per 8 frames.  Returns out_list."""
    B = len(pts_list)
    if (out_list is not None and len(out_list) != B) or (occ_list is not None and len(occ_list) != B):
        raise H.DcfError("camera_mask_points_batch: %d frames, %s outputs, %s occluder sets"
                         % (B, "no" if out_list is None else len(out_list), "no" if occ_list is None else len(occ_list)))
    out_list = pts_list if out_list is None else out_list
    _check_point_frames("camera_mask_points_batch", pts_list, out_list)
    crt = np.ascontiguousarray(np.asarray(crts, dtype=np.float32).reshape(B, 12))
    for b0 in range(0, B, 8):
        sl = slice(b0, min(b0 + 8, B))
        k, ptrs, outs, ns = _chunk_tables(pts_list[sl], out_list[sl])
        occ = np.zeros((k, 16, 5), dtype=np.float32)
        ms = (ctypes.c_int * k)()
        for i in range(k):
            q = None if occ_list is None else occ_list[b0 + i]
            if q is None:
                continue
            q = np.asarray(q, dtype=np.float32).reshape(-1, 5)
            if len(q) > 16:
                raise H.DcfError("camera_mask_points_batch: a frame holds at most 16 occluders (got %d)" % len(q))
            ms[i] = len(q)
            occ[i, :len(q)] = q
        H.call("dcf_camera_mask_points_batch", ctypes.addressof(ptrs), ctypes.addressof(ns), k, H.host_f32(lim), np.ascontiguousarray(crt[sl]),
               float(ulim), float(vlim), int(mode), int(bool(fov)), ctypes.addressof(ms), occ, ctypes.addressof(outs), H.stream_ptr())
    return out_list


def augment_image_batch(img_u8, params, out=None):
    """Train-time camera image augmentation (augment_image.py) of the frames of a batch: img_u8 = a contiguous
    uint8 device tensor [B,3,H,W] (a view at any byte offset of a larger buffer included), params = B augment_image.draw results;
    out: a contiguous uint8 [B,3,H,W] tensor to write into (None = a new one).  It must not overlap the input -- the kernel
    gathers neighbours -- ValueError.  Bit for bit augment_image.transform_image per frame.  One launch per 8 frames.  Returns out."""
    from . import augment_image
    out, B, Hh, Ww = _check_image_pair("augment_image_batch", img_u8, out, len(params), "parameter sets", out_optional=True)
    for p in params:                                 # drawn for another image size: the centre would move
        if (p.get("width", Ww), p.get("height", Hh)) != (Ww, Hh):
            raise H.DcfError("augment_image_batch: parameters of a %d x %d image for a %d x %d one" % (p["width"], p["height"], Ww, Hh))
    for b0 in range(0, B, 8):
        k = min(b0 + 8, B) - b0
        q = np.ascontiguousarray(np.stack([augment_image.vector8(p) for p in params[b0:b0 + k]], 0), dtype=np.float32)
        H.call("dcf_augment_image_batch", img_u8[b0:b0 + k], k, Hh, Ww, q, out[b0:b0 + k], H.stream_ptr())
    return out


PASTE_STAGE_BYTES = 8192       # the staging buffers of dcf_paste_*_batch: at least the larger table (5440 bytes for 8 frames)
PASTE_VALUE_MAX = 4            # up to this many frames per call the tables travel in the kernel argument: no staging
_paste_rings = {}


def _paste_stage(dev):
    """(pinned host buffer, device buffer) for one paste launch of 5 .. 8 frames on the current stream: a ring of four pairs per device (the way of
    LossTotal._stage) -- the pair being refilled was last used four launches ago, so the wait for its event does not block.  The
    event is recorded behind the launch (paste_stage_done), so neither the copy nor the kernel can still read the pair."""
    ring = _paste_rings.get(dev)
    if ring is None:
        ring = _paste_rings[dev] = {"slot": 0, "sets": [[torch.empty(PASTE_STAGE_BYTES, dtype=torch.uint8).pin_memory(),
                                                          torch.empty(PASTE_STAGE_BYTES, dtype=torch.uint8, device=dev), None] for _ in range(4)]}
    st = ring["sets"][ring["slot"]]
    ring["slot"] = (ring["slot"] + 1) % len(ring["sets"])
    if st[2] is not None:
        st[2].synchronize()
    return st


def _paste_stage_done(st):
    st[2] = torch.cuda.Event()
    st[2].record()


def paste_points_batch(pts_list, plans, bank_points, out_list):
    """Train-time object pasting, the points (paste.py): pts_list = B device tensors [n_b,3] fp32 (views at any
    point offset of a larger buffer included), plans = B paste.draw results, bank_points = the bank's `points` on the device
    [P,3] fp32, out_list = B contiguous fp32 device tensors [rows_b,3] with rows_b >= n_b + a_b, overlapping no input.  Bit for bit
    paste.paste_points per frame; rows past n_b + a_b are not written.  One launch per 8 frames; its table travels in the kernel
    argument (up to 4 frames) or in one asynchronous copy from a pinned ring on the current stream (5 .. 8).  Returns the B views
    out_list[b][:n_b + a_b]."""
    B = len(pts_list)
    if len(plans) != B or len(out_list) != B:
        raise H.DcfError("paste_points_batch: %d frames, %d plans, %d outputs" % (B, len(plans), len(out_list)))
    _check_point_frames("paste_points_batch", pts_list, out_list, bank=bank_points)
    res = []
    for b0 in range(0, B, 8):
        sl = slice(b0, min(b0 + 8, B))
        k, ptrs, outs, ns = _chunk_tables(pts_list[sl], out_list[sl], null_by_output=True)
        rec, app = np.zeros((k, 16, 8), dtype=np.float32), np.zeros((k, 16, 2), dtype=np.int64)
        ms = (ctypes.c_int * k)()
        for i, p in enumerate(plans[sl]):
            m = len(p["records"])
            if m > 16 or len(p["append"]) != m:
                raise H.DcfError("paste_points_batch: a plan holds at most 16 records, one append entry each")
            ms[i] = m
            rec[i, :m], app[i, :m] = p["records"], p["append"]
        caps = (ctypes.c_int * k)(*[int(o.shape[0]) for o in out_list[sl]])
        st = _paste_stage(bank_points.device) if k > PASTE_VALUE_MAX else (None, None)
        H.call("dcf_paste_points_batch", ctypes.addressof(ptrs), ctypes.addressof(ns), k, ctypes.addressof(ms), rec, app,
               bank_points if bank_points.shape[0] else None, int(bank_points.shape[0]), ctypes.addressof(outs), ctypes.addressof(caps),
               st[0], st[1], PASTE_STAGE_BYTES, H.stream_ptr())
        if k > PASTE_VALUE_MAX:
            _paste_stage_done(st)
        for i in range(k):
            res.append(out_list[b0 + i][:ns[i] + int(app[i, :ms[i], 1].sum())])
    return res


def paste_patches_batch(img_u8, plans, bank_patch, out):
    """Train-time object pasting, the image patches (paste.py): img_u8 = a contiguous uint8 device tensor
    [B,3,H,W] (a view at any byte offset of a larger buffer included), plans = B paste.draw results, bank_patch = the bank's `patch`
    bytes on the device, out = a contiguous uint8 [B,3,H,W] tensor that does not overlap the input (the batch's image is a view of
    the loader's staging set) -- ValueError.  Byte for byte paste.paste_image per frame.  One launch per 8 frames.  Returns out."""
    out, B, Hh, Ww = _check_image_pair("paste_patches_batch", img_u8, out, len(plans), "plans", also=(("bank_patch", bank_patch),))
    for p in plans:                                  # drawn for another image size: the clipping would be another
        if tuple(p.get("image_hw", (Hh, Ww))) != (Hh, Ww):
            raise ValueError("paste_patches_batch: a plan of %s images for %d x %d ones" % (tuple(p["image_hw"]), Hh, Ww))
    for b0 in range(0, B, 8):
        k = min(b0 + 8, B) - b0
        rec = np.zeros((k, 16, 9), dtype=np.int64)
        ms = (ctypes.c_int * k)()
        for i, p in enumerate(plans[b0:b0 + k]):
            m = len(p["patches"])
            if m > 16:
                raise H.DcfError("paste_patches_batch: a plan holds at most 16 patch records")
            ms[i] = m
            rec[i, :m] = p["patches"]
        st = _paste_stage(img_u8.device) if k > PASTE_VALUE_MAX else (None, None)
        H.call("dcf_paste_patches_batch", img_u8[b0:b0 + k], k, Hh, Ww, ctypes.addressof(ms), rec, bank_patch if bank_patch.numel() else None,
               int(bank_patch.numel()), out[b0:b0 + k], st[0], st[1], PASTE_STAGE_BYTES, H.stream_ptr())
        if k > PASTE_VALUE_MAX:
            _paste_stage_done(st)
    return out


def knn_bev(xyz, cnt, K, h, w, stride, aff, rmax=None, ws=None, out=None):
    """out: optional int32 [K,h,w] tensor to write into (e.g. a frame's slice of a batch tensor)."""
    n_max = xyz.shape[0]
    dev = xyz.device
    idx = torch.empty((K, h, w), dtype=torch.int32, device=dev) if out is None else _chk(out, "out")
    if ws is None:
        ws = torch.empty((H.lib().dcf_knn_workspace_bytes(n_max, h, w),), dtype=torch.uint8, device=dev)
    r2 = -1.0 if rmax is None else float(np.float32(rmax) * np.float32(rmax))
    H.call("dcf_knn_bev", _chk(xyz, "xyz"), cnt, n_max, K, h, w, stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]),
           r2, idx, ws, H.stream_ptr())
    return idx


def knn_ws_stride(n_max, h, w):
    """Bytes between the per-frame workspaces of knn_bev_batch."""
    return (H.lib().dcf_knn_workspace_bytes(n_max, h, w) + 255) // 256 * 256


def knn_bev_batch(xyz, cnt, K, h, w, stride, aff, rmax=None, ws=None, out=None):
    """All frames of a batch in one launch per phase: xyz [B,n_max,3], cnt int32 [B] -> idx int32 [B,K,h,w]
    (= knn_bev frame by frame).  ws: uint8 [B, knn_ws_stride(...)]."""
    B, n_max = xyz.shape[0], xyz.shape[1]
    dev = xyz.device
    st = knn_ws_stride(n_max, h, w)
    idx = torch.empty((B, K, h, w), dtype=torch.int32, device=dev) if out is None else _chk(out, "out")
    if ws is None:
        ws = torch.empty((B, st), dtype=torch.uint8, device=dev)
    if ws.shape[0] < B or ws.stride(0) != st:
        raise H.DcfError("knn_bev_batch: workspace must be [B, %d] bytes" % st)
    r2 = -1.0 if rmax is None else float(np.float32(rmax) * np.float32(rmax))
    H.call("dcf_knn_bev_batch", _chk(xyz, "xyz"), _chk(cnt, "cnt"), B, n_max, K, h, w, stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]),
           r2, idx, ws, st, H.stream_ptr())
    return idx


def knn_bev_batch_shared(xyz, cnt, K, h, w, stride, fine, ws_fine, aff, rmax=None, ws=None, out=None):
    """A coarser site of the same batch: own cell sort (ws) + a search that serves dense regions from the cells of a finer site:
    fine = (h, w, stride) of the knn_bev_batch call whose workspace ws_fine ([B, knn_ws_stride(n_max, fine_h, fine_w)] bytes,
    untouched since) is read.  Same indices as knn_bev_batch."""
    B, n_max = xyz.shape[0], xyz.shape[1]
    fh, fw, fs = fine
    stf = knn_ws_stride(n_max, fh, fw)
    if ws_fine.shape[0] < B or ws_fine.stride(0) != stf:
        raise H.DcfError("knn_bev_batch_shared: the fine site's workspace must be [B, %d] bytes" % stf)
    st = knn_ws_stride(n_max, h, w)
    if ws is None:
        ws = torch.empty((B, st), dtype=torch.uint8, device=xyz.device)
    if ws.shape[0] < B or ws.stride(0) != st:
        raise H.DcfError("knn_bev_batch_shared: workspace must be [B, %d] bytes" % st)
    idx = torch.empty((B, K, h, w), dtype=torch.int32, device=xyz.device) if out is None else _chk(out, "out")
    r2 = -1.0 if rmax is None else float(np.float32(rmax) * np.float32(rmax))
    H.call("dcf_knn_bev_batch_shared", _chk(xyz, "xyz"), _chk(cnt, "cnt"), B, n_max, K, h, w, stride, fh, fw, fs, float(aff[0]), float(aff[1]),
           float(aff[2]), float(aff[3]), r2, idx, ws, st, ws_fine, stf, H.stream_ptr())
    return idx


def knn_bev_sites(xyz, cnt, K, sites, aff, rmax=None):
    """Every fusion site of a batch in one call (dcf_knn_bev_sites): the cell sort of all sites in one launch per phase, then
    the searches.  sites = list of (h, w, stride, fine, ws, out): fine = index of an earlier, finer site whose cells serve this
    site's dense pixels (as knn_bev_batch_shared) or -1 (as knn_bev_batch); ws uint8 [B, knn_ws_stride(n_max, h, w)]; out int32
    [B, K, h, w].  Same maps as the per-site calls."""
    B, n_max = xyz.shape[0], xyz.shape[1]
    arr = (H.KnnSite * len(sites))()
    for i, (h, w, stride, fine, ws, out) in enumerate(sites):
        st = knn_ws_stride(n_max, h, w)
        if ws.shape[0] < B or ws.stride(0) != st or ws.dtype != torch.uint8:
            raise H.DcfError("knn_bev_sites: site %d: workspace must be uint8 [B, %d]" % (i, st))
        if tuple(out.shape) != (B, K, h, w) or out.dtype != torch.int32 or not out.is_contiguous():
            raise H.DcfError("knn_bev_sites: site %d: out must be a contiguous int32 [B, K, h, w]" % i)
        arr[i] = H.KnnSite(h, w, stride, fine, out.data_ptr(), ws.data_ptr(), st)
    r2 = -1.0 if rmax is None else float(np.float32(rmax) * np.float32(rmax))
    H.call("dcf_knn_bev_sites", _chk(xyz, "xyz"), _chk(cnt, "cnt"), B, n_max, K, ctypes.addressof(arr), len(sites), float(aff[0]), float(aff[1]),
           float(aff[2]), float(aff[3]), r2, H.stream_ptr())
    return [t[5] for t in sites]


# ------------------------------------------------------------------ fusion
def point_sample_fwd(dtype, fmap, uv, cnt, n_max, out=None):
    """out: optional [n_max, Cf] tensor to write into (a frame's slice of a batch tensor); every row is written (zeros past cnt)."""
    Hf, Wf, Cf = fmap.shape
    fp = (torch.empty if n_max > 0 else torch.zeros)((max(n_max, 1), Cf), dtype=fmap.dtype, device=fmap.device) if out is None else _chk(out, "out")
    H.call("dcf_point_sample_fwd", dtype, fmap, Hf, Wf, Cf, uv, cnt, n_max, fp, H.stream_ptr())
    return fp


def point_sample_bwd(dtype, gfp, uv, cnt, n_max, gfmap):
    Hf, Wf, Cf = gfmap.shape
    H.call("dcf_point_sample_bwd", dtype, gfp, Hf, Wf, Cf, uv, cnt, n_max, gfmap, H.stream_ptr())
    return gfmap


def point_sample_fwd_batch(dtype, fmap, uv, cnt, n_max, out):
    """All frames in one launch: fmap [B,Hf,Wf,Cf], uv [B,rows,2], cnt int32 [B], out [B,n_max,Cf] (every row is written: zeros past a frame's count)."""
    B, Hf, Wf, Cf = fmap.shape
    H.call("dcf_point_sample_fwd_batch", dtype, _chk(fmap, "fmap"), Hf, Wf, Cf, _chk(uv, "uv"), uv.stride(0), cnt, n_max, _chk(out, "out"), B, H.stream_ptr())
    return out


def point_sample_bwd_batch(dtype, gfp, uv, cnt, n_max, gfmap):
    """gfp [B,n_max,Cf], gfmap fp32 [B,Hf,Wf,Cf] (accumulated into)."""
    B, Hf, Wf, Cf = gfmap.shape
    H.call("dcf_point_sample_bwd_batch", dtype, _chk(gfp, "gfp"), Hf, Wf, Cf, _chk(uv, "uv"), uv.stride(0), cnt, n_max, _chk(gfmap, "gfmap"), B, H.stream_ptr())
    return gfmap


def fusion_gather_fwd_batch(dtype, P, xyz, idx, stride, aff, w1d, b1, hsum, cnt):
    """P [B,rows,Cb], xyz [B,n,3], idx int32 [B,K,h,w] -> hsum [B,h,w,Cb], cnt fp32 [B,h*w] (written)."""
    B, K, h, w = idx.shape
    Cb = P.shape[2]
    H.call("dcf_fusion_gather_fwd_batch", dtype, _chk(P, "P"), P.shape[1], _chk(xyz, "xyz"), xyz.stride(0), _chk(idx, "idx"), K, h, w, stride,
           float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]), w1d, b1, Cb, _chk(hsum, "hsum"), _chk(cnt, "cnt"), B, H.stream_ptr())
    return hsum, cnt


def fusion_gather_bwd_inv_batch(dtype, P, xyz, inv, n_max, g0, khw, stride, aff, w1d, b1, ghsum, gP, gw1d, gb1, ws=None):
    """fusion_gather_bwd_inv for the B frames of a batch in one launch: their maps are g0 .. g0 + B - 1 of the fusion_invert call;
    P [B,rows,Cb], xyz [B,n,3], ghsum [B,h,w,Cb], gP fp32 [B,rows,Cb]."""
    start, ent = inv
    B, rows, Cb = P.shape
    seg = start[g0 * (n_max + 1):]
    H.call("dcf_fusion_gather_bwd_inv_batch", dtype, _chk(P, "P"), rows, _chk(xyz, "xyz"), xyz.stride(0), seg, seg[n_max:], n_max + 1, ent[0], ent[1],
           khw[0] * khw[1] * khw[2], khw[1], khw[2], stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]), w1d, b1, Cb,
           _chk(ghsum, "ghsum"), _chk(gP, "gP"), gw1d, gb1, ws, B, H.stream_ptr())


_DWS_BYTES = {}


def fusion_bwd_direct_workspace(device, max_entries, Cb, B):
    """Zeroed workspace of fusion_gather_bwd_direct_batch for maps of up to max_entries (= K*h*w) pairs (left zero by the kernel)."""
    return torch.zeros((max(H.lib().dcf_fusion_gather_bwd_direct_workspace_bytes(max_entries, Cb, B) // 4, 1),), dtype=torch.float32, device=device)


def fusion_gather_bwd_direct_batch(dtype, P, xyz, inv, n_max, g0, khw, stride, aff, w1d, b1, ghsum, gP, gw1d, gb1, ws, dws):
    """fusion_gather_bwd_inv_batch with gP [B,rows,Cb] in the compute dtype, ZERO on entry: rows are stored whole by their single
    writer; the few rows whose pairs cross a slice boundary go through dws (fusion_bwd_direct_workspace)."""
    start, ent = inv
    B, rows, Cb = P.shape
    me = khw[0] * khw[1] * khw[2]
    if gP.dtype != P.dtype or gP.shape != P.shape:
        raise H.DcfError("fusion_gather_bwd_direct_batch: gP must look like P")
    need = _DWS_BYTES.get((me, Cb, B))
    if need is None:
        need = _DWS_BYTES[(me, Cb, B)] = H.lib().dcf_fusion_gather_bwd_direct_workspace_bytes(me, Cb, B)
    if dws.numel() * 4 < need:
        raise H.DcfError("fusion_gather_bwd_direct_batch: workspace too small")
    # (raw addresses of the map's start segment and of the two pair arrays: four tensor views per call otherwise)
    seg = start.data_ptr() + 4 * g0 * (n_max + 1)
    H.call("dcf_fusion_gather_bwd_direct_batch", dtype, _chk(P, "P"), rows, _chk(xyz, "xyz"), xyz.stride(0), seg, seg + 4 * n_max, n_max + 1,
           ent.data_ptr(), ent.data_ptr() + 4 * ent.stride(0), me, khw[1], khw[2], stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]),
           w1d, b1, Cb, _chk(ghsum, "ghsum"), _chk(gP, "gP"), gw1d, gb1, ws, dws, B, H.stream_ptr())


def fusion_gather_fwd(dtype, P, xyz, idx, stride, aff, w1d, b1, out=None):
    """out: optional (hsum [h,w,Cb], cnt [h*w]) to write into (a frame's slices of batch tensors)."""
    K, h, w = idx.shape
    Cb = P.shape[1]
    if out is not None:
        hsum, cnt = _chk(out[0], "hsum"), _chk(out[1], "cnt")
    else:
        hsum = torch.empty((h, w, Cb), dtype=P.dtype, device=P.device)
        cnt = torch.empty((h * w,), dtype=torch.float32, device=P.device)
    H.call("dcf_fusion_gather_fwd", dtype, P, xyz, idx, K, h, w, stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]),
           w1d, b1, Cb, hsum, cnt, H.stream_ptr())
    return hsum, cnt


def fusion_gather_bwd(dtype, P, xyz, idx, stride, aff, w1d, b1, ghsum, gP, gw1d, gb1):
    K, h, w = idx.shape
    Cb = P.shape[1]
    H.call("dcf_fusion_gather_bwd", dtype, P, xyz, idx, K, h, w, stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]),
           w1d, b1, Cb, ghsum, gP, gw1d, gb1, H.stream_ptr())


def fusion_invert_sizes(maps, n_max):
    """(elements of start, pairs, workspace bytes) of fusion_invert for these maps."""
    return len(maps) * (n_max + 1), sum(t.numel() for t in maps), H.lib().dcf_fusion_invert_workspace_bytes(n_max, len(maps))


def fusion_invert(maps, n_max, out=None):
    """maps: list of KNN maps [K,h,w] (sites x frames of a step).  Returns (start [len(maps)*(n_max+1)], ent [2, pairs]):
    the (pixel, point) pairs of all maps sorted by (map, point) -- see dcf_fusion_invert.
    out: optional (start, ent, ws) buffers of fusion_invert_sizes() to write into."""
    K = maps[0].shape[0]
    dev = maps[0].device
    tab = (H.KnnMap * len(maps))()
    total = 0
    for i, t in enumerate(maps):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.shape[0] == K
        tab[i] = H.KnnMap(t.data_ptr(), t.shape[1], t.shape[2])
        total += t.numel()
    if out is not None:
        start, ent, ws = out
    else:
        start = torch.empty((len(maps) * (n_max + 1),), dtype=torch.int32, device=dev)
        ent = torch.empty((2, total), dtype=torch.int32, device=dev)
        ws = torch.empty((H.lib().dcf_fusion_invert_workspace_bytes(n_max, len(maps)),), dtype=torch.uint8, device=dev)
    H.call("dcf_fusion_invert", ctypes.addressof(tab), len(maps), K, n_max, start, ent[0], ent[1], ws, H.stream_ptr())
    return start, ent


def fusion_bwd_workspace(device, Cb=256):
    """Zeroed workspace of fusion_gather_bwd_inv's slotted dW1d / db1 reduction (left zero: reusable by calls ordered on one stream)."""
    return torch.zeros((H.lib().dcf_fusion_gather_bwd_workspace_bytes(Cb) // 4,), dtype=torch.float32, device=device)


def fusion_gather_bwd_inv(dtype, P, xyz, inv, n_max, g, khw, stride, aff, w1d, b1, ghsum, gP, gw1d, gb1, ws=None):
    """n_max: the point-id range fusion_invert was called with; g: index of this (site, frame) map in that call;
    khw = (K, h, w) of the map.  P / gP may hold fewer rows than n_max (only ids below the valid count occur).
    ws: fusion_bwd_workspace() -> gw1d / gb1 through 16 accumulator copies folded by the last workgroup (16 instead of 256
    same-address atomics per word)."""
    start, ent = inv
    Cb = P.shape[1]
    seg = start[g * (n_max + 1):]
    if ws is not None and ws.numel() * 4 < H.lib().dcf_fusion_gather_bwd_workspace_bytes(Cb):
        raise H.DcfError("fusion_gather_bwd_inv: workspace too small for %d channels" % Cb)
    H.call("dcf_fusion_gather_bwd_inv", dtype, P, xyz, seg, seg[n_max:], ent[0], ent[1], khw[0] * khw[1] * khw[2], khw[1], khw[2], stride,
           float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]), w1d, b1, Cb, ghsum, gP, gw1d, gb1, ws, H.stream_ptr())


def rowscale_bias_fwd(dtype, y, cnt, b2):
    C = y.shape[-1]
    H.call("dcf_rowscale_bias_fwd", dtype, y, cnt, b2, y.numel() // C, C, H.stream_ptr())
    return y


def rowscale_bias_bwd(dtype, gy, cnt, gb2):
    C = gy.shape[-1]
    H.call("dcf_rowscale_bias_bwd", dtype, gy, cnt, gb2, gy.numel() // C, C, H.stream_ptr())


def relu_mask_rowscale_bwd(dtype, gy, y, cnt, gb2):
    """gout = gy * (y > 0) as a NEW tensor; gb2[c] += sum_p cnt[p] * gy[p][c] (one pass over gy: dcf_relu_mask_rowscale_bwd)."""
    C = gy.shape[-1]
    gout = torch.empty_like(gy)
    H.call("dcf_relu_mask_rowscale_bwd", dtype, _chk(gy, "gy"), _chk(y, "y"), cnt, gout, gb2, gy.numel() // C, C, H.stream_ptr())
    return gout


def fusion_gather_bwd_pts(dtype, P, xyz, inv, n_max, g, khw, stride, aff, w1d, b1, ghsum, gP, gw1d, gb1):
    """fusion_gather_bwd_inv with one writer per point row: gP [n_rows, Cb] in the compute dtype, fully written (no zero-fill
    before, no cast after).  Arguments as fusion_gather_bwd_inv."""
    start, ent = inv
    Cb = P.shape[1]
    seg = start[g * (n_max + 1):]
    H.call("dcf_fusion_gather_bwd_pts", dtype, P, xyz, seg, P.shape[0], ent[0], ent[1], khw[0] * khw[1] * khw[2], khw[1], khw[2], stride,
           float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]), w1d, b1, Cb, ghsum, gP, gw1d, gb1, H.stream_ptr())


# ------------------------------------------------------------------ deterministic mode (csrc/fusion_det.hip)
def inv_sort_segments(start, keys, scratch=None, nseg=None):
    """Sort every segment keys[start[s]:start[s+1]] (s < nseg, default len(start) - 1) ascending in place; keys are unique inside a
    segment.  scratch: int32 like keys (segments beyond 4096 keys are sorted through it)."""
    if scratch is None:
        scratch = torch.empty_like(keys)
    if scratch.numel() < keys.numel() or scratch.dtype != torch.int32 or keys.dtype != torch.int32 or start.dtype != torch.int32:
        raise H.DcfError("inv_sort_segments: int32 tensors, scratch as long as keys")
    H.call("dcf_inv_sort_segments", _chk(start, "start"), start.numel() - 1 if nseg is None else int(nseg), _chk(keys, "keys"), scratch, H.stream_ptr())
    return keys


def fusion_invert_sorted(maps, n_max, out=None, scratch=None):
    """fusion_invert with every point's pairs in ascending pixel order ((i << 16) | j): the map no longer depends on the order in
    which the fill's workgroups ran.  scratch: optional int32 [pairs]."""
    start, ent = fusion_invert(maps, n_max, out=out)
    inv_sort_segments(start, ent[0], scratch)
    return start, ent


def cam_invert_buffers(B, n_max, Hf, Wf, device):
    """(start [B*(Hf*Wf+1)], ent [B*4*n_max], scratch like ent, ws) for cam_invert."""
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty((B * (Hf * Wf + 1),), **i32), torch.empty((max(B * 4 * n_max, 1),), **i32), torch.empty((max(B * 4 * n_max, 1),), **i32),
            torch.empty((H.lib().dcf_cam_invert_workspace_bytes(Hf, Wf, B),), dtype=torch.uint8, device=device))


def cam_invert(uv, cnt, n_max, Hf, Wf, out=None):
    """Inverse of the point sampler's scatter: uv [B,rows,2], cnt int32 [B] -> (start, ent, (Hf, Wf)); segment b*(Hf*Wf+1)+pixel of
    ent lists the keys point*4+tap that touch the camera-map pixel, ascending (see dcf_cam_invert)."""
    B = uv.shape[0]
    start, ent, scratch, ws = out if out is not None else cam_invert_buffers(B, n_max, Hf, Wf, uv.device)
    if start.numel() < B * (Hf * Wf + 1) or ent.numel() < B * 4 * n_max or scratch.numel() < B * 4 * n_max:
        raise H.DcfError("cam_invert: buffers too small")
    H.call("dcf_cam_invert", _chk(uv, "uv"), uv.stride(0), _chk(cnt, "cnt"), n_max, Hf, Wf, B, start, ent, scratch, ws, H.stream_ptr())
    return start, ent, (Hf, Wf)


def point_sample_bwd_det(dtype, gfp, uv, cam_inv, gfmap):
    """gfp [B,rows,Cf], uv [B,*,2], cam_inv = cam_invert(...) -> gfmap fp32 [B,Hf,Wf,Cf], every row stored once, fixed order."""
    B, Hf, Wf, Cf = gfmap.shape
    start, ent, hw = cam_inv
    if tuple(hw) != (Hf, Wf) or gfmap.dtype != torch.float32:
        raise H.DcfError("point_sample_bwd_det: the camera-pixel map was built for a %s map, the gradient is %s" % (tuple(hw), (Hf, Wf)))
    H.call("dcf_point_sample_bwd_det", dtype, _chk(gfp, "gfp"), gfp.shape[1], Hf, Wf, Cf, _chk(uv, "uv"), uv.stride(0), start, ent, _chk(gfmap, "gfmap"), B,
           H.stream_ptr())
    return gfmap


def fusion_bwd_det_workspace(device, max_entries, Cb, B):
    """Workspace of fusion_gather_bwd_det (contents free: nothing to zero)."""
    return torch.empty((max(H.lib().dcf_fusion_gather_bwd_det_workspace_bytes(max_entries, Cb, B) // 4, 1),), dtype=torch.float32, device=device)


def fusion_gather_bwd_det(dtype, P, xyz, inv, n_max, g0, khw, stride, aff, w1d, b1, ghsum, gP, gw1d, gb1, ws):
    """fusion_gather_bwd_direct_batch in one fixed order on SORTED maps (fusion_invert_sorted): gP [B,rows,Cb] in the compute dtype,
    every row stored (no zero-fill); gw1d / gb1 accumulated."""
    start, ent = inv
    B, rows, Cb = P.shape
    me = khw[0] * khw[1] * khw[2]
    if gP.dtype != P.dtype or gP.shape != P.shape:
        raise H.DcfError("fusion_gather_bwd_det: gP must look like P")
    if ws.numel() * 4 < H.lib().dcf_fusion_gather_bwd_det_workspace_bytes(me, Cb, B):
        raise H.DcfError("fusion_gather_bwd_det: workspace too small")
    seg = start.data_ptr() + 4 * g0 * (n_max + 1)
    H.call("dcf_fusion_gather_bwd_det", dtype, _chk(P, "P"), rows, _chk(xyz, "xyz"), xyz.stride(0), seg, n_max, ent.data_ptr(),
           ent.data_ptr() + 4 * ent.stride(0), me, khw[1], khw[2], stride, float(aff[0]), float(aff[1]), float(aff[2]), float(aff[3]),
           w1d, b1, Cb, _chk(ghsum, "ghsum"), _chk(gP, "gP"), gw1d, gb1, ws, B, H.stream_ptr())


def rowscale_bias_det_workspace(device, C):
    return torch.empty((H.lib().dcf_rowscale_bias_bwd_det_workspace_bytes(C) // 4,), dtype=torch.float32, device=device)


def rowscale_bias_bwd_det(dtype, gy, cnt, gb2, ws, y=None):
    """gb2[c] += sum_p cnt[p] * gy[p][c] in one fixed order; with y also returns gy * (y > 0) as a new tensor."""
    C = gy.shape[-1]
    gout = None if y is None else torch.empty_like(gy)
    H.call("dcf_rowscale_bias_bwd_det", dtype, _chk(gy, "gy"), None if y is None else _chk(y, "y"), cnt, gout, gb2, gy.numel() // C, C, ws, H.stream_ptr())
    return gout


# ------------------------------------------------------------------ evaluation post-processing
EVAL_NMS_CAP = 4096


def eval_score_filter(pred, threshold, cap=EVAL_NMS_CAP):
    """test.py:88-108 on the device: pred [B,32,h,w] fp32 -> (boxes [B,cap,7], count int32 [B]); per sample anchor 0's boxes
    with score > threshold in raster order, then anchor 1's."""
    B, C, h, w = pred.shape
    if C != 32 or pred.dtype != torch.float32:
        raise H.DcfError("eval_score_filter: pred must be the model output [B,32,h,w] fp32")
    pred = _chk(pred.contiguous(), "pred")
    boxes = torch.zeros((B, cap, 7), dtype=torch.float32, device=pred.device)
    count = torch.zeros((B,), dtype=torch.int32, device=pred.device)
    H.call("dcf_eval_score_filter", pred, B, h, w, float(threshold), cap, boxes, count, H.stream_ptr())
    return boxes, count


def eval_nms(boxes, mode, iou_threshold=0.01, count=None):
    """Greedy suppression in input order (test.py:110-175): boxes [n,7] fp32 on the device -> keep flags int32 [n].
    mode "sat" | "iou" | "bev" (bird's-eye IoU of the (x, y) rectangles, the ranked evaluation's: rows are then in rank order);
    count: optional int32 [1] device tensor with the number of valid rows."""
    n = boxes.shape[0]
    if n > EVAL_NMS_CAP:
        raise H.DcfError("eval_nms: at most %d boxes per call (got %d)" % (EVAL_NMS_CAP, n))
    boxes = _chk(boxes.float().contiguous(), "boxes")
    keep = torch.zeros((max(n, 1),), dtype=torch.int32, device=boxes.device)
    nkeep = torch.zeros((1,), dtype=torch.int32, device=boxes.device)
    ws = torch.empty((H.lib().dcf_eval_nms_workspace_bytes(max(n, 1)),), dtype=torch.uint8, device=boxes.device)
    H.call("dcf_eval_nms", boxes, count, n, {"sat": 0, "iou": 1, "bev": 2}[mode], float(iou_threshold), keep, nkeep, ws, H.stream_ptr())
    return keep[:n], nkeep


def eval_match(pred_boxes, ref_boxes, thresholds, tp):
    """tp[t] += number of pred_boxes [n,7] whose bird's-eye IoU with a labelled row of ref_boxes [R,9] exceeds thresholds[t]
    (fp64 device tensor); tp int32 [len(thresholds)] on the device (test.py:177-206)."""
    n = pred_boxes.shape[0]
    if n == 0:
        return tp
    H.call("dcf_eval_match", _chk(pred_boxes.float().contiguous(), "pred_boxes"), n, _chk(ref_boxes.float().contiguous(), "ref_boxes"),
           ref_boxes.shape[0], thresholds, thresholds.shape[0], tp, H.stream_ptr())
    return tp


# ------------------------------------------------------------------ ranked evaluation (eval_metric: ranked)
def eval_rank_filter(pred, threshold, cap=EVAL_NMS_CAP):
    """pred [B,32,h,w] fp32 -> (boxes [B,cap,7], scores [B,cap], count int32 [B], total int32 [B]): per sample the candidates with
    score > threshold in rank order (score descending, ties to the lower candidate index); total = how many passed,
    count = min(total, cap) -- exactly the cap highest-ranked are kept when total exceeds it."""
    B, C, h, w = pred.shape
    if C != 32 or pred.dtype != torch.float32:
        raise H.DcfError("eval_rank_filter: pred must be the model output [B,32,h,w] fp32")
    if not 0 < cap <= EVAL_NMS_CAP:
        raise H.DcfError("eval_rank_filter: cap must be in 1..%d (got %d)" % (EVAL_NMS_CAP, cap))
    pred = _chk(pred.contiguous(), "pred")
    dev = pred.device
    boxes = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
    scores = torch.zeros((B, cap), dtype=torch.float32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    total = torch.zeros((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((H.lib().dcf_eval_rank_workspace_bytes(B, h, w),), dtype=torch.uint8, device=dev)
    H.call("dcf_eval_rank_filter", pred, B, h, w, float(threshold), cap, boxes, scores, count, total, ws, H.stream_ptr())
    return boxes, scores, count, total


def eval_match_ranked(boxes, keep, count, ref_boxes, thresholds):
    """One-to-one matching of the survivors (keep flags of eval_nms over boxes [n,7], count int32 [1] valid rows) against the
    labelled rows of ref_boxes [R,9], per threshold of thresholds (fp64 device tensor, at most 16): tpmask int32 [n], bit t set
    iff the survivor is a true positive at thresholds[t] (the bits of a uint32)."""
    n, R = boxes.shape[0], ref_boxes.shape[0]
    tpmask = torch.zeros((max(n, 1),), dtype=torch.int32, device=boxes.device)
    if n == 0:
        return tpmask[:0]
    ws = torch.empty((H.lib().dcf_eval_match_ranked_workspace_bytes(n, R),), dtype=torch.uint8, device=boxes.device)
    H.call("dcf_eval_match_ranked", _chk(boxes, "boxes"), _chk(keep, "keep"), count, n, _chk(ref_boxes, "ref_boxes") if R else None, R,
           thresholds, thresholds.shape[0], tpmask, ws, H.stream_ptr())
    return tpmask


def eval_accumulate(scores, tpmask, keep, count, total, ref_boxes, acc_scores, acc_tpmask, state):
    """Appends (score, tpmask) of one sample's survivors, in order, to acc_scores fp32 / acc_tpmask int32 [capacity] at the device
    cursor state[0]; state int64 [4] = (cursor, labelled rows seen, samples with total > len(scores), unused).  The cursor counts
    on past the capacity; nothing is written past it."""
    n, R = scores.shape[0], ref_boxes.shape[0]
    H.call("dcf_eval_accumulate", _chk(scores, "scores"), _chk(tpmask, "tpmask"), _chk(keep, "keep"), count, total, n,
           _chk(ref_boxes, "ref_boxes") if R else None, R, acc_scores, acc_tpmask, acc_scores.shape[0], state, H.stream_ptr())


def eval_ap(acc_scores, acc_tpmask, state, nthr):
    """KITTI R40 average precision of the accumulated detections: (ap fp64 [nthr], tp int64 [nthr]) on the device."""
    cap = acc_scores.shape[0]
    ap = torch.zeros((nthr,), dtype=torch.float64, device=acc_scores.device)
    tp = torch.zeros((nthr,), dtype=torch.int64, device=acc_scores.device)
    ws = torch.empty((H.lib().dcf_eval_ap_workspace_bytes(cap),), dtype=torch.uint8, device=acc_scores.device)
    H.call("dcf_eval_ap", _chk(acc_scores, "acc_scores"), _chk(acc_tpmask, "acc_tpmask"), _chk(state, "state"), cap, nthr, ap, tp, ws, H.stream_ptr())
    return ap, tp


# ------------------------------------------------------------------ KITTI-style protocol (eval_protocol: kitti)
def eval_det_flags(boxes, count, crt, dontcare, image_h, image_w, min_height, overlap):
    """Flag bits of the candidates boxes [n,7] (count int32 [1] valid rows): bit d iff the projected height < min_height[d], bit 3 iff
    more than `overlap` of the projected 2-D box lies in one rectangle of dontcare [D,4] (device, or None).  crt: the frame's [4,3]
    matrix as a HOST array / tensor (it travels as a kernel argument).  Returns int32 [n] (the bits of a uint32)."""
    n = boxes.shape[0]
    flags = torch.zeros((max(n, 1),), dtype=torch.int32, device=boxes.device)
    if n == 0:
        return flags[:0]
    crt = np.ascontiguousarray(crt.detach().cpu().numpy() if isinstance(crt, torch.Tensor) else crt, dtype=np.float32).reshape(12)
    mh = np.ascontiguousarray(min_height, dtype=np.float64).reshape(3)
    D = 0 if dontcare is None else dontcare.shape[0]
    H.call("dcf_eval_det_flags", _chk(boxes, "boxes"), count, n, crt, _chk(dontcare, "dontcare") if D else None, D, int(image_h), int(image_w), mh,
           float(overlap), flags, H.stream_ptr())
    return flags


def eval_iou_levels(boxes, keep, count, ref_boxes):
    """(iou_bev, iou_3d) fp64 [n,R] of the survivors against the labelled rows of ref_boxes [R,9], both from one clip; NaN elsewhere
    (rows >= count are left unwritten)."""
    n, R = boxes.shape[0], ref_boxes.shape[0]
    bev = torch.empty((n, R), dtype=torch.float64, device=boxes.device)
    i3d = torch.empty((n, R), dtype=torch.float64, device=boxes.device)
    if n and R:
        H.call("dcf_eval_iou_levels", _chk(boxes, "boxes"), _chk(keep, "keep"), count, n, _chk(ref_boxes, "ref_boxes"), R, bev, i3d, H.stream_ptr())
    return bev, i3d


def eval_match_levels(iou_bev, iou_3d, keep, count, ref_boxes, levels, flags, thresholds):
    """(tpmask, igmask) int32 [2,n] (the bits of uint32 words, bit 10 d + t): per metric, difficulty and threshold the survivors are
    true positives, ignored or neither (evalkitti.match_levels).  levels int32 [R] on the device, or None (all rows level 0)."""
    n, R = keep.shape[0], ref_boxes.shape[0]
    tpmask = torch.empty((2, max(n, 1)), dtype=torch.int32, device=keep.device)
    igmask = torch.empty((2, max(n, 1)), dtype=torch.int32, device=keep.device)
    if n == 0:
        return tpmask[:, :0], igmask[:, :0]
    if levels is not None and (levels.dtype != torch.int32 or levels.numel() != R):
        raise H.DcfError("eval_match_levels: levels must be int32 [%d]" % R)
    H.call("dcf_eval_match_levels", _chk(iou_bev, "iou_bev") if R else None, _chk(iou_3d, "iou_3d") if R else None, _chk(keep, "keep"), count, n,
           _chk(ref_boxes, "ref_boxes") if R else None, None if levels is None else _chk(levels, "levels"), R, _chk(flags, "flags"), thresholds,
           thresholds.shape[0], tpmask, igmask, H.stream_ptr())
    return tpmask, igmask


def eval_accumulate_levels(scores, tpmask, igmask, keep, count, total, ref_boxes, levels, acc_scores, acc_tpmask, acc_igmask, state):
    """Appends (score, tpmask[2], igmask[2]) of one sample's survivors, in order, at the device cursor state[0]; state int64 [8] =
    (cursor, counted rows seen at easy / moderate / hard, samples with total > len(scores), unused x 3).  acc_tpmask / acc_igmask are
    int32 [2,capacity].  The cursor counts on past the capacity; nothing is written past it."""
    n, R = scores.shape[0], ref_boxes.shape[0]
    if levels is not None and (levels.dtype != torch.int32 or levels.numel() != R):
        raise H.DcfError("eval_accumulate_levels: levels must be int32 [%d]" % R)
    if tpmask.shape != (2, n) or igmask.shape != (2, n) or acc_tpmask.shape != (2, acc_scores.shape[0]) or acc_igmask.shape != acc_tpmask.shape or state.numel() != 8:
        raise H.DcfError("eval_accumulate_levels: masks must be [2,n], accumulators [2,capacity], state int64 [8]")
    H.call("dcf_eval_accumulate_levels", _chk(scores, "scores"), _chk(tpmask, "tpmask"), _chk(igmask, "igmask"), _chk(keep, "keep"), count, total, n,
           _chk(ref_boxes, "ref_boxes") if R else None, None if levels is None else _chk(levels, "levels"), R, acc_scores, _chk(acc_tpmask, "acc_tpmask"),
           _chk(acc_igmask, "acc_igmask"), acc_scores.shape[0], state, H.stream_ptr())


def eval_ap_levels(acc_scores, acc_tpmask, acc_igmask, state, nthr):
    """KITTI R40 average precision per (metric, difficulty, threshold) over the detections not ignored there:
    (ap fp64 [2,3,nthr], tp int64 [2,3,nthr], ignored int64 [2,3,nthr]) on the device."""
    cap = acc_scores.shape[0]
    dev = acc_scores.device
    ap = torch.zeros((2, 3, nthr), dtype=torch.float64, device=dev)
    tp = torch.zeros((2, 3, nthr), dtype=torch.int64, device=dev)
    ig = torch.zeros((2, 3, nthr), dtype=torch.int64, device=dev)
    ws = torch.empty((H.lib().dcf_eval_ap_levels_workspace_bytes(cap),), dtype=torch.uint8, device=dev)
    H.call("dcf_eval_ap_levels", _chk(acc_scores, "acc_scores"), _chk(acc_tpmask, "acc_tpmask"), _chk(acc_igmask, "acc_igmask"), _chk(state, "state"), cap, nthr,
           ap, tp, ig, ws, H.stream_ptr())
    return ap, tp, ig


# ------------------------------------------------------------------ dense focal classification loss (loss_sampling: focal)
def loss_focal_workspace(B, Hh, W, device):
    """(workspace, terms [B,3]) of loss_focal for one map shape; contents free between calls on one stream."""
    nbytes = H.lib().dcf_loss_focal_workspace_bytes(B, Hh, W)
    if nbytes == 0:
        raise H.DcfError("loss_focal: bad map shape %r" % ((B, Hh, W),))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), torch.zeros((B, 3), dtype=torch.float32, device=device)


def loss_focal(cls, reg, anchors, boxes, nbox, grid, span, regress_type, alpha, gamma, eps, gain, reduction, loss, gcls, greg, terms, ws,
               deterministic=False):
    """One launch of the focal objective and its gradients.  cls [B,4,h,w] / reg [B,14,h,w] fp32 views with unit cell stride, anchors
    [2,7,h*w], boxes [B,max,>=7] fp32 and nbox int32 [B] on the device, grid = (xs, xo, ys, yo, reduced_scale); loss [1], gcls / greg
    (greg zeroed) and terms [B,3] are written.  reduction: 0 last, 1 sum, 2 mean."""
    B, _, Hh, W = cls.shape
    xs, xo, ys, yo, rs = [float(v) for v in grid]
    H.call("dcf_loss_focal_fwd_bwd_det" if deterministic else "dcf_loss_focal_fwd_bwd", cls, cls.stride(0), reg,
           reg.stride(0), anchors, _chk(boxes, "boxes"), nbox, boxes.shape[1], boxes.shape[2], B, Hh, W, xs, xo, ys, yo, rs, int(span),
           int(regress_type), float(alpha), float(gamma), float(eps), float(gain), int(reduction), loss, gcls, gcls.stride(0), greg,
           greg.stride(0), terms, ws, H.stream_ptr())
    return loss


# ------------------------------------------------------------------ IoU-based anchor assignment (loss_sampling: anchor)
def assign_anchors_workspace(B, Hh, W, max_box, device, best=False):
    """(workspace, target int32 [B,2,h*w], counts int32 [B,4], best fp64 [B,2,h*w] or None) of assign_anchors_iou for one map shape;
    the workspace's contents are free between calls on one stream."""
    nbytes = H.lib().dcf_assign_anchors_workspace_bytes(B, Hh, W, max_box)
    if nbytes == 0:
        raise H.DcfError("assign_anchors_iou: bad map shape / label rows %r" % ((B, Hh, W, max_box),))
    return (torch.empty(nbytes // 4, dtype=torch.int32, device=device), torch.empty((B, 2, Hh * W), dtype=torch.int32, device=device),
            torch.empty((B, 4), dtype=torch.int32, device=device), torch.empty((B, 2, Hh * W), dtype=torch.float64, device=device) if best else None)


def assign_anchors_iou(anchors, boxes, nbox, Hh, W, pos_iou, neg_iou, target, counts, ws, best=None):
    """Per-anchor targets by rotated bird's-eye IoU (assign.anchor_targets is the host statement): anchors [2,7,h*w] fp32, boxes
    [B,max,>=7] fp32 and nbox int32 [B] on the device; target int32 [B,2,h*w] (label row, -1 negative, -2 ignored), counts int32 [B,4] =
    (positives, ignored, positive through forcing only, void labels) and, if given, best fp64 [B,2,h*w] are written."""
    B = boxes.shape[0]
    H.call("dcf_assign_anchors_iou", _chk(anchors, "anchors"), _chk(boxes, "boxes"), _chk(nbox, "nbox"), boxes.shape[1], boxes.shape[2], B, Hh, W,
           float(pos_iou), float(neg_iou), _chk(target, "target"), None if best is None else _chk(best, "best"), _chk(counts, "counts"), ws,
           H.stream_ptr())
    return target, counts


def loss_anchor_workspace(B, Hh, W, device):
    """(workspace, terms [B,3]) of loss_anchor for one map shape; contents free between calls on one stream."""
    nbytes = H.lib().dcf_loss_anchor_workspace_bytes(B, Hh, W)
    if nbytes == 0:
        raise H.DcfError("loss_anchor: bad map shape %r" % ((B, Hh, W),))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), torch.zeros((B, 3), dtype=torch.float32, device=device)


def loss_anchor(cls, reg, anchors, boxes, target, counts, alpha, gamma, eps, gain, reduction, loss, gcls, greg, terms, ws):
    """The objective on per-anchor targets and its gradients, one launch and a fold.  cls [B,4,h,w] / reg [B,14,h,w] fp32 views with unit
    cell stride, anchors [2,7,h*w], boxes [B,max,>=7] fp32, target int32 [B,2,h*w] and counts int32 [B,4] on the device; loss [1], terms
    [B,3] and every element of gcls / greg of the computed samples are written (no zero fill needed).  reduction: 0 last, 1 sum, 2 mean."""
    B, _, Hh, W = cls.shape
    H.call("dcf_loss_anchor_fwd_bwd", cls, cls.stride(0), reg, reg.stride(0), anchors, _chk(boxes, "boxes"), boxes.shape[1], boxes.shape[2],
           _chk(target, "target"), _chk(counts, "counts"), B, Hh, W, float(alpha), float(gamma), float(eps), float(gain), int(reduction), loss,
           gcls, gcls.stride(0), greg, greg.stride(0), terms, ws, H.stream_ptr())
    return loss


# ------------------------------------------------------------------ rotated-IoU regression term (iou_loss_gain)
def loss_anchor_iou_workspace(B, Hh, W, device, iou_map=False):
    """(workspace, iou_terms [B,2], iou_map fp64 [B,2,h*w] or None) of loss_anchor_iou for one map shape; the workspace's contents are
    free between calls on one stream.  The map starts as zeros: rows of samples `loss_reduction: last` leaves out are never written."""
    nbytes = H.lib().dcf_loss_anchor_iou_workspace_bytes(B, Hh, W)
    if nbytes == 0:
        raise H.DcfError("loss_anchor_iou: bad map shape %r" % ((B, Hh, W),))
    return (torch.empty(nbytes // 8, dtype=torch.float64, device=device), torch.zeros((B, 2), dtype=torch.float32, device=device),
            torch.zeros((B, 2, Hh * W), dtype=torch.float64, device=device) if iou_map else None)


def loss_anchor_iou(reg, anchors, boxes, target, counts, kind, gain, reduction, loss, greg, iou_terms, ws, iou_map=None):
    """The IoU regression term on per-anchor targets, after loss_anchor on the same stream: reg [B,14,h,w] fp32 view with unit cell stride,
    anchors [2,7,h*w], boxes [B,max,>=7] fp32, target int32 [B,2,h*w] and counts int32 [B,4] on the device; kind 0 = 3-D, 1 = bird's-eye.
    loss [1] and the seven greg elements of every positive anchor are ADDED to, iou_terms [B,2] = (mean IoU of the positives, N_b) and, if
    given, iou_map fp64 [B,2,h*w] are written.  reduction: 0 last, 1 sum, 2 mean."""
    B, _, Hh, W = reg.shape
    H.call("dcf_loss_anchor_iou_fwd_bwd", reg, reg.stride(0), anchors, _chk(boxes, "boxes"), boxes.shape[1], boxes.shape[2], _chk(target, "target"),
           _chk(counts, "counts"), B, Hh, W, int(kind), float(gain), int(reduction), loss, greg, greg.stride(0), _chk(iou_terms, "iou_terms"),
           None if iou_map is None else _chk(iou_map, "iou_map"), ws, H.stream_ptr())
    return loss

"""Expected values of the guarded optimiser step (csrc/amp.hip) for tests/test_amp_host.py and tests/test_gpu_amp.py."""
import math

import numpy as np
import torch


def scale_schedule(found, init, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch.amp.GradScaler's update rule (torch._amp_update_scale_), restated: the (scale, growth tracker) pair after each
    step of the found_inf sequence `found`.  Products are formed in double and rounded to float, as torch's kernel does."""
    def f32(x):
        with np.errstate(over="ignore"):
            return float(np.float32(x))

    scale, tracker, out = f32(init), 0, []
    for bad in found:
        if bad:
            scale, tracker = f32(scale * backoff_factor), 0
        else:
            ok = tracker + 1
            if ok == growth_interval:
                grown = f32(scale * growth_factor)
                if math.isfinite(grown):
                    scale = grown
                tracker = 0
            else:
                tracker = ok
        out.append((scale, tracker))
    return out


def torch_schedule(found, init, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """The same sequence from torch._amp_update_scale_ itself on CPU tensors."""
    scale = torch.full((1,), init, dtype=torch.float32)
    tracker = torch.zeros(1, dtype=torch.int32)
    out = []
    for bad in found:
        torch._amp_update_scale_(scale, tracker, torch.full((1,), 1.0 if bad else 0.0), growth_factor, backoff_factor, growth_interval)
        out.append((float(scale.item()), int(tracker.item())))
    return out


def fp16_landing_scale(cfg, x, bboxes, nbox, seed, top=30):
    """The largest power of two <= 2**top at which the quantisation-aware CPU statement of the LiDAR stream
    (oracle/model_quant_ref.py, fp16 storage) seeded with that scale through oracle/loss_ref.py yields finite gradients of
    every parameter.  x [1,Cz,L,W] fp32; np.random.seed(seed) before the loss, as the train step does."""
    from oracle import loss_ref, model_quant_ref, model_ref
    sd = model_ref.make_state_dict(model_ref.lidar_state_shapes(cfg))
    anc = model_ref.anchors(cfg)
    for e in range(top, -1, -1):
        params = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
        pred = model_quant_ref.forward(params, cfg, x.clone(), torch.float16)
        np.random.seed(seed)
        loss = loss_ref.loss_total(cfg, bboxes, nbox, pred[:, 0:4], pred[:, 4:18], anc, reduction=cfg.get("loss_reduction", "last"))
        (loss * float(2 ** e)).sum().backward()
        if all(bool(torch.isfinite(p.grad).all()) for p in params.values() if p.grad is not None):
            return e
    return None

"""Drop-in counterpart of the reference's train.py: Train(config).one_step / get_loss_value.

One process per GPU (torchrun); gradients live in the model's flat arena, so data parallelism
is ONE RCCL all-reduce of that arena per step followed by ONE fused Adam launch -- instead of
the reference's single-process DDP wrapper (train.py:24, which current torch rejects).
"""
import contextlib
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import augment as AUG
from . import augment_image as AUGI
from . import ops
from . import optim as OPT
from . import paste as PST
from . import visibility as VIS
from .loss import LossTotal
from ._hip import torch_dtype as H_torch_dtype
from .model import ObjectDetection_DCF, parse_deterministic_config
from .calib import own_crts
# every block's parser lives beside its feature; the names stay importable from here
from .augment import KEYS as AUGMENT_KEYS, parse_config as parse_augment_config
from .augment_image import KEYS as IMAGE_AUGMENT_KEYS, parse_config as parse_image_augment_config
from .optim import parse_accum_config, parse_guard_config, window_factor
from .paste import parse_config as parse_paste_config


def parse_camera_mask_config(config):
    """The `camera_mask` block (visibility.py): None = off (no block, or both switches false: no buffer, no
    launch), else {"fov_crop", "paste_occlusion"}.  Unknown keys and non-boolean values raise ValueError, and so does
    paste_occlusion: true without an enabled augment_paste block with paste_image: true -- the occluders are the painted patches."""
    out = VIS.parse_config(config)
    if out is not None and out["paste_occlusion"]:
        pst = parse_paste_config(config)
        if pst is None or not pst["paste_image"]:
            raise ValueError("camera_mask.paste_occlusion needs an enabled augment_paste block with paste_image: true")
    return out


def draw_paste_plans(cfg, bank, rank, call, boxes, nums, n_points, crts, config, dropped=None):
    """The per-frame plans of one step (paste.draw) and the labels with the pasted rows behind the frame's own, all on the host:
    (plans, boxes' float32 [B, max_num_bbox, 9], nums' [B]).  cfg None (block absent or disabled): empty plans, the labels as
    they came.  dropped (camera_mask.paste_occlusion): a list; every plan then goes through visibility.drop_covering before its labels
    are appended -- a candidate whose patch would be painted over a nearer label of the frame is not pasted -- and the list
    receives the number of objects each frame lost."""
    src = np.asarray(boxes, dtype=np.float32)
    cnt = [int(v) for v in np.asarray(nums).reshape(-1)]
    hw = (int(config["image_height"]), int(config["image_width"])) if bank is None else bank["image_hw"]
    if cfg is None:
        return [PST.empty_plan(n_points[b], hw) for b in range(len(cnt))], src, cnt
    plans = [PST.draw(cfg, cfg["seed"], rank, call, b, bank, src[b], cnt[b], n_points[b], crts[b], config) for b in range(len(cnt))]
    if dropped is not None:
        drawn = plans
        plans = [VIS.drop_covering(drawn[b], src[b], cnt[b], crts[b], bank) for b in range(len(cnt))]
        dropped.extend(len(d["rows"]) - len(p["rows"]) for d, p in zip(drawn, plans))
    moved = [PST.append_labels(src[b], cnt[b], plans[b]) for b in range(len(cnt))]
    return plans, np.stack([m[0] for m in moved], 0), [m[1] for m in moved]


class FlatAdam(object):
    """Adam(lr, betas=(beta1, 0.999), eps=1e-8) of train.py:28 on the flat parameter arena.
    guard (parse_guard_config): the guarded step of csrc/amp.hip -- loss scale, non-finite skip and clipping decided on the
    device; the bias-correction count is then the device's applied-step count (step_count reads it: a synchronisation).
    recipe (optim.parse_optim_config): `lr` is then the BASE rate and call k runs at optim.lr_at(schedule, lr,
    k), k = opt_calls, the host's count of step() calls (a step the guard skips on the device still counts; the bias correction
    keeps the applied count).  With weight_decay > 0 or ema_decay set the step is dcf_adamw_ema_step (csrc/optim.hip) instead of
    dcf_adam_step / dcf_adam_step_guarded: decoupled decay on the tensors of optim.decay_bits, and `ema`, a second arena that
    follows the parameters, both in the Adam pass.  None: the launches, arguments and allocations of the plain optimiser.
    groups (optim.parse_param_groups): the step is ALWAYS dcf_adamw_ema_step_groups, whether or not decay or
    the average are configured -- group g runs at lr * lr_mult_g with decay_mul_g = 1 - lr * lr_mult_g * weight_decay, a frozen group
    keeps p, m, v and the average bit for bit and its gradient is not read.  None: exactly the calls above."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, guard=None, recipe=None, groups=None):
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self._step_count = 0
        self.m = torch.zeros_like(model.flat_params)
        self.v = torch.zeros_like(model.flat_params)
        self.guard = guard
        self.amp = ops.AmpState(model.flat_params.device, guard["scale"]) if guard is not None else None
        self.recipe = recipe
        self.opt_calls = 0
        self.ema = self.decay_bits = None
        self._ema_fresh = False
        if recipe is not None and recipe["weight_decay"] > 0.0:
            words = OPT.decay_bits(model._table.entries, model.flat_params.numel(), recipe["weight_decay_exclude"])
            self.decay_bits = torch.from_numpy(words.view(np.int64)).to(model.flat_params.device)
        if recipe is not None and recipe["ema_decay"] is not None:
            # until the first step() the average IS the parameters: weights loaded after construction are what it starts from
            self.ema = model.flat_params.detach().clone()
            self._ema_fresh = True
        self.fused = self.decay_bits is not None or self.ema is not None
        self.groups, self.group_ids = groups, None
        if groups is not None:
            n = model.flat_params.numel()
            self.group_ids = ops.AdamGroups(OPT.group_ids(model._table.entries, n, groups), len(groups) + 1, model.flat_params.device)

    def seed_ema(self):
        """Before the first optimiser call (or a checkpoint) the average follows the parameters; no-op afterwards."""
        if self._ema_fresh:
            self.ema.copy_(self.model.flat_params.detach())

    def lr_at(self, k):
        return OPT.lr_at(self.recipe["schedule"], self.lr, k) if self.recipe is not None else self.lr

    def group_rates(self, k):
        """Rates of optimiser call k per parameter-group id (host floats; [the one rate] without param_groups)."""
        return OPT.group_rates(self.groups, self.lr_at(k))

    @property
    def step_count(self):
        if self.amp is not None:
            return int(self.amp.applied_steps.item())
        return self._step_count

    @step_count.setter
    def step_count(self, value):
        if self.amp is not None:
            self.amp.applied_steps.fill_(int(value))
        else:
            self._step_count = int(value)

    def zero_grad(self):
        pass  # the backward pass overwrites the gradient arena

    def step(self, gscale=1.0):
        k = self.opt_calls
        self.opt_calls = k + 1
        lr = self.lr_at(k)                      # by value into the launches below: the step runs outside the captured graphs
        decay_mul, omd = 1.0, 0.0
        if self.fused:
            decay_mul = 1.0 - float(lr) * self.recipe["weight_decay"]         # AdamW's param.mul_(1 - lr * wd); rounded to fp32 at the call
            if self.ema is not None:
                self.seed_ema()
                self._ema_fresh = False
                omd = 1.0 - OPT.ema_decay_at(self.recipe, k)
        if self.groups is not None:
            return self._step_groups(lr, gscale, omd)
        if self.amp is not None:
            self._guard_scan(lr, gscale)
            if self.fused:
                ops.adamw_ema_step(self.model.flat_params, self.model.flat_grads, self.m, self.v, lr, self.betas[0], self.betas[1],
                                   self.eps, 0, gscale, decay_mul, self.decay_bits, self.ema, omd, self.amp)
            else:
                ops.adam_step_guarded(self.model.flat_params, self.model.flat_grads, self.m, self.v, self.betas[0], self.betas[1],
                                      self.eps, self.amp)
            return
        self._step_count += 1
        if self.fused:
            ops.adamw_ema_step(self.model.flat_params, self.model.flat_grads, self.m, self.v, lr, self.betas[0], self.betas[1],
                               self.eps, self._step_count, gscale, decay_mul, self.decay_bits, self.ema, omd)
        else:
            ops.adam_step(self.model.flat_params, self.model.flat_grads, self.m, self.v, lr, self.betas[0], self.betas[1],
                          self.eps, self._step_count, gscale)

    def _guard_scan(self, lr, gscale):
        """The guarded step's two launches in front of the Adam pass: the scan of the gradient arena, then the device-side decision
        (skip, clip factor, next loss scale)."""
        g = self.guard
        ops.grad_stats(self.model.flat_grads, self.amp)
        ops.amp_update(self.amp, gscale, g["mode"] == "dynamic", g["growth_factor"], g["backoff_factor"], g["growth_interval"],
                       g["max_norm"], lr, self.betas[0], self.betas[1])

    def _step_groups(self, lr, gscale, omd):
        """step() with param_groups: the guard's scan and norm run over the WHOLE arena (a frozen tensor whose gradient the backward
        still computes counts; the frozen trunk prefix contributes exact zeros), then the one grouped pass."""
        wd = self.recipe["weight_decay"] if self.recipe is not None else 0.0
        table = OPT.group_table(self.groups, lr, wd)
        if self.amp is not None:
            self._guard_scan(lr, gscale)
            step = 0
        else:
            self._step_count += 1
            step = self._step_count
        ops.adamw_ema_step_groups(self.model.flat_params, self.model.flat_grads, self.m, self.v, lr, self.betas[0], self.betas[1], self.eps,
                                  step, self.group_ids, table, gscale, self.decay_bits, self.ema, omd, self.amp)

    def state_dict(self):
        sd = {"step": self.step_count, "m": self.m, "v": self.v, "opt_calls": self.opt_calls}
        if self.ema is not None:
            self.seed_ema()
            sd["ema"] = self.ema
        return sd

    def load_state_dict(self, sd):
        """A state written before the recipe existed has neither `opt_calls` nor `ema`: the clock then continues at the step
        count and the average starts from the parameters as they are now (load the model first)."""
        self.step_count = int(sd["step"])
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.opt_calls = int(sd.get("opt_calls", sd["step"]))
        if self.ema is not None:
            self.ema.copy_(sd["ema"] if sd.get("ema") is not None else self.model.flat_params.detach())
            self._ema_fresh = False


def world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def this_rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _through_host(t):
    """gloo with a device tensor (DCF_DIST_BACKEND=gloo: several ranks sharing one GPU in the functional tests): the
    collective runs on a host copy.  RCCL (the product path) takes the device tensor itself."""
    return t.is_cuda and dist.get_backend() == "gloo"


def allreduce_grads(flat_grads):
    """Sum the gradient arena over ranks (RCCL over xGMI on the GPU box, gloo in the CPU tests)."""
    if world() > 1:
        if _through_host(flat_grads):
            h = flat_grads.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            flat_grads.copy_(h)
        else:
            dist.all_reduce(flat_grads, op=dist.ReduceOp.SUM)
    return world()


def broadcast_from_rank0(t):
    if world() > 1:
        if _through_host(t):
            h = t.cpu()
            dist.broadcast(h, 0)
            t.copy_(h)
        else:
            dist.broadcast(t, 0)


class Train(nn.Module):
    # gradient accumulation, off: no open window, and the bucket hook adds nothing (one_step sets these per call)
    accum, accum_buf, _accum_index, _accum_closing, _accum_added = None, None, 0, False, 0

    def __init__(self, config):
        super(Train, self).__init__()
        self.config = config
        # deterministic: true -- one_step as a pure function of the state and the frames (per rank); bad combinations raise here
        self.deterministic = parse_deterministic_config(config)
        # gradient accumulation (grad_accum_steps / grad_accum_reduce; None = off, the default): one optimiser step per window of k
        # one_step calls.  The accumulator (below) is a second gradient arena at a fixed address, filled outside the captured graphs;
        # the count of the open window's micro-steps lives on the host
        self.accum = parse_accum_config(config)
        self.loss_total = LossTotal(config)
        self.model = ObjectDetection_DCF(config).cuda()
        self.loss_value = None
        # guarded optimiser step (loss_scale / grad_clip_norm; None = the plain Adam step, the default)
        self.guard = parse_guard_config(config)
        # training recipe (lr_schedule / weight_decay / ema_decay; None = the constant-rate Adam step, the default)
        self.recipe = OPT.parse_optim_config(config)
        # fine-tuning the camera stream (finetune.py; all off by default).  fusion.image_pretrained: a
        # torchvision-layout trunk, loaded on every rank before sync_replicas().  param_groups: per-group rate multipliers and frozen
        # groups in the optimiser pass; the longest frozen PREFIX of the camera trunk (stem, then whole stages) also leaves the
        # backward plan -- frozen_range = its arena range (exact zeros in the gradient arena), None when there is none
        pre = (config.get("fusion") or {}).get("image_pretrained", None)
        if pre is not None:
            from . import finetune as FT
            FT.load_image_trunk_file(self.model, pre, self.model.image_input_order)
        keys = [e[0] for e in self.model._table.entries]
        self.param_groups = OPT.parse_param_groups(config.get("param_groups", None), keys)
        units = OPT.frozen_trunk_units(keys, self.param_groups)
        self.frozen_range = self.model.set_frozen_trunk(units) if units else None
        self.optimizer = FlatAdam(self.model, config["learning_rate"], (config["beta1"], 0.999), guard=self.guard, recipe=self.recipe,
                                  groups=self.param_groups)
        self._ema_swapped = False
        self.sync_replicas()
        self._side = None
        self.static_geometry = bool(config.get("static_geometry", True))
        self._geo_sets, self._geo_slot = {}, 0
        # data parallel: all-reduce the LiDAR + fusion gradient bucket under the camera stream's backward.  True (default) =
        # when the world has more than one rank; "force" = also in a one-rank process group (the functional test of the
        # bucketed path on RCCL with the one GPU a test box has, tests/test_gpu_dp.py); False = one all-reduce at the end.
        ov = config.get("overlap_allreduce", os.environ.get("DCF_OVERLAP_ALLREDUCE", "1") != "0")
        self.overlap_force = ov == "force"
        self.overlap_allreduce = bool(ov)
        # factor applied to every rank's gradient INSIDE the RCCL reduction (ncclRedOp PreMulSum) and undone in the Adam step's
        # gradient scale -- e.g. a power of two that lifts small fp16 gradients over the exchange; None = plain sum
        self.allreduce_premul = config.get("allreduce_premul", None)
        # grad_bucket_dtype: "bf16" exchanges the gradient buckets as bf16 (half the bytes over xGMI: 48 MB instead of 96 MB per
        # step at cfg2; every rank rounds its own gradient once, the sum of the rounded values is widened back to fp32 for Adam);
        # "f32" (default) exchanges the fp32 arena itself
        self.grad_bucket_dtype = str(config.get("grad_bucket_dtype", os.environ.get("DCF_GRAD_BUCKET_DTYPE", "f32"))).lower()
        if self.grad_bucket_dtype not in ("f32", "fp32", "bf16"):
            raise ValueError("grad_bucket_dtype must be f32 or bf16 (got %r)" % (self.grad_bucket_dtype,))
        self._g16 = None
        self._pending, self._reduced, self._widen = [], 0, []
        # train-time BEV augmentation (augment.py; None = off, the default): one_step_raw draws the frames' parameters from
        # (seed, rank, aug_calls, frame) -- no generator state, the count is all a checkpoint has to carry
        self.augment = parse_augment_config(config)
        self.aug_calls = 0
        # train-time camera image augmentation (augment_image.py; None = off, the default: no buffer, no launch).  It draws from
        # the same (seed, rank, aug_calls, frame) on hash streams of its own; the augmented image lives in ONE persistent buffer,
        # written and read on the compute stream
        self.image_augment = parse_image_augment_config(config)
        self._aug_image = None
        # train-time object pasting (paste.py, objbank.py; None = off, the default: no bank, no buffer, no launch).  The third block
        # on the same (seed, rank, aug_calls, frame); the bank's points and patch bytes are uploaded here, once; last_paste = the
        # accepted bank rows per frame of the last step (host lists, for logs)
        self.paste = parse_paste_config(config)
        self._paste_bank, self._paste_dev, self._paste_image_buf = None, None, None
        self.last_paste = []
        if self.paste is not None:
            from . import objbank
            try:
                self._paste_bank = objbank.load(self.paste["bank"])
            except OSError as e:
                raise ValueError("augment_paste.bank: cannot read %r (%s)" % (self.paste["bank"], e))
            PST.check_bank(self._paste_bank, (config["image_height"], config["image_width"]) if self.paste["paste_image"] else None)
            dev = self.model.flat_params.device
            self._paste_dev = (torch.from_numpy(self._paste_bank["points"]).to(dev), torch.from_numpy(self._paste_bank["patch"]).to(dev))
        # the camera visibility mask (visibility.py; None = off, the default: no buffer, no launch).  fov_crop acts wherever
        # geometry_async runs (train and evaluation), paste_occlusion where pasting does; last_masked = per frame of the last
        # paste step (patch records that act as occluders, objects dropped by visibility.drop_covering), host counts for logs
        self.camera_mask = parse_camera_mask_config(config)
        self.last_masked = []
        # the accumulator of gradient accumulation: allocated only when a window holds more than one micro-step
        self.accum_buf = torch.empty_like(self.model.flat_grads.detach()) if self.accum is not None else None
        self._accum_index = 0
        self._accum_closing, self._accum_added = False, 0

    def sync_replicas(self):
        """Identical replicas: rank 0's parameters, buffers, optimiser moments and step count win (called at construction;
        call it again after loading weights or a checkpoint on rank 0 only)."""
        for t in (self.model.flat_params, self.model._bufflat, self.optimizer.m, self.optimizer.v):
            broadcast_from_rank0(t)
        if self.optimizer.ema is not None:       # the weight average, and below the clock of the schedule and of the average
            self.optimizer.seed_ema()
            broadcast_from_rank0(self.optimizer.ema)
        if world() > 1:
            oc = torch.tensor([self.optimizer.opt_calls], dtype=torch.int64)
            if dist.get_backend() != "gloo":
                oc = oc.to(self.model.flat_params.device)
            dist.broadcast(oc, 0)
            self.optimizer.opt_calls = int(oc.item())
        if self.optimizer.amp is not None:       # loss scale, growth tracker and step counters (the applied count included)
            broadcast_from_rank0(self.optimizer.amp.raw)
        elif world() > 1:                        # Adam's bias correction depends on it
            sc = torch.tensor([self.optimizer.step_count], dtype=torch.int64)
            if dist.get_backend() != "gloo":
                sc = sc.to(self.model.flat_params.device)
            dist.broadcast(sc, 0)
            self.optimizer.step_count = int(sc.item())

    def _geo_set(self, B, mp, fast, dims):
        """Persistent device buffers of the per-step geometry, two sets used in turn: a step's geometry is produced on the side
        stream while the previous step's backward may still read its own set.  One zero-fill per step (the projection
        outputs are dense-packed and zero-padded, data_import_carla.py:263-266) instead of a dozen allocations + fills, and
        fixed addresses, so that captured graphs can read the geometry without staging copies."""
        self._geo_slot ^= 1
        key = (B, mp, fast, self._geo_slot)
        st = self._geo_sets.get(key)
        if st is None:
            Cz, L, W = dims
            dev = self.model.flat_params.device
            st = {"slot": self._geo_slot, "free_event": None}
            if fast:
                from ._hip import torch_dtype
                st["x_lidar"] = torch.empty((B, L, W, Cz), dtype=torch_dtype(self.model.dtype), device=dev)
            else:
                st["x_lidar"] = torch.empty((B, Cz, L, W), dtype=torch.float32, device=dev)
            st["proj"] = torch.zeros((B * mp * 5 + 16,), dtype=torch.float32, device=dev)        # [xyz | uv | counts]
            st["xyz"] = st["proj"][:B * mp * 3].view(B, mp, 3)
            st["uv"] = st["proj"][B * mp * 3:B * mp * 5].view(B, mp, 2)
            st["cnt"] = st["proj"][B * mp * 5:B * mp * 5 + B].view(torch.int32)
            st["cnt_host"] = torch.empty(B, dtype=torch.int32).pin_memory()
            if self.model.fusion_enabled:
                st["fusion"] = self.model.fusion_buffers(B, mp, dev)
            self._geo_sets[key] = st
        return st

    def geometry_async(self, frame_geometry, points_list, crts=None, wait_event=None, augment=None, image_augment=None, paste=None):
        """Per-frame geometry (voxelise, project, KNN of the fusion sites) on a side HIP stream, so that these
        small latency-bound kernels overlap the camera stream's convolutions on the compute stream.
        Returns (x_lidar [B,Cz,L,W], geom) where geom carries the events the engine waits on.
        crts: optional per-frame [4,3] projection matrices (KITTI calibrates every frame).
        wait_event: event the side stream has to wait for before it reads the points (FrameLoader's H2D copies).
        augment: optional per-frame parameters (augment.draw): the side stream first writes the augmented points (dropped ones
        as +inf rows, which every range test rejects) into a persistent buffer of the geometry set, and everything below runs
        on those, with projection matrices that keep every point on the pixel of its original (augment.compose_crt).
        image_augment: optional per-frame parameters (augment_image.draw) of an image that was zoomed / shifted / flipped: the
        projection matrices (after the BEV composition) move every point's pixel along (augment_image.compose_crt_image); points
        that now project outside the image fail the projection kernel's limit test as it is.
        paste: optional per-frame plans (paste.draw): the side stream FIRST writes the pasted frames (scene points inside a pasted
        box as +inf rows, the bank's points appended) into a persistent buffer of the geometry set; `augment` then reads that
        buffer -- its point-drop hash simply runs over the longer frame.
        The returned tensors live in one of two persistent buffer sets (config static_geometry, default on): they stay
        valid until the second-next call."""
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
        if wait_event is not None:
            self._side.wait_event(wait_event)
        Cz, L, W = frame_geometry.grid.dims
        Bn, mp = len(points_list), int(frame_geometry.config["max_num_pc"])
        # 16-bit compute types: the voxeliser writes the engine's input image ([B,L,W,Cz] in that type) directly -- no fp32
        # grid, no transpose (the model recognises it by its dtype); f32 keeps the reference's [B,Cz,L,W] grid
        fast = self.model.dtype != 0 and frame_geometry.voxel_mode == 0 and Bn <= 8
        direct = self.static_geometry and all(p.shape[0] <= mp for p in points_list)
        st = None
        if direct:
            # (allocated under the side stream: memory handed out by the caching allocator is only safe to write on the stream
            # it was requested on -- a block the compute stream has just released may still be in use by its queued kernels)
            with torch.cuda.stream(self._side):
                st = self._geo_set(Bn, mp, fast, (Cz, L, W))
        if st is not None:
            if st["free_event"] is not None:
                self._side.wait_event(st["free_event"])        # the step that last read this set has finished with it
                st["free_event"] = None
            elif st.get("used"):
                self._side.wait_stream(main)                   # handed out before, never consumed by one_step: be conservative
            st["used"] = True
        with torch.cuda.stream(self._side):
            pcs, uvs, cnts = [], [], []
            points_list, crts = self._point_stages(frame_geometry, points_list, crts, st, mp, paste, augment, image_augment)
            if st is not None:
                x_lidar = st["x_lidar"]
                st["proj"].zero_()
                xyz_all, uv_all, cnt_all = st["xyz"], st["uv"], st["cnt"]
            else:
                x_lidar = torch.empty((Bn, L, W, Cz), dtype=H_torch_dtype(self.model.dtype), device="cuda") if fast else \
                    torch.empty((Bn, Cz, L, W), dtype=torch.float32, device="cuda")
                xyz_all = torch.zeros((Bn, mp, 3), dtype=torch.float32, device="cuda")
                uv_all = torch.zeros((Bn, mp, 2), dtype=torch.float32, device="cuda")
                cnt_all = torch.zeros((Bn,), dtype=torch.int32, device="cuda")
            # projection first: its valid-point counts go to the host (pinned, asynchronous) while the voxeliser and the KNN
            # still run; the engine sizes the per-point fusion tensors by them instead of max_num_pc (Plan._fusion_rows)
            # the frames' projections land side by side in batch tensors (no per-frame allocations, no stack copies)
            inplace = True
            if getattr(frame_geometry, "project_batch", None) is not None and frame_geometry.project_batch(points_list, crts, xyz_all, uv_all, cnt_all):
                pass                                    # every frame in one launch per phase (count / scan / scatter)
            else:
                for b, pts in enumerate(points_list):
                    pc, uv, cnt = frame_geometry.project(pts, crt=None if crts is None else crts[b],
                                                         out=(xyz_all[b], uv_all[b], cnt_all[b:b + 1]))
                    inplace = inplace and pc.data_ptr() == xyz_all[b].data_ptr()
                    pcs.append(pc); uvs.append(uv); cnts.append(cnt)
            cnt_dev = cnt_all if inplace else torch.cat(cnts, 0)
            cnt_host = st["cnt_host"] if st is not None else torch.empty(Bn, dtype=torch.int32).pin_memory()
            cnt_host.copy_(cnt_dev, non_blocking=True)
            ev_cnt = torch.cuda.Event()
            ev_cnt.record()
            frame_geometry.voxelize_batch(points_list, x_lidar, self.model.dtype if fast else None)   # written in place, frames side by side
            ev_vox = torch.cuda.Event()
            ev_vox.record()
            geom = None
            if self.model.fusion_enabled:
                fb = st.get("fusion") if st is not None else None
                if inplace:
                    geom = self.model.fusion_geometry(xyz_all, uv_all, cnt_all, bufs=fb)
                else:                                   # a frame with more than max_num_pc points: the copying path
                    geom = self.model.fusion_geometry(torch.stack(pcs, 0), torch.stack(uvs, 0), cnt_dev)
                ev = torch.cuda.Event()
                ev.record()
                geom["event"] = ev
                geom["cnt_host"], geom["cnt_event"] = cnt_host, ev_cnt
                self.model.fusion_inverse(geom, bufs=fb if inplace else None)        # needed by the backward only: its own event
                ev_inv = torch.cuda.Event()
                ev_inv.record()
                geom["inv_event"] = ev_inv
            else:
                geom = {}
            geom["voxel_event"] = ev_vox
        if st is not None:
            geom["_set"] = st                # one_step records the set's free event when the step has consumed it
            geom["static"] = inplace
        else:
            # tensors born on the side stream are consumed on the compute stream
            x_lidar.record_stream(main)
            born = [geom.get("xyz"), geom.get("uv"), geom.get("cnt")] + list(geom.get("idx") or [])
            born += list(geom.get("inv") or [])
            born += list((geom.get("cam_inv") or ())[:2])
            for t in born:
                if t is not None:
                    t.record_stream(main)
        return x_lidar, geom

    @staticmethod
    def _stage_buffers(st, name, src, mp, rows=None):
        """Where a point stage writes the frames `src`: views of the geometry set's persistent [B, max_num_pc, 3] buffer st[name] --
        fixed addresses; allocated on first use, under the caller's side-stream context (the comment in geometry_async says why)
        -- or, without a set (a frame over max_num_pc), new tensors.  rows None (mask, augment): frame b gets [b, :n_b] of the
        buffer, or a tensor like src[b].  rows (paste, whose frames grow to rows[b]): whole [b] rows of the buffer, and only when
        max(rows) <= max_num_pc, else tensors of rows[b] rows -- the row count of an output is the capacity the kernel is told."""
        if st is None or (rows is not None and max(rows) > mp):
            return [torch.empty((p.shape[0] if rows is None else rows[b], 3), dtype=torch.float32, device=p.device) for b, p in enumerate(src)]
        if name not in st:
            st[name] = torch.empty((len(src), mp, 3), dtype=torch.float32, device=src[0].device)
        return [st[name][b] if rows is not None else st[name][b, :p.shape[0]] for b, p in enumerate(src)]

    def _point_stages(self, frame_geometry, points_list, crts, st, mp, paste, augment, image_augment):
        """The point stages of geometry_async, on the side stream in front of the projection: paste, then the camera mask, then the
        BEV transform, each reading what the one before wrote; and the projection matrices under the two augmentations.  Returns
        (points_list, crts)."""
        Bn = len(points_list)
        for name, per_frame in (("paste", paste), ("augment", augment), ("image_augment", image_augment)):
            if per_frame is not None and len(per_frame) != Bn:
                raise ValueError("%s: %d %s for %d frames" % (name, len(per_frame), "plans" if name == "paste" else "parameter sets", Bn))
        if paste is not None:
            if self._paste_dev is None:
                raise ValueError("paste: the trainer was built without an object bank (augment_paste)")
            src = [frame_geometry._pts(p) for p in points_list]
            rows = [int(p.shape[0]) + int(q["append"][:, 1].sum()) for p, q in zip(src, paste)]
            points_list = ops.paste_points_batch(src, list(paste), self._paste_dev[0], self._stage_buffers(st, "paste", src, mp, rows))
        if self.camera_mask is not None:
            points_list = self._camera_mask_points(frame_geometry, points_list, crts, paste, st, mp)
        if augment is not None:
            src = [frame_geometry._pts(p) for p in points_list]
            points_list = ops.augment_points_batch(src, list(augment), self._stage_buffers(st, "aug", src, mp))
            crts = [AUG.compose_crt(m, q) for m, q in zip(own_crts(frame_geometry.crt, crts, Bn), augment)]
        if image_augment is not None:
            crts = [AUGI.compose_crt_image(m, q) for m, q in zip(own_crts(frame_geometry.crt, crts, Bn), image_augment)]
        return points_list, crts

    def _camera_mask_points(self, frame_geometry, points_list, crts, paste, st, mp):
        """The camera visibility mask of geometry_async, on the side stream behind the paste launch and in
        front of `augment`: every frame under its OWN, un-augmented matrix -- augment.compose_crt keeps every point on the pixel of
        its original, so the decision holds under the BEV and image blocks.  Pasted frames (buffers of this call) are masked in
        place; the loader's staging views are never written: their masked copy goes to a persistent [B, max_num_pc, 3] buffer of
        the geometry set, or -- a frame over max_num_pc, as for `augment` -- to new tensors."""
        cm, Bn = self.camera_mask, len(points_list)
        own = own_crts(frame_geometry.crt, crts, Bn)
        occ = None
        if cm["paste_occlusion"] and paste is not None:
            occ = [VIS.occluders(paste[b], self._paste_bank, own[b]) for b in range(Bn)]
            if not any(len(q) for q in occ):
                occ = None
        if not cm["fov_crop"] and occ is None:
            return points_list
        src = [frame_geometry._pts(p) for p in points_list]
        dst = src if paste is not None else (None if st is None else self._stage_buffers(st, "mask", src, mp))
        return frame_geometry.mask_points(src, own, cm["fov_crop"], occ, out=dst)

    def _predict(self, lidar_voxel, camera_image, extra):
        pred = self.model(lidar_voxel, camera_image, **extra)
        return torch.split(pred, [4, 14, 14], dim=1)

    def _bucket_ready(self, ranges):
        """Backend hook (world size > 1): arena ranges whose gradients are final.  Their all-reduce starts now -- RCCL runs it
        on its own stream behind the finalisation launch, under whatever the backward still has to do -- and is waited for
        before the optimiser step."""
        g = self.model.flat_grads
        for a, b in ranges:
            if b <= a:
                continue
            seg = g[a:b]
            if self._accum_closing:
                # the window's closing micro-step: the range's earlier micro-gradients come in first (behind the finalisation launch,
                # same stream, in front of the bf16 cast), so that the collective below carries the window's sum
                ops.grad_accumulate(seg, self.accum_buf[a:b], 1)
                self._accum_added += b - a
            if self.grad_bucket_dtype == "bf16":
                # the bucket goes out in bf16: rounded here (behind the finalisation launch, same stream), summed by the collective,
                # widened back into the fp32 arena once the collective is done (one_step, before the optimiser step)
                from . import _hip as H
                if self._g16 is None or self._g16.numel() != g.numel():
                    self._g16 = torch.empty(g.numel(), dtype=torch.bfloat16, device=g.device)
                seg16 = self._g16[a:b]
                H.call("dcf_cast", H.F32, seg, H.BF16, seg16, b - a, H.stream_ptr())
                self._widen.append((a, b))
                if _through_host(seg16):
                    h = seg16.cpu()
                    dist.all_reduce(h, op=dist.ReduceOp.SUM)
                    seg16.copy_(h)
                else:
                    self._pending.append(dist.all_reduce(seg16, op=dist.ReduceOp.SUM, async_op=True))
            elif _through_host(seg):
                h = seg.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM)
                seg.copy_(h)
            else:
                op = dist.ReduceOp.SUM if self.allreduce_premul is None else dist._make_nccl_premul_sum(float(self.allreduce_premul))
                self._pending.append(dist.all_reduce(seg, op=op, async_op=True))
            self._reduced += b - a

    def one_step(self, lidar_voxel, camera_image, object_data, num_ref_box, **extra):
        if self._ema_swapped:
            raise RuntimeError("one_step inside ema_weights(): the parameter arena holds the averaged weights")
        pred_cls, pred_reg, _ = self._predict(lidar_voxel, camera_image, extra)
        self.loss_value = self.loss_total(object_data, num_ref_box, pred_cls, pred_reg)
        self.optimizer.zero_grad()
        n = world()
        grouped = dist.is_available() and dist.is_initialized()
        overlap = ((n > 1 or (self.overlap_force and grouped)) and self.overlap_allreduce and not self.model.graphs_wanted(lidar_voxel.shape[0])
                   and self.model._backend is not None)
        # gradient accumulation: micro-step j of its window; only the closing one exchanges gradients and reaches the optimiser
        j = self._accum_index + 1
        closing = self.accum is None or j >= self.accum["steps"]
        overlap = overlap and closing
        premul = 1.0
        self._pending, self._reduced, self._widen = [], 0, []
        self._accum_closing, self._accum_added = closing and j > 1, 0
        if overlap:
            self.model._backend.bucket_hook = self._bucket_ready
        try:
            if self.optimizer.amp is not None:
                # seeded with the device's loss scale: a one-element multiply, no read on the host (_FusedLoss.backward scales its
                # gradient maps by the incoming gradient; under hip_graphs they reach the captured backward through its static buffer)
                (self.loss_value * self.optimizer.amp.scale_next).backward()
            else:
                self.loss_value.backward()
        finally:
            if overlap:
                self.model._backend.bucket_hook = None
            self._accum_closing = False
        if not closing:
            # acc = g (the window's first micro-step) or acc += g: the left fold S_j = S_(j-1) + g_j.  No collective, no scan of
            # the gradient, no optimiser launch; parameters, moments, clocks and the average stay where they are
            ops.grad_accumulate(self.accum_buf, self.model.flat_grads, 0 if j == 1 else 1)
            self._accum_index = j
            self._release_geometry(extra)
            return
        if j > 1 and self._accum_added != self.model.flat_grads.numel():
            if self._accum_added:
                raise RuntimeError("gradient buckets added the accumulator to %d of %d elements" % (self._accum_added, self.model.flat_grads.numel()))
            ops.grad_accumulate(self.model.flat_grads, self.accum_buf, 1)        # g += acc: the arena now holds the window's sum
        self._accum_index = 0
        if overlap and self._reduced == self.model.flat_grads.numel():
            for w in self._pending:
                w.wait()
            if self._widen:                         # bf16 buckets: the summed values back into the fp32 arena
                from . import _hip as H
                for a, b in self._widen:
                    H.call("dcf_cast", H.BF16, self._g16[a:b], H.F32, self.model.flat_grads[a:b], b - a, H.stream_ptr())
            elif self.allreduce_premul is not None and not _through_host(self.model.flat_grads):
                premul = float(self.allreduce_premul)
        else:                                      # single rank, captured graphs, or a backward that skipped the buckets
            for w in self._pending:
                w.wait()
            if self._reduced:
                raise RuntimeError("gradient buckets covered %d of %d elements" % (self._reduced, self.model.flat_grads.numel()))
            allreduce_grads(self.model.flat_grads)
        if self.accum is None:
            self.optimizer.step(1.0 / (n * premul))
        else:                                      # the window's 1 / j (mean) rides in the gradient scale, by value
            self.optimizer.step((1.0 / (n * premul)) * window_factor(self.accum, j))
        self._release_geometry(extra)

    def _release_geometry(self, extra):
        st = (extra.get("geom") or {}).get("_set")
        if st is not None:                         # the geometry buffers of this step may be refilled from here on
            st["free_event"] = torch.cuda.Event()
            st["free_event"].record()

    # ------------------------------------------------------------------ gradient accumulation
    def accum_index(self):
        """Micro-steps gathered in the open window (host int, no device read): 0 at a window boundary, and always with accumulation off."""
        return self._accum_index

    def finish_window(self):
        """Close a short window: the optimiser step with the j micro-steps gathered so far (`mean` divides by j), through the same
        exchange and optimiser calls as a full one -- the exchange is one all-reduce of the whole fp32 arena, since no backward
        runs here to overlap with.  No-op at a boundary and with accumulation off."""
        j = self._accum_index
        if self.accum is None or j == 0:
            return
        if self._ema_swapped:
            raise RuntimeError("finish_window inside ema_weights(): the parameter arena holds the averaged weights")
        ops.grad_accumulate(self.model.flat_grads, self.accum_buf, 0)            # the arena held g_j alone: it now holds S_j
        self._accum_index = 0
        n = allreduce_grads(self.model.flat_grads)
        self.optimizer.step((1.0 / n) * window_factor(self.accum, j))

    def one_step_raw(self, frame_geometry, batch):
        """One train step from a FrameLoader batch (raw points + image in HBM): the sample pipeline, geometry on the side stream, then
        one_step.  Every block of the pipeline is one `if`; all of them draw at the step's one call count, which ticks once when any
        of them drew (the camera mask draws nothing).  Everything is pasted in the un-augmented frame: the
        labels get the pasted rows before augment.transform_boxes moves them, the side stream writes the pasted points in front of
        the mask and the BEV transform, and the patches are painted (compute stream) in front of the image transform."""
        batch.wait()
        call = self.aug_calls
        points, crts, image = batch["points"], batch.get("crt"), batch["image"]
        boxes, nums, plans, params, iparams = batch["bboxes"], batch["num_bboxes"], None, None, None
        if self.paste is not None:
            plans, boxes, nums = self._draw_paste(frame_geometry, points, crts, boxes, nums, call)
        if self.augment is not None:
            params, boxes, nums = self._draw_augment(frame_geometry, boxes, nums, call)
        if self.paste is not None and self.paste["paste_image"]:
            image = self._paste_image(image, plans)
        if self.image_augment is not None:
            image, iparams = self._augment_image(image, call)
        if not (plans is None and params is None and iparams is None):
            self.aug_calls = call + 1
        x_lidar, geom = self.geometry_async(frame_geometry, points, crts=crts, wait_event=batch.event, augment=params, image_augment=iparams,
                                            paste=plans)
        self.one_step(x_lidar, image, boxes, nums, geom=geom)

    def _draw_paste(self, frame_geometry, points, crts, boxes, nums, call):
        """This step's per-frame paste plans (draw_paste_plans at `call`, every frame under its own matrix) and the labels with the
        pasted rows appended (host tensors); last_paste / last_masked keep what the logs print."""
        dropped = [] if (self.camera_mask is not None and self.camera_mask["paste_occlusion"]) else None
        plans, new_boxes, new_nums = draw_paste_plans(self.paste, self._paste_bank, this_rank(), call, boxes.detach().cpu().numpy(),
                                                      torch.as_tensor(nums).numpy(), [int(p.shape[0]) for p in points],
                                                      own_crts(frame_geometry.crt, crts, len(points)), frame_geometry.config, dropped=dropped)
        self.last_paste = [list(p["rows"]) for p in plans]
        if dropped is not None:
            self.last_masked = [(len(p["patches"]), d) for p, d in zip(plans, dropped)]
        return plans, torch.from_numpy(new_boxes).to(boxes.dtype), torch.tensor(new_nums, dtype=torch.as_tensor(nums).dtype)

    def _paste_image(self, image, plans):
        """The batch's uint8 [B,3,H,W] image with this step's patches painted in: one launch on the compute stream -- the stream of
        its consumer (`_augment_image` or the model), so no events -- into the trainer's one persistent buffer (allocated on first
        use, re-made when the shape changes); the batch's own image, a view of the loader's staging set, is not written."""
        if image.dtype != torch.uint8 or image.dim() != 4 or not image.is_cuda:
            raise ValueError("augment_paste needs the batch's image as a uint8 [B,3,H,W] device tensor (got %s %s)" % (image.dtype, tuple(image.shape)))
        if tuple(int(v) for v in image.shape[2:]) != tuple(int(v) for v in self._paste_bank["image_hw"]):
            raise ValueError("augment_paste: the bank holds patches of %s images, the batch's are %s"
                             % (tuple(int(v) for v in self._paste_bank["image_hw"]), tuple(image.shape[2:])))
        buf = self._paste_image_buf
        if buf is None or buf.shape != image.shape or buf.device != image.device:
            buf = self._paste_image_buf = torch.empty(tuple(image.shape), dtype=torch.uint8, device=image.device)
        return ops.paste_patches_batch(image.contiguous(), plans, self._paste_dev[1], buf)

    def _augment_image(self, image, call):
        """This step's per-frame image parameters (augment_image.draw at `call`) and the augmented uint8 [B,3,H,W] image: one launch
        on the compute stream -- the stream of its consumer, so no events -- into the trainer's one persistent buffer (allocated
        on first use, re-made when the shape changes).  Outside the captured graphs: a replay copies it into its static image
        buffer as it does any image."""
        if image.dtype != torch.uint8 or image.dim() != 4 or not image.is_cuda:
            raise ValueError("augment_image needs the batch's image as a uint8 [B,3,H,W] device tensor (got %s %s)" % (image.dtype, tuple(image.shape)))
        Bn, _, Hh, Ww = (int(v) for v in image.shape)
        cfg, rank = self.image_augment, this_rank()
        iparams = [AUGI.draw(cfg, cfg["seed"], rank, call, b, Ww, Hh) for b in range(Bn)]
        if self._aug_image is None or self._aug_image.shape != image.shape or self._aug_image.device != image.device:
            self._aug_image = torch.empty(tuple(image.shape), dtype=torch.uint8, device=image.device)
        ops.augment_image_batch(image.contiguous(), iparams, self._aug_image)
        return self._aug_image, iparams

    def _draw_augment(self, frame_geometry, boxes, nums, call):
        """This step's per-frame augmentation parameters (augment.draw at `call`) and the labels under them (host tensors of
        max_num_bbox rows: no device read, no synchronisation)."""
        Bn, rank = int(boxes.shape[0]), this_rank()
        params = [AUG.draw(self.augment, self.augment["seed"], rank, call, b) for b in range(Bn)]
        src, cnt = boxes.detach().cpu().numpy(), [int(v) for v in torch.as_tensor(nums).reshape(-1)]
        moved = [AUG.transform_boxes(src[b], cnt[b], params[b], frame_geometry.config) for b in range(Bn)]
        new_boxes = torch.from_numpy(np.stack([m[0] for m in moved], 0)).to(boxes.dtype)
        new_nums = torch.tensor([m[1] for m in moved], dtype=torch.as_tensor(nums).dtype)
        return params, new_boxes, new_nums

    # ------------------------------------------------------------------ guarded step: device-side read-outs (no synchronisation)
    def loss_scale(self):
        """The scale the next backward is seeded with (device tensor, a copy); None without loss_scale / grad_clip_norm."""
        return None if self.optimizer.amp is None else self.optimizer.amp.scale_next.clone()

    def grad_norm(self):
        """Global L2 norm of the last step's averaged, unscaled gradient (device tensor, a copy; before clipping)."""
        return None if self.optimizer.amp is None else self.optimizer.amp.grad_norm.clone()

    def loss_terms(self):
        """loss_sampling: focal -- [B,3] fp32 = (classification term, regression term without the gain, positive cells) per sample of
        the last step, unweighted; zero rows for the samples `loss_reduction: last` leaves out (device tensor, a copy).
        loss_sampling: anchor -- the same, the third column counting positive anchors.  None in the other modes."""
        terms = self.loss_total.last_terms
        return None if terms is None else terms.clone()

    def loss_iou(self):
        """iou_loss_gain > 0 -- [B,2] fp32 = (mean rotated IoU of the positive anchors' decoded boxes with their labels, positive anchors)
        per sample of the last step; zero rows for the samples `loss_reduction: last` leaves out (device tensor, a copy, no
        synchronisation).  None when the term is off or nothing has been computed yet."""
        iou = self.loss_total.last_iou
        return None if iou is None else iou.clone()

    def skipped_steps(self):
        """Steps skipped for a non-finite gradient so far (device int64 tensor, a copy)."""
        return None if self.optimizer.amp is None else self.optimizer.amp.skipped_steps.clone()

    # ------------------------------------------------------------------ training recipe: read-outs (no synchronisation)
    def learning_rate(self):
        """The rate the NEXT optimiser call runs at (host float: the schedule is a function of the host's call count)."""
        return float(self.optimizer.lr_at(self.optimizer.opt_calls))

    def learning_rates(self):
        """The rates the NEXT optimiser call runs at, per parameter-group id (host floats, no device read): entry 0 is the base
        group's, entry i the i-th listed group's (0.0 when frozen); one entry without param_groups."""
        return self.optimizer.group_rates(self.optimizer.opt_calls)

    def ema_params(self):
        """The averaged weights: a device arena laid out like model.flat_params (the tensor itself); None without ema_decay."""
        if self.optimizer.ema is None:
            return None
        if self._ema_swapped:
            raise RuntimeError("ema_params() inside ema_weights(): the arenas are exchanged")
        self.optimizer.seed_ema()
        return self.optimizer.ema

    def ema_state_dict(self):
        """The model's state_dict (the reference's key names) with the averaged weights for the parameters; buffers (BatchNorm
        statistics) are the model's own.  None without ema_decay."""
        ema = self.ema_params()
        if ema is None:
            return None
        from .engine import ParamTable
        sd = {k: v.detach() for k, v in self.model.state_dict().items()}
        for key, shape, off, n, layout in self.model._table.entries:
            sd[key] = ParamTable.view(ema, shape, off, n, layout)
        return sd

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body on the averaged weights: the CONTENTS of the parameter arena and of the EMA arena are exchanged in place and
        exchanged back on exit (also on an exception).  No address changes, so captured graphs and the backend's tables stay valid;
        the backend re-folds the weight images on the next forward by itself.  Does not nest; one_step inside raises."""
        if self.optimizer.ema is None:
            raise RuntimeError("ema_weights(): ema_decay is not configured")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() does not nest")
        self.optimizer.seed_ema()
        p, e = self.model.flat_params.detach(), self.optimizer.ema

        def exchange():
            tmp = p.clone()
            p.copy_(e)
            e.copy_(tmp)

        exchange()
        self._ema_swapped = True
        try:
            yield self
        finally:
            exchange()
            self._ema_swapped = False

    # ------------------------------------------------------------------ checkpoint / resume
    def save_checkpoint(self, path, epoch=0):
        """Model state_dict (the reference's key names, train.py:79) plus what the reference never saved:
        optimiser moments / step count and the epoch, so that training can really resume."""
        sd = {k: v.detach().clone().contiguous().cpu() for k, v in self.model.state_dict().items()}
        if self._ema_swapped:
            raise RuntimeError("save_checkpoint inside ema_weights(): the arenas are exchanged")
        opt = {"step": self.optimizer.step_count, "m": self.optimizer.m.cpu(), "v": self.optimizer.v.cpu(),
               "opt_calls": int(self.optimizer.opt_calls)}
        if self.optimizer.ema is not None:         # the weight average (the schedule's clock is opt_calls above)
            self.optimizer.seed_ema()
            opt["ema"] = self.optimizer.ema.cpu()
        if self.optimizer.amp is not None:         # the guard state (scale, growth tracker, counters), without the partials workspace
            opt["amp"] = self.optimizer.amp.header.cpu()
        ck = {"model": sd, "optimizer": opt, "epoch": int(epoch), "loss_calls": int(getattr(self.loss_total, "calls", 0)),
              "aug_calls": int(self.aug_calls)}
        if self.accum is not None:                 # gradient accumulation: where the window stands and, inside one, its sum so far
            ck["accum_index"] = int(self._accum_index)
            if self._accum_index:
                ck["accum"] = self.accum_buf.cpu()
        torch.save(ck, path)

    def load_checkpoint(self, path):
        ck = torch.load(path, map_location="cpu")
        if "model" not in ck:                      # a bare state_dict written by the reference's train.py
            self.model.load_state_dict(ck)
            return 0
        self.model.load_state_dict(ck["model"])
        self.optimizer.load_state_dict({k: (v.to(self.model.flat_params.device) if torch.is_tensor(v) else v)
                                        for k, v in ck["optimizer"].items() if k != "amp"})
        amp = ck["optimizer"].get("amp")
        if self.optimizer.amp is not None and amp is not None:
            self.optimizer.amp.header.copy_(amp)    # a checkpoint without it keeps the configured initial scale
        if hasattr(self.loss_total, "calls"):       # device sampling: a resumed run continues the draw sequence instead of replaying it
            self.loss_total.calls = int(ck.get("loss_calls", self.optimizer.step_count))
        self.aug_calls = int(ck.get("aug_calls", self.optimizer.step_count))    # augmentation: the draw sequence continues likewise
        # gradient accumulation: a checkpoint without the keys (or written at a boundary) loads at a window boundary; one written
        # inside a window needs a trainer that can hold it
        idx = int(ck.get("accum_index", 0))
        if idx and (self.accum is None or idx >= self.accum["steps"] or ck.get("accum") is None):
            raise ValueError("the checkpoint was written %d micro-steps into an accumulation window: load it with grad_accum_steps > %d"
                             % (idx, idx))
        if idx:
            self.accum_buf.copy_(ck["accum"])
        self._accum_index = idx
        return int(ck.get("epoch", 0))

    def get_loss_value(self, lidar_voxel, camera_image, object_data, num_ref_box, **extra):
        with torch.no_grad():
            pred_cls, pred_reg, _ = self._predict(lidar_voxel, camera_image, extra)
            self.loss_value = self.loss_total(object_data, num_ref_box, pred_cls, pred_reg)
        return self.loss_value.item(), pred_cls, pred_reg


_HOST_PG = None        # gloo side group of init_distributed(): host-side fences that never touch RCCL


def _eval_barrier(timeout_s=None):
    """All ranks meet before and after rank 0's evaluation (train.main): no rank enters a gradient all-reduce while rank 0 is
    still evaluating.  The device is drained first; the fence itself is a HOST barrier on the gloo side group
    (dist.monitored_barrier: TCP store round trips, its own timeout, names the rank that did not arrive) -- with the product's
    `nccl` backend a plain dist.barrier() is itself an RCCL all-reduce, i.e. the waiting ranks would sit in a pending collective
    under the RCCL watchdog for as long as rank 0 evaluates.  Timeout: DCF_EVAL_BARRIER_TIMEOUT_S (default
    3600 s, an evaluation pass over the whole test set)."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if _HOST_PG is not None:
        import datetime
        t = float(timeout_s if timeout_s is not None else os.environ.get("DCF_EVAL_BARRIER_TIMEOUT_S", "3600"))
        dist.monitored_barrier(group=_HOST_PG, timeout=datetime.timedelta(seconds=t))
    else:
        dist.barrier()          # the default group is gloo already (functional runs) or no side group could be made


def init_distributed():
    """env:// rendezvous, one rank per GPU (RANK/LOCAL_RANK/WORLD_SIZE from torchrun)."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    # (DCF_FORCE_DIST=1: a process group even for one rank -- the RCCL path on a one-GPU test box)
    if (ws > 1 or os.environ.get("DCF_FORCE_DIST") == "1") and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # "nccl" is RCCL on ROCm (xGMI). DCF_DIST_BACKEND=gloo lets two ranks share one GPU for functional tests.
        backend = os.environ.get("DCF_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
    global _HOST_PG
    if dist.is_available() and dist.is_initialized() and _HOST_PG is None and dist.get_world_size() > 1:
        # host-side fences (evaluation barriers) go through a gloo group of their own: created once, by every rank, here
        _HOST_PG = dist.new_group(backend="gloo") if dist.get_backend() != "gloo" else dist.group.WORLD
    return ws


def make_dataset(config, mode="train"):
    """train.py:58-65: CarlaDataset or KittiDataset by config["dataset_name"], in raw mode for the FrameLoader;
    synthetic frames when the data directory does not exist."""
    from .data_import_carla import CarlaDataset, SyntheticDataset
    from .data_import_kitti import KittiDataset
    if config.get("dataset_name") == "kitti":
        ds = KittiDataset(config, mode=mode, raw=True)
        if len(ds):
            return ds
    elif os.path.isdir(config["train_data_dir" if mode == "train" else "test_data_dir"]):
        ds = CarlaDataset(config, mode=mode, raw=True)
        if len(ds):
            return ds
    print("no %s frames under the configured data directory: synthetic frames" % mode)
    return SyntheticDataset(config, length=64, raw=True)


def evaluate(training, tester, dataset, loader, max_batches=None):
    """The reference's evaluation pass (train.py:87-100 every 500 batches, :105-122 at the end of an epoch): loss, the
    score-threshold / NMS / precision-recall counters of test.Test over the test loader.  Returns (mean loss, cumulative
    loss, number of positives, number of labelled boxes, TP counters per IoU threshold)."""
    tester.initialize_ap()
    cum = 0.0
    n = 0
    # ema_decay with ema_eval (default true): the pass runs on the averaged weights
    averaged = getattr(training, "recipe", None) is not None and training.recipe["ema_decay"] is not None and training.recipe["ema_eval"]
    with (training.ema_weights() if averaged else contextlib.nullcontext()):
        for n, batch in enumerate(loader, 1):
            batch.wait()
            x_lidar, geom = training.geometry_async(dataset.geometry, batch["points"], crts=batch.get("crt"), wait_event=batch.event)
            extra = {}
            if getattr(tester, "_kitti", None) is not None and tester._kitti() is not None:      # eval_protocol: kitti
                extra = dict(levels=batch.get("bbox_level"), dontcare=batch.get("dontcare"),    # crt: what geometry_async projected this batch with
                             crt=own_crts(dataset.geometry.crt, batch.get("crt"), len(batch["points"])))
            value, _ = tester.get_eval_value_onestep(x_lidar, batch["image"], batch["bboxes"], batch["num_bboxes"], geom=geom, **extra)
            cum += value
            if max_batches is not None and n >= max_batches:
                break
    if hasattr(tester, "summary"):                                         # eval_metric: ranked (test.RankedTest): the one synchronisation
        tester.summary()
    else:
        tester.display_average_precision()
    return cum / max(n, 1), cum, tester.get_num_P(), tester.get_num_T(), tester.get_num_TP_set()


def make_tester(model, config):
    """test.Test (`eval_metric` absent or compat: the reference's post-processing) or test.RankedTest (`eval_metric: ranked`)."""
    from .test import RankedTest, Test
    from . import evalkitti
    metric = config.get("eval_metric") or "compat"
    if metric not in ("compat", "ranked"):
        raise ValueError("eval_metric must be compat or ranked (got %r)" % (metric,))
    evalkitti.protocol(config)                                             # eval_protocol: kitti needs eval_metric: ranked
    return (RankedTest if metric == "ranked" else Test)(model, config)


def _print_ranked(tester):
    if hasattr(tester, "summary"):
        s = tester.summary()
        if s.get("protocol") == "kitti":
            from . import evalkitti
            print("    " + evalkitti.report_line(s, tester._kitti()["report_iou"]))
            return
        print("    AP (R40) %s, mAP %.4f" % ({t: round(v, 4) for t, v in s["ap"].items()}, s["map"]))


def main():
    import yaml
    from .frame_loader import FrameLoader
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "config", "config_carla.yaml")) as f:
        config = yaml.safe_load(f)
    init_distributed()
    rank0 = not dist.is_initialized() or dist.get_rank() == 0
    dataset = make_dataset(config)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, shuffle=True) if world() > 1 else None
    loader = FrameLoader(dataset, config["batch_size"], sampler=sampler, shuffle=True, num_workers=int(config.get("num_workers", 4)),
                         drop_last=True)
    training = Train(config)
    # the reference builds Test(training.model) before the loop (train.py:76), which is what puts the trained module in eval
    # mode: bn_mode "eval" is the default here, and with bn_mode "module" this constructor has the same effect
    tester = make_tester(training.model, config)
    test_dataset = make_dataset(config, "test") if rank0 else None
    test_loader = FrameLoader(test_dataset, config["batch_size"], shuffle=False, num_workers=int(config.get("num_workers", 4)),
                              drop_last=True) if rank0 else None
    os.makedirs("./saved_model", exist_ok=True)
    if rank0 and training.accum is not None:
        k = training.accum["steps"]
        print("gradient accumulation: %d micro-steps per optimiser step (%s), effective batch %d = %d frames x %d ranks x %d"
              % (k, training.accum["reduce"], config["batch_size"] * world() * k, config["batch_size"], world(), k))
    for epoch in range(config["num_epoch"]):
        if sampler is not None:
            sampler.set_epoch(epoch)
        if rank0:
            torch.save(training.model.state_dict(), "./saved_model/" + config["saved_model_name"])
            if training.ema_params() is not None:                          # the averaged weights beside the model, same key names
                torch.save(training.ema_state_dict(), "./saved_model/" + config["saved_model_name"] + "_ema")
            if training.param_groups is None:
                print("epoch %d: learning rate %.6g" % (epoch, training.learning_rate()))
            else:
                print("epoch %d: learning rate %.6g, per parameter group %s" % (epoch, training.learning_rate(), " ".join("%.6g" % r for r in training.learning_rates())))
        terms_sum, terms_n = None, 0                                       # focal: the epoch's mean terms, added up on the device
        iou_sum = None                                                     # iou_loss_gain: (sum of mean IoU x positives, positives), on the device
        pasted, pasted_frames = 0, 0                                       # augment_paste: accepted objects / frames of the epoch
        occluders, covering = 0, 0                                         # camera_mask.paste_occlusion: occluding patches / dropped objects
        for batch_ndx, batch in enumerate(loader):
            training.one_step_raw(dataset.geometry, batch)
            if training.paste is not None:
                pasted += sum(len(rows) for rows in training.last_paste)
                pasted_frames += len(training.last_paste)
                occluders += sum(m for m, _ in training.last_masked)
                covering += sum(d for _, d in training.last_masked)
            terms = training.loss_terms()
            if terms is not None:                                          # (the batch mean is over the samples the reduction counts)
                counted = terms[-1:] if training.loss_total.reduction == "last" else terms
                terms_sum = counted.mean(0) if terms_sum is None else terms_sum + counted.mean(0)
                terms_n += 1
            iou = training.loss_iou()
            if iou is not None:                                            # weighted by the positives: the epoch mean is over anchors
                step = torch.stack(((iou[:, 0] * iou[:, 1]).sum(), iou[:, 1].sum()))
                iou_sum = step if iou_sum is None else iou_sum + step
            if batch_ndx % 100 == 0:
                print("training at ", batch_ndx, "is processed, loss %.4f" % training.loss_value.item())
            if batch_ndx % 500 == 0 and batch_ndx != 0:                    # train.py:87-100
                # Rank 0 evaluates, the others WAIT HERE: without the barriers they would walk into the next step's gradient
                # all-reduce and sit in it for as long as the evaluation takes (minutes: an RCCL watchdog hazard).  A barrier on
                # the host (monitored_barrier on the gloo side group of init_distributed) has no such timeout coupling to a pending collective.
                _eval_barrier()
                if rank0:
                    mean, cum, npos, nt, tp = evaluate(training, tester, test_dataset, test_loader, max_batches=int(config.get("eval_batches", 7)))           # `batch_ndx_ > 5`
                    print("batch %d: validation loss %.4f, positives %d, labelled %d, TP@0.5 %d" % (batch_ndx, mean, npos, nt, tp[0.5]))
                    _print_ranked(tester)
                _eval_barrier()
        training.finish_window()                                           # a short last window steps with what it has: the
        #                                                                    evaluation below and the next save see no open window
        if rank0 and pasted_frames:
            print("epoch %d: %.2f pasted objects per frame (%d frames)" % (epoch, pasted / pasted_frames, pasted_frames))
            if training.camera_mask is not None and training.camera_mask["paste_occlusion"]:
                print("epoch %d: camera mask: %.2f occluding patches and %.2f objects dropped over nearer labels per frame"
                      % (epoch, occluders / pasted_frames, covering / pasted_frames))
        if rank0 and terms_n:
            cls_mean, reg_mean, npos_mean = (terms_sum / terms_n).tolist()
            what = "positive anchors" if training.loss_total.sampling == "anchor" else "positive cells"
            print("epoch %d: focal classification %.4f, regression %.4f, %s %.1f (batch means)" % (epoch, cls_mean, reg_mean, what, npos_mean))
        if rank0 and iou_sum is not None:
            total, n = iou_sum.tolist()
            print("epoch %d: mean %s IoU of the positive anchors %.4f (%d anchors)" % (epoch, training.loss_total.iou_kind, total / max(n, 1.0), int(n)))
        _eval_barrier()
        if rank0:                                                          # train.py:105-122
            mean, cum, npos, nt, tp = evaluate(training, tester, test_dataset, test_loader, max_batches=int(config.get("eval_batches_epoch", 12)))   # `batch_ndx > 10`
            print("epoch %d: validation loss %.4f (cumulative %.2f), positives %d, labelled %d, TP %s" % (epoch, mean, cum, npos, nt, dict(tp)))
            _print_ranked(tester)
        _eval_barrier()


if __name__ == "__main__":
    main()

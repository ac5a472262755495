"""Host: every config parser of the train-time pipeline against one table -- per row either the exact return value (types included:
tuples stay tuples, floats stay floats) or a ValueError whose text names the key.  The rows hold the cases on which the parsers'
value checks differ on purpose: numeric strings (the guard keys take them, nothing else does), negatives (the recipe's number check
rejects them, the augmentation blocks leave them to their range rules), bools, nan and inf for every key family."""
import re

import numpy as np
import pytest

from _util import pkg

NAN, INF = float("nan"), float("inf")


class Raises(object):
    """The row raises ValueError and the message holds every one of `needles`."""

    def __init__(self, *needles):
        self.needles = needles

    def __repr__(self):
        return "Raises%r" % (self.needles,)


def same(got, want):
    """Equal values of equal types, through dicts, lists, tuples and arrays."""
    if type(got) is not type(want):
        return False
    if isinstance(want, dict):
        return set(got) == set(want) and all(same(got[k], want[k]) for k in want)
    if isinstance(want, (list, tuple)):
        return len(got) == len(want) and all(same(a, b) for a, b in zip(got, want))
    if isinstance(want, np.ndarray):
        return got.dtype == want.dtype and np.array_equal(got, want)
    return got == want


def _train(name):
    return lambda *a: getattr(pkg("train"), name)(*a)


def _mod(module, name):
    return lambda *a: getattr(pkg(module), name)(*a)


guard, accum, window = _train("parse_guard_config"), _train("parse_accum_config"), _train("window_factor")
bev, image, paste_cfg, mask = (_train("parse_augment_config"), _train("parse_image_augment_config"), _train("parse_paste_config"),
                               _train("parse_camera_mask_config"))
schedule, recipe, groups = _mod("optim", "parse_schedule"), _mod("optim", "parse_optim_config"), _mod("optim", "parse_param_groups")
mask_alone, paste_check, norm = _mod("visibility", "parse_config"), _mod("paste", "check_config"), _mod("finetune", "parse_image_norm")

GUARD_DEFAULT = {"mode": None, "scale": 1.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "max_norm": None}
BEV_DEFAULT = {"seed": 0, "rotation_deg": 0.0, "scale": (1.0, 1.0), "flip_prob": 0.0, "point_drop": (0.0, 0.0)}
IMAGE_DEFAULT = {"seed": 0, "zoom": (1.0, 1.0), "shift": (0.0, 0.0), "flip_prob": 0.0, "brightness": (1.0, 1.0), "contrast": (1.0, 1.0),
                 "channel_gain": (1.0, 1.0), "drop_prob": 0.0}
PASTE_DEFAULT = {"seed": 0, "bank": "bank.npz", "target_objects": 15, "max_candidates": 16, "margin": 0.0, "paste_image": True}
SCHEDULE_DEFAULT = {"kind": "constant", "warmup_steps": 0, "warmup_start_factor": 0.0, "milestones": (), "gamma": 0.1, "total_steps": None,
                    "min_lr": 0.0}
RECIPE_DEFAULT = {"schedule": None, "weight_decay": 0.0, "weight_decay_exclude": (), "ema_decay": None, "ema_warmup": False, "ema_eval": True}


def _bev(**blk):
    return {"augment": dict({"enabled": True}, **blk)}


def _image(**blk):
    return {"augment_image": dict({"enabled": True}, **blk)}


def _paste(**blk):
    return {"augment_paste": dict({"enabled": True, "bank": "bank.npz"}, **blk)}


def _group(**g):
    return [dict({"match": ["a."]}, **g)]


ROWS = [
    # ------------------------------------------------------------------ the guarded step (flat keys; numeric strings are taken)
    (guard, ({},), None),
    (guard, ({"loss_scale": "none"},), None),
    (guard, ({"loss_scale": None},), None),
    (guard, ({"loss_scale": " Dynamic "},), dict(GUARD_DEFAULT, mode="dynamic", scale=65536.0)),
    (guard, ({"loss_scale": "dynamic", "loss_scale_init": "1024"},), dict(GUARD_DEFAULT, mode="dynamic", scale=1024.0)),
    (guard, ({"loss_scale": 128},), dict(GUARD_DEFAULT, mode="static", scale=128.0)),
    (guard, ({"loss_scale": "128"},), dict(GUARD_DEFAULT, mode="static", scale=128.0)),
    (guard, ({"grad_clip_norm": "1.5"},), dict(GUARD_DEFAULT, max_norm=1.5)),
    (guard, ({"grad_clip_norm": 2, "loss_scale_growth_factor": "3", "loss_scale_backoff_factor": "0.25", "loss_scale_growth_interval": 7},),
     dict(GUARD_DEFAULT, max_norm=2.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7)),
    (guard, ({"loss_scale": "big"},), Raises("loss_scale", "'big'")),
    (guard, ({"loss_scale": 0},), Raises("loss_scale")),
    (guard, ({"loss_scale": -2.0},), Raises("loss_scale")),
    (guard, ({"loss_scale": "dynamic", "loss_scale_init": 0},), Raises("loss_scale_init")),
    (guard, ({"loss_scale_growth_factor": 1.0},), Raises("loss_scale_growth_factor")),
    (guard, ({"loss_scale_backoff_factor": 1.0},), Raises("loss_scale_backoff_factor")),
    (guard, ({"loss_scale_backoff_factor": -0.5},), Raises("loss_scale_backoff_factor", "(0, 1)")),
    (guard, ({"grad_clip_norm": 0},), Raises("grad_clip_norm")),
    (guard, ({"grad_clip_norm": -1.0},), Raises("grad_clip_norm", "positive")),
    (guard, ({"loss_scale_growth_interval": True},), Raises("loss_scale_growth_interval")),
    (guard, ({"loss_scale_growth_interval": 0},), Raises("loss_scale_growth_interval")),
    (guard, ({"loss_scale_growth_interval": 5.0},), Raises("loss_scale_growth_interval")),
    (guard, ({"loss_scale_growth_interval": "5"},), Raises("loss_scale_growth_interval")),
    # ------------------------------------------------------------------ gradient accumulation
    (accum, ({},), None),
    (accum, ({"grad_accum_steps": 1},), None),
    (accum, ({"grad_accum_steps": 4},), {"steps": 4, "reduce": "mean"}),
    (accum, ({"grad_accum_steps": 2, "grad_accum_reduce": " SUM "},), {"steps": 2, "reduce": "sum"}),
    (accum, ({"grad_accum_steps": 1, "grad_accum_reduce": "median"},), Raises("grad_accum_reduce", "'median'")),
    (accum, ({"grad_accum_steps": 1, "grad_accum_reduce": None},), Raises("grad_accum_reduce")),
    (accum, ({"grad_accum_steps": True},), Raises("grad_accum_steps")),
    (accum, ({"grad_accum_steps": 0},), Raises("grad_accum_steps")),
    (accum, ({"grad_accum_steps": 2.0},), Raises("grad_accum_steps")),
    (accum, ({"grad_accum_steps": "2"},), Raises("grad_accum_steps")),
    (window, (None, 3), 1.0),
    (window, ({"steps": 4, "reduce": "sum"}, 3), 1.0),
    (window, ({"steps": 4, "reduce": "mean"}, 4), 0.25),
    (window, ({"steps": 4, "reduce": "mean"}, 0), Raises("micro-step")),
    (window, ({"steps": 4, "reduce": "mean"}, True), Raises("micro-step")),
    # ------------------------------------------------------------------ augment
    (bev, ({},), None),
    (bev, ({"augment": None},), None),
    (bev, ({"augment": [1, 2]},), Raises("augment must be a mapping")),
    (bev, (_bev(bogus=1),), Raises("augment: unknown keys", "bogus")),
    (bev, (_bev(),), BEV_DEFAULT),
    (bev, ({"augment": {}},), None),
    (bev, (_bev(seed=7, rotation_deg=20, scale=[1, 2], flip_prob=1, point_drop=(0, 0.5)),),
     {"seed": 7, "rotation_deg": 20.0, "scale": (1.0, 2.0), "flip_prob": 1.0, "point_drop": (0.0, 0.5)}),
    (bev, (_bev(enabled=False, rotation_deg=20.0, scale=[0.9, 1.1]),), None),
    (bev, (_bev(enabled=False, rotation_deg=-1.0),), Raises("augment.rotation_deg")),
    (bev, (_bev(enabled=False, scale=[1.1, 0.9]),), Raises("augment.scale", "lo > hi")),
    (bev, (_bev(enabled=1),), Raises("augment.enabled")),
    (bev, (_bev(seed=True),), Raises("augment.seed")),
    (bev, (_bev(seed=1.0),), Raises("augment.seed")),
    (bev, (_bev(rotation_deg=-0.5),), Raises("augment.rotation_deg", "r >= 0")),
    (bev, (_bev(scale=[1.1, 0.9]),), Raises("augment.scale", "lo > hi")),
    (bev, (_bev(scale=[0.0, 1.0]),), Raises("augment.scale", "positive")),
    (bev, (_bev(scale=[1.0, 1.0, 1.0]),), Raises("augment.scale")),
    (bev, (_bev(scale=1.0),), Raises("augment.scale")),
    (bev, (_bev(flip_prob=1.5),), Raises("augment.flip_prob", "probability")),
    (bev, (_bev(flip_prob=-0.5),), Raises("augment.flip_prob", "probability")),
    (bev, (_bev(point_drop=[0.1, 1.2]),), Raises("augment.point_drop", "probability")),
    (bev, (_bev(point_drop=[0.3, 0.2]),), Raises("augment.point_drop", "lo > hi")),
    # ------------------------------------------------------------------ augment_image
    (image, ({},), None),
    (image, ({"augment_image": "on"},), Raises("augment_image must be a mapping")),
    (image, (_image(bogus=1),), Raises("augment_image: unknown keys", "bogus")),
    (image, (_image(),), IMAGE_DEFAULT),
    (image, (_image(seed=3, zoom=[0.5, 2], shift=(0.5, 0), flip_prob=1, brightness=[0.8, 1.2], contrast=[1, 1], channel_gain=[0.9, 1.1], drop_prob=0.25),),
     {"seed": 3, "zoom": (0.5, 2.0), "shift": (0.5, 0.0), "flip_prob": 1.0, "brightness": (0.8, 1.2), "contrast": (1.0, 1.0),
      "channel_gain": (0.9, 1.1), "drop_prob": 0.25}),
    (image, (_image(enabled=False, zoom=[0.8, 1.25]),), None),
    (image, (_image(enabled=False, zoom=[0.4, 1.0]),), Raises("augment_image.zoom", ">= 0.5")),
    (image, (_image(zoom=[0.4, 1.0]),), Raises("augment_image.zoom", ">= 0.5")),
    (image, (_image(zoom=[1.25, 0.8]),), Raises("augment_image.zoom", "lo > hi")),
    (image, (_image(zoom=[0.8]),), Raises("augment_image.zoom", "[0.8]")),
    (image, (_image(shift=[0.6, 0.0]),), Raises("augment_image.shift", "[0, 0.5]")),
    (image, (_image(shift=[0.0, 0.51]),), Raises("augment_image.shift", "[0, 0.5]")),
    (image, (_image(shift=[-0.1, 0.0]),), Raises("augment_image.shift", "[0, 0.5]")),        # by the range rule, not by the number check
    (image, (_image(brightness=[0.0, 1.0]),), Raises("augment_image.brightness", "positive")),
    (image, (_image(contrast=[-1.0, 1.0]),), Raises("augment_image.contrast", "positive")),
    (image, (_image(channel_gain=[1.2, 0.8]),), Raises("augment_image.channel_gain", "lo > hi")),
    (image, (_image(drop_prob=-0.1),), Raises("augment_image.drop_prob", "probability")),
    (image, (_image(flip_prob=1.01),), Raises("augment_image.flip_prob", "probability")),
    (image, (_image(enabled="yes"),), Raises("augment_image.enabled")),
    (image, (_image(seed=False),), Raises("augment_image.seed")),
    # ------------------------------------------------------------------ augment_paste
    (paste_cfg, ({},), None),
    (paste_cfg, ({"augment_paste": 3},), Raises("augment_paste must be a mapping")),
    (paste_cfg, (_paste(bogus=1),), Raises("augment_paste: unknown keys", "bogus")),
    (paste_cfg, (_paste(),), PASTE_DEFAULT),
    (paste_cfg, (_paste(seed=9, target_objects=4, max_candidates=8, margin=1, paste_image=False),),
     {"seed": 9, "bank": "bank.npz", "target_objects": 4, "max_candidates": 8, "margin": 1.0, "paste_image": False}),
    (paste_cfg, ({"augment_paste": {"enabled": False, "margin": 0.1}},), None),
    (paste_cfg, ({"augment_paste": {"enabled": False, "max_candidates": 17}},), Raises("augment_paste.max_candidates", "17")),
    (paste_cfg, (_paste(max_candidates=17),), Raises("augment_paste.max_candidates", "17")),
    (paste_cfg, (_paste(max_candidates=0),), Raises("augment_paste.max_candidates")),
    (paste_cfg, (_paste(max_candidates=True),), Raises("augment_paste.max_candidates")),
    (paste_cfg, ({"augment_paste": {"enabled": True}},), Raises("augment_paste.bank")),
    (paste_cfg, ({"augment_paste": {"enabled": True, "bank": ""}},), Raises("augment_paste.bank")),
    (paste_cfg, (_paste(bank=5),), Raises("augment_paste.bank")),
    (paste_cfg, (_paste(target_objects=-1),), Raises("augment_paste.target_objects")),
    (paste_cfg, (_paste(target_objects=2.0),), Raises("augment_paste.target_objects")),
    (paste_cfg, (_paste(target_objects=True),), Raises("augment_paste.target_objects")),
    (paste_cfg, (_paste(margin=-0.5),), Raises("augment_paste.margin")),
    (paste_cfg, (_paste(paste_image=1),), Raises("augment_paste.paste_image")),
    (paste_cfg, (_paste(enabled=0),), Raises("augment_paste.enabled")),
    (paste_cfg, (_paste(seed=True),), Raises("augment_paste.seed")),
    (paste_check, ({},), None),
    (paste_check, ({"target_objects": 0, "max_candidates": 16, "margin": 0},), None),
    (paste_check, ({"max_candidates": 17},), Raises("augment_paste.max_candidates")),
    (paste_check, ({"margin": INF},), Raises("augment_paste.margin")),
    # ------------------------------------------------------------------ camera_mask
    (mask, ({},), None),
    (mask, ({"camera_mask": {}},), None),
    (mask, ({"camera_mask": {"fov_crop": False, "paste_occlusion": False}},), None),
    (mask, ({"camera_mask": {"fov_crop": True}},), {"fov_crop": True, "paste_occlusion": False}),
    (mask, ({"camera_mask": [True]},), Raises("camera_mask must be a mapping")),
    (mask, ({"camera_mask": {"bogus": True}},), Raises("camera_mask: unknown keys", "bogus")),
    (mask, ({"camera_mask": {"fov_crop": 1}},), Raises("camera_mask.fov_crop")),
    (mask, ({"camera_mask": {"paste_occlusion": "yes"}},), Raises("camera_mask.paste_occlusion")),
    (mask, ({"camera_mask": {"paste_occlusion": True}},), Raises("camera_mask.paste_occlusion", "augment_paste")),
    (mask, (dict(_paste(enabled=False), camera_mask={"paste_occlusion": True}),), Raises("camera_mask.paste_occlusion", "augment_paste")),
    (mask, (dict(_paste(paste_image=False), camera_mask={"paste_occlusion": True}),), Raises("camera_mask.paste_occlusion", "paste_image")),
    (mask, (dict(_paste(), camera_mask={"paste_occlusion": True}),), {"fov_crop": False, "paste_occlusion": True}),
    (mask, (dict(_paste(max_candidates=17), camera_mask={"paste_occlusion": True}),), Raises("augment_paste.max_candidates")),
    (mask_alone, ({"camera_mask": {"paste_occlusion": True}},), {"fov_crop": False, "paste_occlusion": True}),
    (mask_alone, ({"camera_mask": {"fov_crop": None}},), Raises("camera_mask.fov_crop")),
    # ------------------------------------------------------------------ lr_schedule (the number check rejects negatives)
    (schedule, (None,), None),
    (schedule, ({},), SCHEDULE_DEFAULT),
    (schedule, ({"kind": "step", "warmup_steps": 3, "warmup_start_factor": 1, "milestones": [5, 5, 10], "gamma": 0.5, "min_lr": 0},),
     dict(SCHEDULE_DEFAULT, kind="step", warmup_steps=3, warmup_start_factor=1.0, milestones=(5, 5, 10), gamma=0.5)),
    (schedule, ({"kind": "cosine", "total_steps": 100, "min_lr": 1e-5},), dict(SCHEDULE_DEFAULT, kind="cosine", total_steps=100, min_lr=1e-5)),
    (schedule, ([],), Raises("lr_schedule must be a mapping")),
    (schedule, ({"bogus": 1},), Raises("lr_schedule: unknown keys", "bogus")),
    (schedule, ({"kind": "linear"},), Raises("lr_schedule.kind", "'linear'")),
    (schedule, ({"kind": "step", "milestones": [10, 5]},), Raises("lr_schedule.milestones", "sorted")),
    (schedule, ({"milestones": 5},), Raises("lr_schedule.milestones")),
    (schedule, ({"milestones": [True]},), Raises("lr_schedule.milestones")),
    (schedule, ({"milestones": [-1]},), Raises("lr_schedule.milestones")),
    (schedule, ({"kind": "cosine"},), Raises("total_steps")),
    (schedule, ({"kind": "cosine", "total_steps": 5, "warmup_steps": 5},), Raises("total_steps", "warmup_steps")),
    (schedule, ({"total_steps": 2.5},), Raises("lr_schedule.total_steps")),
    (schedule, ({"warmup_steps": True},), Raises("lr_schedule.warmup_steps")),
    (schedule, ({"warmup_steps": -1},), Raises("lr_schedule.warmup_steps", "-1")),
    (schedule, ({"warmup_steps": 1.5},), Raises("lr_schedule.warmup_steps")),
    (schedule, ({"warmup_start_factor": 1.5},), Raises("lr_schedule.warmup_start_factor")),
    (schedule, ({"gamma": -0.1},), Raises("lr_schedule.gamma", "must not be negative")),
    (schedule, ({"min_lr": -1e-6},), Raises("lr_schedule.min_lr", "must not be negative")),
    # ------------------------------------------------------------------ weight_decay / ema_decay
    (recipe, ({},), None),
    (recipe, ({"weight_decay": None},), None),
    (recipe, ({"weight_decay": 0},), None),
    (recipe, ({"weight_decay": 1},), dict(RECIPE_DEFAULT, weight_decay=1.0)),
    (recipe, ({"weight_decay": 0.01, "weight_decay_exclude": ["bn", "bias"]},), dict(RECIPE_DEFAULT, weight_decay=0.01, weight_decay_exclude=("bn", "bias"))),
    (recipe, ({"ema_decay": 0, "ema_warmup": True, "ema_eval": False},), dict(RECIPE_DEFAULT, ema_decay=0.0, ema_warmup=True, ema_eval=False)),
    (recipe, ({"lr_schedule": {}},), dict(RECIPE_DEFAULT, schedule=SCHEDULE_DEFAULT)),
    (recipe, ({"weight_decay": -0.01},), Raises("weight_decay", "must not be negative")),
    (recipe, ({"ema_decay": -0.1},), Raises("ema_decay", "must not be negative")),
    (recipe, ({"ema_decay": 1.0},), Raises("ema_decay", "[0, 1)")),
    (recipe, ({"ema_warmup": 1},), Raises("ema_warmup")),
    (recipe, ({"ema_eval": "yes"},), Raises("ema_eval")),
    (recipe, ({"weight_decay_exclude": "bn"},), Raises("weight_decay_exclude")),
    (recipe, ({"weight_decay_exclude": ["bn", ""]},), Raises("weight_decay_exclude")),
    (recipe, ({"lr_schedule": {"kind": "cosine"}},), Raises("total_steps")),
    # ------------------------------------------------------------------ param_groups
    (groups, (None,), None),
    (groups, ([],), None),
    (groups, ([{"match": ["a."], "lr_mult": 0.1}, {"match": ("b.", "c."), "frozen": True}, {"match": ["d"], "lr_mult": 2, "frozen": False}],),
     [{"match": ("a.",), "lr_mult": 0.1, "frozen": False}, {"match": ("b.", "c."), "lr_mult": 1.0, "frozen": True},
      {"match": ("d",), "lr_mult": 2.0, "frozen": False}]),
    (groups, (_group(lr_mult=0.5), ["a.w", "z.w"]), [{"match": ("a.",), "lr_mult": 0.5, "frozen": False}]),
    (groups, (_group(lr_mult=0.5), ["b.w", "z.w"]), Raises("param_groups", "match no parameter")),
    (groups, ({"match": ["a."]},), Raises("param_groups must be a list")),
    (groups, ([5],), Raises("param_groups[0] must be a mapping")),
    (groups, (_group(bogus=1),), Raises("param_groups[0]: unknown keys", "bogus")),
    (groups, ([{"lr_mult": 0.1}],), Raises("param_groups[0].match")),
    (groups, ([{"match": []}],), Raises("param_groups[0].match")),
    (groups, ([{"match": [""]}],), Raises("param_groups[0].match")),
    (groups, ([{"match": "a."}],), Raises("param_groups[0].match")),
    (groups, (_group(frozen=1),), Raises("param_groups[0].frozen")),
    (groups, (_group(frozen=True, lr_mult=1.0),), Raises("param_groups[0]", "exclude each other")),
    (groups, (_group(lr_mult=-1),), Raises("param_groups[0].lr_mult", "must not be negative")),
    (groups, ([{"match": ["a."]}] * 16,), Raises("param_groups", "at most 15")),
    # ------------------------------------------------------------------ fusion.image_norm
    (norm, (None,), None),
    (norm, ({"mean": [0.485, 0.456, 0.406], "std": (1, 0.5, 0.25)},),
     (np.array([0.485, 0.456, 0.406], dtype=np.float32), np.array([1.0, 0.5, 0.25], dtype=np.float32))),
    (norm, ([0.5, 0.5, 0.5],), Raises("fusion.image_norm must be a mapping")),
    (norm, ({"mean": [0, 0, 0], "std": [1, 1, 1], "bogus": 1},), Raises("fusion.image_norm: unknown keys", "bogus")),
    (norm, ({"std": [1, 1, 1]},), Raises("fusion.image_norm.mean")),
    (norm, ({"mean": [0, 0], "std": [1, 1, 1]},), Raises("fusion.image_norm.mean")),
    (norm, ({"mean": [0, 0, 0], "std": [1, 0, 1]},), Raises("fusion.image_norm.std", "greater than 0")),
    (norm, ({"mean": [0, 0, 0], "std": [1, -1, 1]},), Raises("fusion.image_norm.std", "greater than 0")),
    (norm, ({"mean": [0, 0, 0], "std": [1, 1e-50, 1]},), Raises("fusion.image_norm.std", "greater than 0")),
    (norm, ({"mean": [1e39, 0, 0], "std": [1, 1, 1]},), Raises("fusion.image_norm.mean", "overflows")),
]

# every key family that takes a number: (parser, value -> arguments, the key's name in the message, numeric strings taken)
NUMBER_KEYS = [
    (guard, lambda v: ({"loss_scale": v},), "loss_scale", True),
    (guard, lambda v: ({"loss_scale": "dynamic", "loss_scale_init": v},), "loss_scale_init", True),
    (guard, lambda v: ({"loss_scale_growth_factor": v},), "loss_scale_growth_factor", True),
    (guard, lambda v: ({"loss_scale_backoff_factor": v},), "loss_scale_backoff_factor", True),
    (guard, lambda v: ({"grad_clip_norm": v},), "grad_clip_norm", True),
    (bev, lambda v: (_bev(rotation_deg=v),), "augment.rotation_deg", False),
    (bev, lambda v: (_bev(scale=[v, 1.0]),), "augment.scale", False),
    (bev, lambda v: (_bev(flip_prob=v),), "augment.flip_prob", False),
    (bev, lambda v: (_bev(point_drop=[0.0, v]),), "augment.point_drop", False),
    (image, lambda v: (_image(zoom=[v, 1.0]),), "augment_image.zoom", False),
    (image, lambda v: (_image(shift=[0.0, v]),), "augment_image.shift", False),
    (image, lambda v: (_image(flip_prob=v),), "augment_image.flip_prob", False),
    (image, lambda v: (_image(brightness=[v, 1.0]),), "augment_image.brightness", False),
    (image, lambda v: (_image(contrast=[1.0, v]),), "augment_image.contrast", False),
    (image, lambda v: (_image(channel_gain=[v, 1.0]),), "augment_image.channel_gain", False),
    (image, lambda v: (_image(drop_prob=v),), "augment_image.drop_prob", False),
    (paste_cfg, lambda v: (_paste(margin=v),), "augment_paste.margin", False),
    (paste_check, lambda v: ({"margin": v},), "augment_paste.margin", False),
    (schedule, lambda v: ({"warmup_start_factor": v},), "lr_schedule.warmup_start_factor", False),
    (schedule, lambda v: ({"gamma": v},), "lr_schedule.gamma", False),
    (schedule, lambda v: ({"min_lr": v},), "lr_schedule.min_lr", False),
    (recipe, lambda v: ({"weight_decay": v},), "weight_decay", False),
    (recipe, lambda v: ({"ema_decay": v},), "ema_decay", False),
    (groups, lambda v: (_group(lr_mult=v),), "param_groups[0].lr_mult", False),
    (norm, lambda v: ({"mean": [v, 0.5, 0.5], "std": [1, 1, 1]},), "fusion.image_norm.mean", False),
    (norm, lambda v: ({"mean": [0, 0, 0], "std": [1, v, 1]},), "fusion.image_norm.std", False),
]
# and an integer: a bool, a float and a string are no integer anywhere
INTEGER_KEYS = [
    (guard, lambda v: ({"loss_scale_growth_interval": v},), "loss_scale_growth_interval"),
    (accum, lambda v: ({"grad_accum_steps": v},), "grad_accum_steps"),
    (bev, lambda v: (_bev(seed=v),), "augment.seed"),
    (image, lambda v: (_image(seed=v),), "augment_image.seed"),
    (paste_cfg, lambda v: (_paste(seed=v),), "augment_paste.seed"),
    (paste_cfg, lambda v: (_paste(target_objects=v),), "augment_paste.target_objects"),
    (paste_cfg, lambda v: (_paste(max_candidates=v),), "augment_paste.max_candidates"),
    (schedule, lambda v: ({"warmup_steps": v},), "lr_schedule.warmup_steps"),
    (schedule, lambda v: ({"milestones": [v]},), "lr_schedule.milestones"),
    (schedule, lambda v: ({"total_steps": v},), "lr_schedule.total_steps"),
]
for _parser, _make, _key, _strings in NUMBER_KEYS:
    for _bad in (True, False, NAN, INF, -INF, None if _key in ("loss_scale", "grad_clip_norm", "weight_decay", "ema_decay") else [1.0]):
        if _bad is not None:
            ROWS.append((_parser, _make(_bad), Raises(_key)))
    if not _strings:
        ROWS.append((_parser, _make("0.75"), Raises(_key, "'0.75'")))
    ROWS.append((_parser, _make("0.75x"), Raises(_key)))
for _parser, _make, _key in INTEGER_KEYS:
    for _bad in (True, 2.0, "2", NAN):
        ROWS.append((_parser, _make(_bad), Raises(_key)))


def _row_id(row):
    return re.sub(r"[^A-Za-z0-9_.\[\]-]+", "_", "%r" % (row[1],))[:60]


@pytest.mark.parametrize("row", ROWS, ids=[_row_id(r) for r in ROWS])
def test_parser_row(row):
    parser, args, want = row
    if isinstance(want, Raises):
        with pytest.raises(ValueError) as e:
            parser(*args)
        assert type(e.value) is ValueError
        for needle in want.needles:
            assert needle in str(e.value), (needle, str(e.value))
    else:
        got = parser(*args)
        assert same(got, want), (got, want)


def test_numeric_strings_are_a_choice_of_the_guard_keys_alone():
    """The same string under every number key: a number for the guard's keys, a ValueError everywhere else."""
    taken = [key for parser, make, key, strings in NUMBER_KEYS if strings]
    assert taken == ["loss_scale", "loss_scale_init", "loss_scale_growth_factor", "loss_scale_backoff_factor", "grad_clip_norm"]
    assert same(guard({"loss_scale": "0.75"}), dict(GUARD_DEFAULT, mode="static", scale=0.75))
    assert same(guard({"loss_scale": "dynamic", "loss_scale_init": "0.75"}), dict(GUARD_DEFAULT, mode="dynamic", scale=0.75))
    assert same(guard({"loss_scale": 2, "loss_scale_growth_factor": "1.75"}), dict(GUARD_DEFAULT, mode="static", scale=2.0, growth_factor=1.75))
    assert same(guard({"loss_scale": 2, "loss_scale_backoff_factor": "0.75"}), dict(GUARD_DEFAULT, mode="static", scale=2.0, backoff_factor=0.75))
    assert same(guard({"grad_clip_norm": "0.75"}), dict(GUARD_DEFAULT, max_norm=0.75))


def test_the_trainer_module_keeps_the_names():
    T = pkg("train")
    assert T.AUGMENT_KEYS == ("enabled", "seed", "rotation_deg", "scale", "flip_prob", "point_drop")
    assert T.IMAGE_AUGMENT_KEYS == ("enabled", "seed", "zoom", "shift", "flip_prob", "brightness", "contrast", "channel_gain", "drop_prob")
    for name in ("parse_guard_config", "parse_accum_config", "window_factor", "parse_augment_config", "parse_image_augment_config",
                 "parse_paste_config", "parse_camera_mask_config", "draw_paste_plans", "FlatAdam", "_eval_barrier"):
        assert callable(getattr(T, name)), name
    assert hasattr(T, "_HOST_PG")

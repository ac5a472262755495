"""Host statements of the training recipe: learning-rate schedule, decoupled weight decay, weight EMA.

Plain Python / numpy, no device: the trainer (train.FlatAdam) evaluates them per optimiser call and hands the results to the
optimiser kernels by value (csrc/optim.hip, dcf_adamw_ema_step).  The clock of all three is the HOST's count of optimiser
calls k = 0, 1, 2, ... -- a step the device-side guard skips still advances it, as a torch scheduler stepped beside GradScaler
does -- so nothing here ever reads the device.

The parsers of the optimiser's other config keys live here too: the guarded step (parse_guard_config) and
gradient accumulation (parse_accum_config, window_factor, section 17).  All value checks are cfgcheck's.
"""
import math

import numpy as np

from . import cfgcheck as C

SCHEDULE_KEYS = ("kind", "warmup_steps", "warmup_start_factor", "milestones", "gamma", "total_steps", "min_lr")
SCHEDULE_KINDS = ("constant", "step", "cosine")


def parse_guard_config(cfg):
    """The guarded optimiser step's keys (config_carla.yaml), validated; None = none of them set (the plain Adam step).
      loss_scale                      none | a positive number (static scale; 1 = the non-finite skip alone) | dynamic
      loss_scale_init                 first dynamic scale (GradScaler's 65536)
      loss_scale_growth_factor / loss_scale_backoff_factor / loss_scale_growth_interval    GradScaler's 2.0 / 0.5 / 2000
      grad_clip_norm                  null | maximum global L2 norm of the averaged, unscaled gradient
    Bad values raise ValueError.  These keys -- and no others -- take numeric strings (YAML reads 1e4 as one)."""
    ls = cfg.get("loss_scale", "none")
    if ls is None or (isinstance(ls, str) and ls.strip().lower() == "none"):
        mode, scale = None, 1.0
    elif isinstance(ls, str) and ls.strip().lower() == "dynamic":
        mode, scale = "dynamic", C.number("loss_scale_init", cfg.get("loss_scale_init", 65536.0), strings=True)
        if scale <= 0:
            raise ValueError("loss_scale_init must be positive (got %r)" % (cfg.get("loss_scale_init"),))
    else:
        scale = C.number("loss_scale", ls, strings=True)
        if scale <= 0:
            raise ValueError("loss_scale must be none, dynamic or a positive number (got %r)" % (ls,))
        mode = "static"
    growth = C.number("loss_scale_growth_factor", cfg.get("loss_scale_growth_factor", 2.0), strings=True)
    backoff = C.number("loss_scale_backoff_factor", cfg.get("loss_scale_backoff_factor", 0.5), strings=True)
    if growth <= 1.0:
        raise ValueError("loss_scale_growth_factor must be > 1 (got %r)" % (growth,))
    if not 0.0 < backoff < 1.0:
        raise ValueError("loss_scale_backoff_factor must be in (0, 1) (got %r)" % (backoff,))
    gi = C.integer("loss_scale_growth_interval", cfg.get("loss_scale_growth_interval", 2000), lo=1)
    clip = cfg.get("grad_clip_norm", None)
    if clip is not None:
        clip = C.number("grad_clip_norm", clip, strings=True)
        if clip <= 0:
            raise ValueError("grad_clip_norm must be positive or null (got %r)" % (cfg.get("grad_clip_norm"),))
    if mode is None and clip is None:
        return None
    return {"mode": mode, "scale": scale, "growth_factor": growth, "backoff_factor": backoff, "growth_interval": gi,
            "max_norm": clip}


def parse_accum_config(cfg):
    """Gradient accumulation (config_carla.yaml), validated: None = off (grad_accum_steps absent or 1: today's
    step), else {"steps": k, "reduce": "mean" | "sum"}.
      grad_accum_steps     k >= 1: one optimiser step per k one_step calls (micro-steps)
      grad_accum_reduce    mean (default): the optimiser sees (g_1 + ... + g_j) / j over the window's j micro-steps; sum: the plain sum
    Bad values raise ValueError, whether accumulation is on or not."""
    k = C.integer("grad_accum_steps", cfg.get("grad_accum_steps", 1), lo=1)
    red = cfg.get("grad_accum_reduce", "mean")
    if not isinstance(red, str) or red.strip().lower() not in ("mean", "sum"):
        raise ValueError("grad_accum_reduce must be mean or sum (got %r)" % (red,))
    if k == 1:
        return None
    return {"steps": k, "reduce": red.strip().lower()}


def window_factor(accum, j):
    """What a window of j micro-steps multiplies into the optimiser's gradient scale: 1 / j under `mean`, 1 under `sum` (and with
    accumulation off, accum None)."""
    if accum is None or accum["reduce"] == "sum":
        return 1.0
    if isinstance(j, bool) or not isinstance(j, int) or j < 1:
        raise ValueError("a window holds at least one micro-step (got %r)" % (j,))
    return 1.0 / j


def parse_schedule(blk):
    """The `lr_schedule` block, validated: None (absent) or {"kind", "warmup_steps", "warmup_start_factor", "milestones", "gamma",
    "total_steps", "min_lr"}.  The recipe's numbers must not be negative."""
    if blk is None:
        return None
    C.block("lr_schedule", blk, SCHEDULE_KEYS)
    kind = blk.get("kind", "constant")
    if kind not in SCHEDULE_KINDS:
        raise ValueError("lr_schedule.kind must be one of %s (got %r)" % (list(SCHEDULE_KINDS), kind))
    warm = C.integer("lr_schedule.warmup_steps", blk.get("warmup_steps", 0), lo=0)
    f0 = C.number("lr_schedule.warmup_start_factor", blk.get("warmup_start_factor", 0.0), nonneg=True)
    if f0 > 1.0:
        raise ValueError("lr_schedule.warmup_start_factor must be in [0, 1] (got %r)" % (f0,))
    ms = blk.get("milestones", [])
    if not isinstance(ms, (list, tuple)):
        raise ValueError("lr_schedule.milestones must be a list (got %r)" % (ms,))
    ms = [C.integer("lr_schedule.milestones", m, lo=0) for m in ms]
    if any(b < a for a, b in zip(ms, ms[1:])):
        raise ValueError("lr_schedule.milestones must be sorted (got %r)" % (ms,))
    gamma = C.number("lr_schedule.gamma", blk.get("gamma", 0.1), nonneg=True)
    min_lr = C.number("lr_schedule.min_lr", blk.get("min_lr", 0.0), nonneg=True)
    total = blk.get("total_steps", None)
    if total is not None:
        total = C.integer("lr_schedule.total_steps", total, lo=0)
    if kind == "cosine":
        if total is None:
            raise ValueError("lr_schedule: kind cosine needs total_steps")
        if total <= warm:
            raise ValueError("lr_schedule: total_steps (%d) must exceed warmup_steps (%d)" % (total, warm))
    return {"kind": kind, "warmup_steps": warm, "warmup_start_factor": f0, "milestones": tuple(ms), "gamma": gamma,
            "total_steps": total, "min_lr": min_lr}


def parse_optim_config(config):
    """The recipe's keys (config_carla.yaml), validated when the trainer is built.  None = none of them configured (the optimiser
    then makes exactly the launches it made before the recipe existed); else
      {"schedule": parse_schedule's block or None, "weight_decay", "weight_decay_exclude": tuple of substrings,
       "ema_decay": None or d in [0, 1), "ema_warmup", "ema_eval"}.
    Bad values raise ValueError whether or not the feature they belong to is enabled."""
    sched = parse_schedule(config.get("lr_schedule", None))
    wd = config.get("weight_decay", 0.0)
    wd = 0.0 if wd is None else C.number("weight_decay", wd, nonneg=True)
    ex = config.get("weight_decay_exclude", None)
    if ex is None:
        ex = []
    if not isinstance(ex, (list, tuple)) or any(not isinstance(s, str) or not s for s in ex):
        raise ValueError("weight_decay_exclude must be a list of non-empty strings (got %r)" % (ex,))
    d = config.get("ema_decay", None)
    if d is not None:
        d = C.number("ema_decay", d, nonneg=True)
        if d >= 1.0:
            raise ValueError("ema_decay must be in [0, 1) (got %r)" % (d,))
    warm = C.flag("ema_warmup", config.get("ema_warmup", False))
    ev = C.flag("ema_eval", config.get("ema_eval", True))
    if sched is None and wd == 0.0 and d is None:
        return None
    return {"schedule": sched, "weight_decay": wd, "weight_decay_exclude": tuple(ex), "ema_decay": d, "ema_warmup": warm,
            "ema_eval": ev}


def lr_at(sched, base_lr, k):
    """Learning rate of optimiser call k (0-based), float64, a pure function of k.  sched None = the base rate."""
    base = float(base_lr)
    if sched is None:
        return base
    k = int(k)
    warm = sched["warmup_steps"]
    if k < warm:
        f0 = sched["warmup_start_factor"]
        return base * (f0 + (1.0 - f0) * k / warm)
    j = k - warm
    kind = sched["kind"]
    if kind == "step":
        return base * sched["gamma"] ** sum(1 for m in sched["milestones"] if m <= j)
    if kind == "cosine":
        T = sched["total_steps"] - warm
        lo = sched["min_lr"]
        return lo + (base - lo) * (1.0 + math.cos(math.pi * min(j, T) / T)) / 2.0
    return base


def ema_decay_at(cfg, k):
    """Decay d_k of the weight average at optimiser call k: e' = d_k * e + (1 - d_k) * p'.  ema_warmup: min(d, (1 + k) / (10 + k)),
    so that the first calls do not average in the initial weights with the full horizon."""
    d = float(cfg["ema_decay"])
    if cfg.get("ema_warmup", False):
        d = min(d, (1.0 + k) / (10.0 + k))
    return d


def decays(key, shape, exclude=()):
    """Decoupled weight decay applies to convolution and linear weights: tensors of two or more logical dimensions whose key
    holds none of the `weight_decay_exclude` substrings.  Biases and BatchNorm affine parameters (1-D) never decay."""
    return len(shape) >= 2 and not any(s in key for s in exclude)


def decay_bits(table_entries, n_params, exclude=()):
    """The decay mask of dcf_adamw_ema_step from engine.ParamTable.entries [(key, logical shape, offset, physical numel, layout)]:
    uint64 words, one bit per float4 group (group j = arena elements 4j .. 4j+3 = bit j % 64 of word j / 64).  A decaying tensor
    sets the bits of its whole PHYSICAL extent (`ohwi` and `stem` layouts included: the stem's zero padding stays zero under a
    multiply, and so do the up to three padding elements behind a tensor).  ParamTable keeps every tensor 16-byte aligned, so no
    group holds elements of two tensors."""
    groups = (int(n_params) + 3) // 4
    bits = np.zeros(groups, dtype=bool)
    for key, shape, off, n, layout in table_entries:
        if off % 4:
            raise ValueError("parameter %s starts at element %d: not 16-byte aligned" % (key, off))
        if off + n > n_params:
            raise ValueError("parameter %s ends behind the arena (%d + %d > %d)" % (key, off, n, n_params))
        if decays(key, shape, exclude):
            bits[off // 4:(off + n + 3) // 4] = True
    padded = np.zeros((groups + 63) // 64 * 64, dtype=np.uint8)
    padded[:groups] = bits
    by = np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little")        # byte b of a word = its bits 8b .. 8b+7
    return np.ascontiguousarray(by).view("<u8").astype(np.uint64).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- parameter groups
# `param_groups`: a list of {match, lr_mult | frozen}; the first group whose `match` holds a substring of a
# parameter's state-dict key wins, listed group i has id i + 1, and an unmatched parameter is group 0 (lr_mult 1, not frozen).
GROUP_KEYS = ("match", "lr_mult", "frozen")
MAX_GROUPS = 16                         # DCF_ADAM_MAX_GROUPS: group 0 + at most 15 listed groups
TRUNK = "image_backbone."


def parse_param_groups(blk, keys=None):
    """The `param_groups` list, validated: None (absent or empty) or [{"match": tuple of substrings, "lr_mult": float >= 0,
    "frozen": bool}].  keys (the model's parameter keys): a group that wins no parameter raises too."""
    if blk is None:
        return None
    if not isinstance(blk, (list, tuple)):
        raise ValueError("param_groups must be a list of groups (got %r)" % (blk,))
    if len(blk) == 0:
        return None
    if len(blk) > MAX_GROUPS - 1:
        raise ValueError("param_groups: at most %d groups (got %d)" % (MAX_GROUPS - 1, len(blk)))
    out = []
    for i, g in enumerate(blk):
        name = "param_groups[%d]" % i
        C.block(name, g, GROUP_KEYS)
        match = g.get("match", None)
        if not isinstance(match, (list, tuple)) or len(match) == 0 or any(not isinstance(s, str) or not s for s in match):
            raise ValueError("%s.match must be a non-empty list of non-empty strings (got %r)" % (name, match))
        frozen = C.flag(name + ".frozen", g.get("frozen", False))
        if frozen and "lr_mult" in g:
            raise ValueError("%s: frozen and lr_mult exclude each other" % name)
        mult = C.number(name + ".lr_mult", g.get("lr_mult", 1.0), nonneg=True)
        out.append({"match": tuple(match), "lr_mult": mult, "frozen": frozen})
    if keys is not None:
        won = set(group_of(k, out) for k in keys)
        idle = [i for i in range(len(out)) if i + 1 not in won]
        if idle:
            raise ValueError("param_groups: groups %s match no parameter (first match wins)" % ([out[i]["match"] for i in idle],))
    return out


def group_of(key, groups):
    """Id of the parameter group of state-dict key `key`: 1 + the index of the first listed group with a matching substring, else 0."""
    for i, g in enumerate(groups or ()):
        if any(s in key for s in g["match"]):
            return i + 1
    return 0


def group_ids(table_entries, n_params, groups):
    """The id array of dcf_adamw_ema_step_groups from engine.ParamTable.entries: uint8[ceil(n / 4)], one id per float4 group of the
    arena.  Built as decay_bits is: a tensor names its whole PHYSICAL extent (layout padding and the up to three padding elements
    behind it included), and ParamTable's 16-byte alignment -- no float4 group holds elements of two tensors -- is asserted.
    Groups no tensor covers keep id 0."""
    ids = np.zeros((int(n_params) + 3) // 4, dtype=np.uint8)
    for key, shape, off, n, layout in table_entries:
        if off % 4:
            raise ValueError("parameter %s starts at element %d: not 16-byte aligned" % (key, off))
        if off + n > n_params:
            raise ValueError("parameter %s ends behind the arena (%d + %d > %d)" % (key, off, n, n_params))
        ids[off // 4:(off + n + 3) // 4] = group_of(key, groups)
    return ids


def group_table(groups, lr, weight_decay=0.0):
    """[(mu, decay_mul, frozen)] per group id 0 .. len(groups) for an optimiser call at rate lr (float64): decay_mul_g =
    fl32(1 - lr * mu_g * weight_decay), formed in float64 and rounded once, as the single decay_mul of dcf_adamw_ema_step is."""
    rows = [(1.0, False)] + [(0.0 if g["frozen"] else g["lr_mult"], g["frozen"]) for g in (groups or ())]
    return [(float(mu), float(np.float32(1.0 - float(lr) * float(mu) * float(weight_decay))), bool(fz)) for mu, fz in rows]


def group_rates(groups, lr):
    """Rates of the next call per group id (host floats): lr * mu_g, 0.0 for a frozen group."""
    return [float(lr) * mu for mu, _, _ in group_table(groups, lr)]


def frozen_trunk_units(keys, groups):
    """Length of the frozen PREFIX of the camera trunk: 0 = none, 1 = the stem (image_backbone.conv1 + .bn1), 2 = stem + layer1, ...,
    5 = stem + all four stages.  A unit counts when it has parameters and every one of them lies in a frozen group; the prefix ends
    at the first unit that does not (a frozen layer1 behind a live stem gives 0: its input gradient is still needed)."""
    if not groups:
        return 0
    units = [[] for _ in range(5)]
    for k in keys:
        if not k.startswith(TRUNK):
            continue
        rest = k[len(TRUNK):]
        if rest.startswith("conv1.") or rest.startswith("bn1."):
            units[0].append(k)
        else:
            for li in range(1, 5):
                if rest.startswith("layer%d." % li):
                    units[li].append(k)
    n = 0
    for li, ks in enumerate(units):
        gid = [group_of(k, groups) for k in ks]
        stem_whole = li != 0 or (any(TRUNK + "conv1." in k for k in ks) and any(TRUNK + "bn1." in k for k in ks))
        if not ks or not stem_whole or any(g == 0 or not groups[g - 1]["frozen"] for g in gid):
            break
        n = li + 1
    return n

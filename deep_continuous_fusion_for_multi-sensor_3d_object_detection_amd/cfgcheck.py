"""The value checks of every config parser (optim, augment, augment_image, paste, visibility, finetune): one definition each.

Plain functions, nothing imported from the package.  `name` is the dotted key as the message shows it; every failure is a ValueError
that carries the name and the offending value.  Where the parsers differ on purpose the difference is an argument at the call
site: the guarded step's keys take numeric strings (`strings=True`), the recipe's keys and the paste margin reject negatives in the
number check (`nonneg=True`), the augmentation blocks leave the sign to their own range rules.
"""
import math


def block(name, blk, keys):
    """A mapping with none but the known keys; returns it."""
    if not isinstance(blk, dict):
        raise ValueError("%s must be a mapping (got %r)" % (name, blk))
    unknown = sorted(set(blk) - set(keys))
    if unknown:
        raise ValueError("%s: unknown keys %s (known: %s)" % (name, unknown, list(keys)))
    return blk


def seeded_block(config, name, keys):
    """The head of an augmentation block: None when config has no such block, else (block, enabled, seed), checked."""
    blk = config.get(name, None)
    if blk is None:
        return None
    block(name, blk, keys)
    return blk, flag(name + ".enabled", blk.get("enabled", False)), integer(name + ".seed", blk.get("seed", 0))


def number(name, v, strings=False, nonneg=False):
    """A finite int or float as a float; a bool is no number.  strings: whatever float() converts counts too (a numeric string)."""
    try:
        f = float(v) if not isinstance(v, bool) and (strings or isinstance(v, (int, float))) else None
    except (TypeError, ValueError):
        f = None
    if f is None:
        raise ValueError("%s must be a number (got %r)" % (name, v))
    if not math.isfinite(f):
        raise ValueError("%s must be finite (got %r)" % (name, v))
    if nonneg and f < 0:
        raise ValueError("%s must not be negative (got %r)" % (name, v))
    return f


def integer(name, v, lo=None, hi=None):
    """An int (no bool, no float, no string) with lo <= v (<= hi) where given."""
    if isinstance(v, bool) or not isinstance(v, int) or (lo is not None and v < lo) or (hi is not None and v > hi):
        bounds = "" if lo is None else (" >= %d" % lo if hi is None else " in %d..%d" % (lo, hi))
        raise ValueError("%s must be an integer%s (got %r)" % (name, bounds, v))
    return int(v)


def flag(name, v):
    if not isinstance(v, bool):
        raise ValueError("%s must be true or false (got %r)" % (name, v))
    return v


def pair(name, v, form="a pair"):
    """A list or tuple of two numbers as a tuple of floats."""
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise ValueError("%s must be %s (got %r)" % (name, form, v))
    return number(name, v[0]), number(name, v[1])


def interval(name, v):
    """A pair with lo <= hi."""
    lo, hi = pair(name, v, "[lo, hi]")
    if lo > hi:
        raise ValueError("%s: lo > hi (got %r)" % (name, v))
    return lo, hi


def probability(name, v):
    f = number(name, v)
    if not 0.0 <= f <= 1.0:
        raise ValueError("%s must be a probability in [0, 1] (got %r)" % (name, v))
    return f

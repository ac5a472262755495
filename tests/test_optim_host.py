"""CPU suite: the training recipe's host statements (optim.py) -- the learning-rate schedule against hand
values and torch's schedulers, the EMA decay, config validation, the decay mask of a hand-built parameter table, the host-side
argument checks of dcf_adamw_ema_step and the ISA of the built kernels (kernel names, no packed fp32 VALU)."""
import ctypes
import math
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch
import yaml

from _util import PKG, ROOT, pkg

CSRC = os.path.join(ROOT, PKG, "csrc")


def _cfg(**over):
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")))
    cfg.update(over)
    return cfg


def test_defaults_configure_nothing():
    O = pkg("optim")
    assert O.parse_optim_config(_cfg()) is None                  # the shipped config documents the keys as comments only
    assert O.parse_optim_config({}) is None
    assert O.parse_optim_config(dict(weight_decay=0.0, weight_decay_exclude=[], ema_decay=None, ema_warmup=False, ema_eval=True,
                                     lr_schedule=None)) is None
    assert O.lr_at(None, 1e-4, 7) == 1e-4


def test_config_values():
    O = pkg("optim")
    r = O.parse_optim_config(_cfg(weight_decay=0.01))
    assert r == {"schedule": None, "weight_decay": 0.01, "weight_decay_exclude": (), "ema_decay": None, "ema_warmup": False,
                 "ema_eval": True}
    r = O.parse_optim_config(_cfg(ema_decay=0.999, ema_warmup=True, ema_eval=False, weight_decay_exclude=["head"]))
    assert r["ema_decay"] == 0.999 and r["ema_warmup"] is True and r["ema_eval"] is False and r["weight_decay_exclude"] == ("head",)
    r = O.parse_optim_config(_cfg(lr_schedule=dict(kind="cosine", total_steps=100, warmup_steps=10, min_lr=1e-6)))
    assert r["schedule"] == {"kind": "cosine", "warmup_steps": 10, "warmup_start_factor": 0.0, "milestones": (), "gamma": 0.1,
                             "total_steps": 100, "min_lr": 1e-6}
    assert O.parse_optim_config(_cfg(lr_schedule={}))["schedule"]["kind"] == "constant"
    assert O.parse_optim_config(_cfg(ema_decay=0))["ema_decay"] == 0.0


def test_lr_at_hand_values():
    """Values that are exact in float64: binary fractions for the base rate, the factors and the minimum."""
    O = pkg("optim")
    base = 0.5
    s = O.parse_schedule(dict(kind="constant", warmup_steps=10, warmup_start_factor=0.0))
    assert O.lr_at(s, 1.0, 3) == 0.3 * 1.0                       # warm-up step 3 of 10 from factor 0
    assert O.lr_at(s, base, 0) == 0.0 and O.lr_at(s, base, 5) == 0.25 and O.lr_at(s, base, 10) == base and O.lr_at(s, base, 999) == base
    s = O.parse_schedule(dict(kind="constant", warmup_steps=4, warmup_start_factor=0.5))
    assert [O.lr_at(s, base, k) for k in range(6)] == [0.25, 0.3125, 0.375, 0.4375, 0.5, 0.5]
    s = O.parse_schedule(dict(kind="step", warmup_steps=2, warmup_start_factor=0.5, milestones=[3, 5, 5], gamma=0.5))
    #   k: 0     1      2..4 (j 0..2)   5..6 (j 3..4)   7.. (j >= 5: two milestones at 5)
    assert [O.lr_at(s, base, k) for k in range(9)] == [0.25, 0.375, 0.5, 0.5, 0.5, 0.25, 0.25, 0.0625, 0.0625]
    s = O.parse_schedule(dict(kind="step", milestones=[0], gamma=0.25))
    assert O.lr_at(s, base, 0) == 0.125                          # a milestone at j = 0 counts from the first call on
    s = O.parse_schedule(dict(kind="cosine", warmup_steps=2, total_steps=10, min_lr=0.25))         # T = 8
    assert O.lr_at(s, base, 2) == base                           # j = 0
    assert O.lr_at(s, base, 6) == (base + 0.25) / 2              # j = T / 2: the midpoint
    assert O.lr_at(s, base, 10) == 0.25                          # j = T: the end value
    assert O.lr_at(s, base, 11) == 0.25 and O.lr_at(s, base, 10 ** 6) == 0.25       # j > T stays there
    assert all(O.lr_at(s, base, k) > O.lr_at(s, base, k + 1) for k in range(2, 10))
    assert isinstance(O.lr_at(s, np.float32(0.5), 3), float)


# Largest relative deviation from torch's schedulers over the 300 steps below, measured on the CPU (torch 2.10): 2.7e-16 for
# step (torch multiplies the running rate by gamma at a milestone, the statement evaluates base * gamma ** count) and 1.3e-15 for
# cosine (torch's recursive form carries float64 rounding from step to step).  The bounds are ten times those.
TORCH_DEVIATION = {"step": 2.7e-16, "cosine": 1.3e-15}


@pytest.mark.parametrize("kind", ["step", "cosine"])
def test_lr_at_against_torch_schedulers(kind):
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, MultiStepLR, SequentialLR
    O = pkg("optim")
    base, warm = 1e-3, 20
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base)
    if kind == "step":
        blk = dict(kind="step", warmup_steps=warm, warmup_start_factor=0.1, milestones=[50, 120, 200], gamma=0.5)
        second = MultiStepLR(opt, milestones=[50, 120, 200], gamma=0.5)
    else:
        blk = dict(kind="cosine", warmup_steps=warm, warmup_start_factor=0.1, total_steps=300, min_lr=1e-5)
        second = CosineAnnealingLR(opt, T_max=300 - warm, eta_min=1e-5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sch = SequentialLR(opt, [LinearLR(opt, start_factor=0.1, end_factor=1.0, total_iters=warm), second], milestones=[warm])
        s = O.parse_schedule(blk)
        worst = 0.0
        for k in range(300):
            want = opt.param_groups[0]["lr"]
            worst = max(worst, abs(O.lr_at(s, base, k) - want) / want)
            opt.step()
            sch.step()
    print("%s: largest relative deviation from torch %g" % (kind, worst))
    assert worst <= 10 * TORCH_DEVIATION[kind]


def test_ema_decay_at():
    O = pkg("optim")
    assert O.ema_decay_at({"ema_decay": 0.999, "ema_warmup": False}, 0) == 0.999
    assert O.ema_decay_at({"ema_decay": 0.999}, 12345) == 0.999
    w = {"ema_decay": 0.999, "ema_warmup": True}
    assert O.ema_decay_at(w, 0) == 0.1 and O.ema_decay_at(w, 8) == 0.5 and O.ema_decay_at(w, 90) == 0.91
    assert O.ema_decay_at(w, 8990) == 8991.0 / 9000.0 and O.ema_decay_at(w, 8991) == 0.999 and O.ema_decay_at(w, 10 ** 7) == 0.999
    assert O.ema_decay_at({"ema_decay": 0.05, "ema_warmup": True}, 0) == 0.05


@pytest.mark.parametrize("over", [
    dict(lr_schedule=dict(kind="cosine", total_steps=10, bogus=1)),                 # unknown key
    dict(lr_schedule=dict(kind="linear")), dict(lr_schedule="cosine"), dict(lr_schedule=[1]),
    dict(lr_schedule=dict(kind="cosine")),                                           # cosine without total_steps
    dict(lr_schedule=dict(kind="cosine", total_steps=5, warmup_steps=5)),            # nothing left to anneal over
    dict(lr_schedule=dict(kind="step", milestones=[5, 3])),                          # unsorted
    dict(lr_schedule=dict(kind="step", milestones=[-1, 3])), dict(lr_schedule=dict(kind="step", milestones=3)),
    dict(lr_schedule=dict(kind="step", milestones=[1.5])),
    dict(lr_schedule=dict(kind="step", gamma=-0.5)), dict(lr_schedule=dict(kind="step", gamma=float("nan"))),
    dict(lr_schedule=dict(warmup_steps=-1)), dict(lr_schedule=dict(warmup_steps=2.5)), dict(lr_schedule=dict(warmup_steps=True)),
    dict(lr_schedule=dict(warmup_start_factor=-0.1)), dict(lr_schedule=dict(warmup_start_factor=1.5)),
    dict(lr_schedule=dict(warmup_start_factor=float("inf"))),
    dict(lr_schedule=dict(kind="cosine", total_steps=10, min_lr=-1e-6)), dict(lr_schedule=dict(kind="cosine", total_steps=-10)),
    dict(weight_decay=-0.01), dict(weight_decay=float("inf")), dict(weight_decay=float("nan")), dict(weight_decay="0.01"),
    dict(weight_decay=True),
    dict(weight_decay_exclude="head"), dict(weight_decay_exclude=[1]), dict(weight_decay_exclude=[""]),       # also with weight_decay 0
    dict(ema_decay=1.0), dict(ema_decay=1.5), dict(ema_decay=-0.1), dict(ema_decay=float("nan")), dict(ema_decay="0.999"),
    dict(ema_warmup=1), dict(ema_warmup="yes"), dict(ema_eval=0), dict(ema_eval=None),                          # also with ema_decay null
])
def test_bad_recipe_config_raises(over):
    with pytest.raises(ValueError):
        pkg("optim").parse_optim_config(_cfg(**over))


def _hand_table():
    """plain 1-D tensor of 5 elements (padded to 8), an ohwi weight [O=3, I=2, 3, 3] (54 elements, padded to 56), a stem weight
    [2, 3, 7, 7] (stored [2, 7, 8, 4] = 448), a 1-D tensor of 4 and a plain 2-D weight [3, 3] (9, padded to 12)."""
    E = pkg("engine")
    t = E.ParamTable()
    t.add_param("bn.weight", (5,))
    t.add_param("block.conv.weight", (3, 2, 3, 3), "ohwi")
    t.add_param("stem.conv.weight", (2, 3, 7, 7), "stem")
    t.add_param("bn.bias", (4,))
    t.add_param("fc.weight", (3, 3))
    return t


def _bit_list(words, groups):
    return [(int(words[j // 64]) >> (j % 64)) & 1 for j in range(groups)]


def test_decay_bits_of_a_hand_built_table():
    O = pkg("optim")
    t = _hand_table()
    assert [e[2] for e in t.entries] == [0, 8, 64, 512, 516] and t.n_params == 528
    assert all(off % 4 == 0 for _, _, off, _, _ in t.entries)                # no float4 group spans two tensors
    w = O.decay_bits(t.entries, t.n_params)
    groups = t.n_params // 4                                                  # 132 groups -> 3 words
    assert w.dtype == np.uint64 and w.shape == (3,)
    #   groups 0-1 bn.weight (clear) | 2-15 ohwi, tail group 15 included | 16-127 stem, its zero padding included |
    #   128 bn.bias (clear) | 129-131 fc.weight, tail group 131 included
    want = [0] * 2 + [1] * 14 + [1] * 112 + [0] + [1] * 3
    assert _bit_list(w, groups) == want
    assert int(w[0]) == 0xFFFFFFFFFFFFFFFC and int(w[1]) == 0xFFFFFFFFFFFFFFFF and int(w[2]) == 0b1110
    # weight_decay_exclude clears a tensor by a substring of its key
    w = O.decay_bits(t.entries, t.n_params, exclude=("stem.",))
    assert _bit_list(w, groups) == [0] * 2 + [1] * 14 + [0] * 112 + [0] + [1] * 3
    w = O.decay_bits(t.entries, t.n_params, exclude=("conv", "fc"))
    assert not w.any()
    # exactly 64 groups: one word, no empty second one
    assert O.decay_bits([("w", (16, 16), 0, 256, "plain")], 256).tolist() == [2 ** 64 - 1]
    assert O.decay_bits([("w", (16, 16), 0, 256, "plain"), ("v", (2, 2), 256, 4, "plain")], 260).tolist() == [2 ** 64 - 1, 1]
    with pytest.raises(ValueError):
        O.decay_bits([("w", (2, 3), 2, 6, "plain")], 8)                       # a tensor that is not 16-byte aligned


def test_decay_bits_of_the_model_table_cover_exactly_the_weights():
    O, E = pkg("optim"), pkg("engine")
    cfg = _cfg()
    plan = E.Plan(cfg, with_image=True, cf=64, image_arch="resnet18")
    t = plan.table
    w = O.decay_bits(t.entries, t.n_params)
    bits = np.array(_bit_list(w, (t.n_params + 3) // 4), dtype=bool)
    assert len(w) == ((t.n_params + 3) // 4 + 63) // 64
    for key, shape, off, n, layout in t.entries:
        seg = bits[off // 4:(off + n + 3) // 4]
        assert seg.all() if len(shape) >= 2 else not seg.any(), key
    assert any(len(e[1]) == 1 for e in t.entries) and any(e[4] == "ohwi" for e in t.entries)


def test_adamw_ema_entry_validates_on_the_host():
    """Bad arguments are rejected before anything touches a device, and the error names the function."""
    H = pkg("_hip")
    L = H.lib()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15
    p, g, m, v, e, bits, st = a, a + 256, a + 512, a + 768, a + 1024, a + 1280, a + 1536
    ok = (0.001, 0.9, 0.999, 1e-8, 1, 1.0, 1.0, 0.0)                       # lr, beta1, beta2, eps, step, gscale, decay_mul, ema_omd

    def bad(*args):
        rc = L.dcf_adamw_ema_step(*args)
        assert rc == -1 and b"dcf_adamw_ema_step" in L.dcf_last_error(), (rc, L.dcf_last_error())

    bad(p, g, m, v, e, bits, -1, *ok, None, None)                                       # n < 0
    for k in range(4):                                                                  # null arrays
        arr = [p, g, m, v]
        arr[k] = None
        bad(*arr, e, bits, 16, *ok, None, None)
    bad(p, g, m, v, e, bits, 16, 0.001, 0.9, 0.999, 1e-8, 0, 1.0, 1.0, 0.0, None, None)  # step < 1 without a state
    for k in range(4):                                                                  # misaligned arrays
        arr = [p, g, m, v]
        arr[k] += 4
        bad(*arr, e, bits, 16, *ok, None, None)
    bad(p, g, m, v, e + 8, bits, 16, *ok, None, None)                                   # misaligned ema
    bad(p, g, m, v, e, bits + 4, 16, *ok, None, None)                                   # misaligned mask
    for dm in (float("nan"), float("inf")):
        bad(p, g, m, v, e, bits, 16, 0.001, 0.9, 0.999, 1e-8, 1, 1.0, dm, 0.0, None, None)
    for omd in (float("nan"), float("inf"), -0.25, 1.5):
        bad(p, g, m, v, e, bits, 16, 0.001, 0.9, 0.999, 1e-8, 1, 1.0, 1.0, omd, None, None)
    for other in (p, g, m, v):                                                          # ema aliases one of the four
        bad(p, g, m, v, other, bits, 16, *ok, None, None)
        bad(p, g, m, v, other + 32, bits, 16, *ok, None, None)                          # overlaps its tail
    # with a state, step is ignored (0 is fine) -- and n = 0 returns before any launch
    assert L.dcf_adamw_ema_step(p, g, m, v, e, bits, 0, 0.001, 0.9, 0.999, 1e-8, 0, 1.0, 1.0, 0.0, st, None) == 0
    assert L.dcf_adamw_ema_step(p, g, m, v, None, None, 0, *ok, None, None) == 0
    assert H.lib().dcf_version() == 202                    # an addition: the ABI version does not move


def _device_code(obj, tmp):
    fat, co = os.path.join(tmp, "optim.fatbin"), os.path.join(tmp, "optim.gfx950.co")
    subprocess.check_call(["/opt/rocm/llvm/bin/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call(["/opt/rocm/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout


def test_optim_object_has_its_kernels_and_no_packed_fp32(tmp_path):
    obj = os.path.join(CSRC, "optim.o")
    pkg("_hip").build()                                   # (no-op when the library is up to date)
    asm = _device_code(obj, str(tmp_path))
    for k in ("k_adamw_ema_flat", "k_adamw_ema_stride"):
        assert k in asm, k
    assert len(re.findall(r"v_pk_(mul|add|fma)_f32", asm)) == 0

"""CPU suite: the guarded optimiser step (csrc/amp.hip) -- config validation, host-side argument checks of its C entry points,
the Python restatement of GradScaler's schedule that tests/test_gpu_amp.py takes its expected values from, and the ISA of the
built kernels (no packed fp32 VALU)."""
import ctypes
import os
import random
import re
import subprocess

import pytest
import yaml

from _amp_ref import scale_schedule, torch_schedule
from _util import PKG, ROOT, pkg

CSRC = os.path.join(ROOT, PKG, "csrc")


def _cfg(**over):
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")))
    cfg.update(over)
    return cfg


def test_defaults_keep_the_plain_step():
    T = pkg("train")
    assert T.parse_guard_config(_cfg()) is None
    base = _cfg()
    for k in ("loss_scale", "loss_scale_init", "loss_scale_growth_factor", "loss_scale_backoff_factor", "loss_scale_growth_interval",
              "grad_clip_norm"):
        base.pop(k)
    assert T.parse_guard_config(base) is None                      # missing keys: today's behaviour
    assert T.parse_guard_config({"loss_scale": None}) is None


def test_guard_config_values():
    T = pkg("train")
    g = T.parse_guard_config(_cfg(loss_scale="dynamic"))
    assert g == {"mode": "dynamic", "scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                 "max_norm": None}
    g = T.parse_guard_config(_cfg(loss_scale=1024))
    assert g["mode"] == "static" and g["scale"] == 1024.0 and g["max_norm"] is None
    g = T.parse_guard_config(_cfg(grad_clip_norm=5))
    assert g["mode"] is None and g["scale"] == 1.0 and g["max_norm"] == 5.0          # clipping alone: guarded path, scale 1
    g = T.parse_guard_config(_cfg(loss_scale="dynamic", loss_scale_init=2 ** 30, loss_scale_growth_interval=2))
    assert g["scale"] == 2.0 ** 30 and g["growth_interval"] == 2


@pytest.mark.parametrize("over", [dict(loss_scale="bogus"), dict(loss_scale=-1.0), dict(loss_scale=0), dict(grad_clip_norm=0),
                                  dict(grad_clip_norm=-2.0), dict(loss_scale="dynamic", loss_scale_init=0),
                                  dict(loss_scale_growth_interval=0), dict(loss_scale_growth_factor=1.0),
                                  dict(loss_scale_backoff_factor=1.5), dict(loss_scale=float("inf")), dict(loss_scale=True)])
def test_bad_guard_config_raises(over):
    with pytest.raises(ValueError):
        pkg("train").parse_guard_config(_cfg(**over))


def test_guarded_entry_points_validate_on_the_host():
    """Bad arguments are rejected before anything touches a device, and the error names the function."""
    H = pkg("_hip")
    L = H.lib()
    st = ctypes.create_string_buffer(ctypes.sizeof(H.AmpState) + 16)
    sp = (ctypes.addressof(st) + 15) & ~15
    rc = L.dcf_grad_stats(sp, -1, sp, None)                       # n < 0
    assert rc == -1 and b"dcf_grad_stats" in L.dcf_last_error()
    rc = L.dcf_grad_stats(sp, 16, None, None)                     # null state
    assert rc == -1 and b"dcf_grad_stats" in L.dcf_last_error()
    rc = L.dcf_amp_update(None, 1.0, 1, 2.0, 0.5, 2000, 0.0, 1e-4, 0.9, 0.999, None)
    assert rc == -1 and b"dcf_amp_update" in L.dcf_last_error()
    rc = L.dcf_amp_update(sp, 1.0, 1, 2.0, 0.5, 0, 0.0, 1e-4, 0.9, 0.999, None)        # growth_interval 0
    assert rc == -1 and b"dcf_amp_update" in L.dcf_last_error()
    rc = L.dcf_adam_step_guarded(sp, sp, sp, sp, -1, 0.9, 0.999, 1e-8, sp, None)       # n < 0
    assert rc == -1 and b"dcf_adam_step_guarded" in L.dcf_last_error()
    rc = L.dcf_adam_step_guarded(sp, sp, sp, sp, 16, 0.9, 0.999, 1e-8, None, None)     # null state
    assert rc == -1 and b"dcf_adam_step_guarded" in L.dcf_last_error()


def test_state_struct_layout():
    H = pkg("_hip")
    assert ctypes.sizeof(H.AmpState) == 64 + 8 * H.AMP_PARTS
    assert H.AmpState.applied_steps.offset % 8 == 0 and H.AmpState.part_sum.offset == 64
    assert H.lib().dcf_version() == 202


@pytest.mark.parametrize("interval", [1, 2, 3, 7, 2000])
def test_schedule_restatement_equals_torch(interval):
    """The restatement the GPU tests take their expected scales from equals torch._amp_update_scale_ exactly, over random
    found_inf sequences of 200 steps (growth to float overflow included: a scale that would become inf stays)."""
    rng = random.Random(1000 + interval)
    for p_bad, init in ((0.0, 65536.0), (0.05, 65536.0), (0.3, 2.0 ** 30), (0.6, 1.0), (0.02, 2.0 ** 120)):
        found = [rng.random() < p_bad for _ in range(200)]
        for gf, bf in ((2.0, 0.5), (4.0, 0.25), (1.5, 0.75)):
            assert scale_schedule(found, init, gf, bf, interval) == torch_schedule(found, init, gf, bf, interval), (interval, p_bad, gf)


def _device_code(obj, tmp):
    fat, co = os.path.join(tmp, "amp.fatbin"), os.path.join(tmp, "amp.gfx950.co")
    subprocess.check_call(["/opt/rocm/llvm/bin/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call(["/opt/rocm/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout


def test_amp_object_has_no_packed_fp32_and_keeps_the_nonfinite_test(tmp_path):
    obj = os.path.join(CSRC, "amp.o")
    pkg("_hip").build()                                   # (no-op when the library is up to date)
    asm = _device_code(obj, str(tmp_path))
    for k in ("k_grad_stats", "k_amp_update", "k_adam_guarded"):
        assert k in asm, k
    assert len(re.findall(r"v_pk_(mul|add|fma)_f32", asm)) == 0
    # the non-finite test is an integer test of the exponent field: it must be in the code of k_grad_stats
    body = asm[asm.index("<_Z12k_grad_stats"):]
    body = body[:body.index("s_endpgm")]
    assert "0x7f800000" in body

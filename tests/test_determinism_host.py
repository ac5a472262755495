"""`deterministic: true` without a GPU: the new exports exist in the header, the ctypes table and the built library; the config key
parses as documented; the sources of the deterministic path hold no float atomics."""
import os
import re

import pytest

from _util import PKG, ROOT, pkg

EXPORTS = ["dcf_inv_sort_segments", "dcf_cam_invert_workspace_bytes", "dcf_cam_invert", "dcf_point_sample_bwd_det",
           "dcf_fusion_gather_bwd_det_workspace_bytes", "dcf_fusion_gather_bwd_det", "dcf_rowscale_bias_bwd_det_workspace_bytes",
           "dcf_rowscale_bias_bwd_det", "dcf_rows_fold", "dcf_loss_fwd_bwd_det", "dcf_loss_sample_fwd_bwd_det"]
CSRC = os.path.join(ROOT, PKG, "csrc")


def test_exports_declared_bound_and_built():
    H = pkg("_hip")
    header = open(os.path.join(ROOT, "include", "dcf_hip.h")).read()
    L = H.lib()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/dcf_hip.h" % name
        assert name in H.SIGNATURES, "%s has no ctypes signature" % name
        assert getattr(L, name) is not None
    assert L.dcf_version() >= 202


def _fusion_cfg(**kw):
    cfg = {"voxel_mode": "compat", "fusion": {"enabled": True, "image_channels": 64},
           "lidar_module": {"out_feature1": 32, "out_feature2": 64, "out_feature3": 128, "out_feature4": 192, "out_feature5": 256}}
    cfg.update(kw)
    return cfg


def test_config_key_default_environment_and_explicit_value(monkeypatch):
    parse = pkg("train").parse_deterministic_config
    monkeypatch.delenv("DCF_DETERMINISTIC", raising=False)
    monkeypatch.delenv("DCF_FUSION_INV", raising=False)
    assert parse(_fusion_cfg()) is False
    assert parse(_fusion_cfg(deterministic=True)) is True
    assert parse(_fusion_cfg(deterministic=False)) is False
    monkeypatch.setenv("DCF_DETERMINISTIC", "1")
    assert parse(_fusion_cfg()) is True                          # the environment is the default of an absent key ...
    assert parse(_fusion_cfg(deterministic=False)) is False      # ... and an explicit false beats it
    monkeypatch.setenv("DCF_DETERMINISTIC", "0")
    assert parse(_fusion_cfg()) is False
    assert parse(_fusion_cfg(deterministic=True)) is True
    for bad in (2, "maybe", 1.5, [True]):
        with pytest.raises(ValueError):
            parse(_fusion_cfg(deterministic=bad))


def test_config_rejected_combinations(monkeypatch):
    parse = pkg("train").parse_deterministic_config
    monkeypatch.delenv("DCF_DETERMINISTIC", raising=False)
    monkeypatch.delenv("DCF_FUSION_INV", raising=False)
    with pytest.raises(ValueError, match="accum"):
        parse(_fusion_cfg(deterministic=True, voxel_mode="accum"))
    assert parse(_fusion_cfg(deterministic=False, voxel_mode="accum")) is False          # the default mode keeps every voxeliser
    with pytest.raises(ValueError, match="image_channels"):
        parse(_fusion_cfg(deterministic=True, fusion={"enabled": True, "image_channels": 96}))
    lm = dict(_fusion_cfg()["lidar_module"], out_feature2=96)
    with pytest.raises(ValueError, match="out_feature2"):
        parse(_fusion_cfg(deterministic=True, lidar_module=lm))
    assert parse(_fusion_cfg(deterministic=True, lidar_module=lm, fusion={"enabled": False})) is True      # no fusion sites: nothing to exclude
    monkeypatch.setenv("DCF_FUSION_INV", "0")
    with pytest.raises(ValueError, match="inverse"):
        parse(_fusion_cfg(deterministic=True))
    monkeypatch.setenv("DCF_DETERMINISTIC", "1")
    with pytest.raises(ValueError):
        parse(_fusion_cfg(voxel_mode="accum"))                   # the environment default is validated like the key


def test_loss_and_model_read_the_key(monkeypatch):
    """The layers that branch on the mode take it from the config (the model without a device: construction is host-side)."""
    import yaml
    monkeypatch.delenv("DCF_DETERMINISTIC", raising=False)
    cfg = yaml.safe_load(open(os.path.join(ROOT, PKG, "config", "config_carla.yaml")))
    parse = pkg("train").parse_deterministic_config
    assert parse(cfg) is False                                   # the shipped configuration: off ...
    monkeypatch.setenv("DCF_DETERMINISTIC", "1")
    assert parse(cfg) is True                                    # ... and the key is left unset there, so the environment can turn it on (bench.py)
    monkeypatch.delenv("DCF_DETERMINISTIC", raising=False)
    assert pkg("loss").LossTotal(cfg).deterministic is False
    assert pkg("loss").LossTotal(dict(cfg, deterministic=True)).deterministic is True
    small = dict(cfg, deterministic=True, voxel_length=64, voxel_width=32)
    small["lidar_module"] = dict(cfg["lidar_module"], out_feature2=48)
    small["fusion"] = dict(enabled=True, K=3, r_max=None, image_channels=64)
    with pytest.raises(ValueError, match="out_feature2"):
        pkg("model").ObjectDetection_DCF(small)


_FLOAT_ATOMIC = re.compile(r"\b(atomicAdd|atomicSub|atomicExch|atomicMax|atomicMin|unsafeAtomicAdd|atomicAdd_system|__hip_atomic_fetch_add)\s*\(")


def _float_atomics(text):
    """(line number, line) of every atomic call in `text` that is not provably on an integer: its first argument must name a
    cursor / counter declared `int *` or `unsigned *` in the same text."""
    ints = set(re.findall(r"\b(?:int|unsigned|int32_t|uint32_t)\s*\*\s*(?:__restrict__\s+)?(\w+)", text))
    found = []
    for no, line in enumerate(text.split("\n"), 1):
        code = line.split("//")[0]
        for m in _FLOAT_ATOMIC.finditer(code):
            arg = code[m.end():].lstrip("&( ")
            name = re.match(r"\w+", arg)
            if name is None or name.group(0) not in ints:
                found.append((no, line.strip()))
    return found


def test_deterministic_sources_hold_no_float_atomics():
    """Files marked DCF-DETERMINISTIC-SOURCE are scanned whole; in the other kernel files every region between DCF-DET-BEGIN and
    DCF-DET-END (the DET branches of the loss kernels).  Integer cursors are allowed."""
    marked, regions = 0, 0
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h", ".cpp")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        if "DCF-DETERMINISTIC-SOURCE" in text:
            marked += 1
            assert not _float_atomics(text), (fn, _float_atomics(text))
            assert "atomicAdd(" in text                          # the scan sees the integer cursors it lets through
        for body in re.findall(r"DCF-DET-BEGIN(.*?)DCF-DET-END", text, flags=re.S):
            regions += 1
            assert not _FLOAT_ATOMIC.search(body), (fn, body[:200])
    assert marked >= 1 and regions >= 4
    # the scan itself: a float atomic is found, an integer cursor is not
    assert _float_atomics("float *g; int *cursor;\natomicAdd(&g[i], v);\natomicAdd(&cursor[k], 1);") == [(2, "atomicAdd(&g[i], v);")]
    # and the default kernels' float atomics sit outside the marked regions (the mode exists because of them)
    assert _float_atomics(open(os.path.join(CSRC, "fusion.hip")).read())

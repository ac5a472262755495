"""GPU: the launches of the train-time sample pipeline (Train.one_step_raw) per combination of its blocks -- which kernels run, in
which order, on which stream -- and what a block that is off leaves behind: no buffer, no launch, no tick of the counter.  The
kernels themselves are pinned elsewhere (test_gpu_augment, test_gpu_augment_image, test_gpu_paste, test_gpu_camera_mask); this file
only watches `_hip.call`.  The tiny trainer, the bank and the staged batch are test_gpu_paste's."""
import pytest
import torch

from _util import pkg
from test_gpu_paste import BEV, IMG, _paste_block, _tiny_cfg, _trainer, world            # noqa: F401 (world is a fixture)

pytestmark = pytest.mark.gpu

PATCHES, IMAGE = "dcf_paste_patches_batch", "dcf_augment_image_batch"
POINTS, MASK, BEV_POINTS, PROJECT = "dcf_paste_points_batch", "dcf_camera_mask_points_batch", "dcf_augment_points_batch", "dcf_project_filter_batch"
PIPELINE = (PATCHES, IMAGE, POINTS, MASK, BEV_POINTS, PROJECT)

# name -> (the blocks that are on, the launches of every step up to and including the projection)
CASES = {
    "none": ((), [PROJECT]),
    "augment": (("augment",), [BEV_POINTS, PROJECT]),
    "augment_image": (("augment_image",), [IMAGE, PROJECT]),
    "augment_paste": (("augment_paste",), [PATCHES, POINTS, PROJECT]),
    "camera_mask": (("fov_crop",), [MASK, PROJECT]),
    "paste_occlusion": (("augment_paste", "paste_occlusion"), [PATCHES, POINTS, MASK, PROJECT]),
    "augment_both": (("augment", "augment_image"), [IMAGE, BEV_POINTS, PROJECT]),
    "all_four": (("augment", "augment_image", "augment_paste", "fov_crop", "paste_occlusion"), [PATCHES, IMAGE, POINTS, MASK, BEV_POINTS, PROJECT]),
}


def _config(on, world):
    over = {}
    if "augment" in on:
        over["augment"] = dict(BEV)
    if "augment_image" in on:
        over["augment_image"] = dict(IMG)
    if "augment_paste" in on:
        over["augment_paste"] = _paste_block(world)
    if "fov_crop" in on or "paste_occlusion" in on:
        over["camera_mask"] = {"fov_crop": "fov_crop" in on, "paste_occlusion": "paste_occlusion" in on}
    return _tiny_cfg(**over)


@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence_streams_counter_and_buffers(case, world, monkeypatch):
    H = pkg("_hip")
    on, want = CASES[case]
    tr = _trainer(_config(on, world))
    log, forward = [], H.call

    def recorder(name, *args):
        log.append((name, args[-1] if args else None))
        return forward(name, *args)

    monkeypatch.setattr(H, "call", recorder)
    compute = torch.cuda.current_stream().cuda_stream
    for step in range(2):
        del log[:]
        tr.one_step_raw(world["geo"], world["batch"])
        torch.cuda.synchronize()
        names = [n for n, _ in log]
        assert PROJECT in names
        seen = [(n, s) for n, s in log[:names.index(PROJECT) + 1] if n in PIPELINE]
        print(case, step, [n for n, _ in seen])
        assert [n for n, _ in seen] == want, (case, step)
        # the image launches on the compute stream; the point launches and the projection on ONE other stream
        assert all(s == compute for n, s in seen if n in (PATCHES, IMAGE))
        side = set(s for n, s in seen if n not in (PATCHES, IMAGE))
        assert len(side) == 1 and compute not in side and side == {tr._side.cuda_stream}
    monkeypatch.undo()
    # the counter ticks once per step iff a block that draws is on; the mask alone draws nothing
    assert tr.aug_calls == (2 if set(on) & {"augment", "augment_image", "augment_paste"} else 0)
    keys = set(k for st in tr._geo_sets.values() for k in st)
    assert len(tr._geo_sets) == 2
    if "augment" in on:
        assert tr.augment is not None and "aug" in keys
    else:
        assert tr.augment is None and "aug" not in keys
    if "augment_image" in on:
        assert tr.image_augment is not None and tr._aug_image is not None
    else:
        assert tr.image_augment is None and tr._aug_image is None
    if "augment_paste" in on:
        assert tr.paste is not None and tr._paste_image_buf is not None and "paste" in keys and len(tr.last_paste) == 2
    else:
        assert tr.paste is None and tr._paste_image_buf is None and tr._paste_dev is None and tr._paste_bank is None
        assert "paste" not in keys and tr.last_paste == []
    if "fov_crop" in on or "paste_occlusion" in on:
        assert tr.camera_mask is not None
        assert ("mask" in keys) == ("augment_paste" not in on)                # pasted frames are masked in place
    else:
        assert tr.camera_mask is None and "mask" not in keys
    assert (len(tr.last_masked) == 2) if "paste_occlusion" in on else (tr.last_masked == [])

"""CPU suite: the host statement of `loss_sampling: hard` (loss.hard_negatives / float_order / LossTotal on CPU tensors) -- what the
device selection of csrc/loss.hip is compared with bit for bit in tests/test_gpu_loss_hard.py."""
import numpy as np
import pytest
import torch

from _util import M64, golden_cfg, load_golden, pkg, rand32
from test_gpu_loss_sampling import _setup, sampler_statement


def _hard_cfg(n_boxes, **over):
    cfg, boxes, nb, cls, reg, H, W = _setup(n_boxes, far=n_boxes >= 3)
    return dict(cfg, loss_sampling="hard", **over), boxes, nb, cls, reg, H, W


def test_unknown_mode_names_all_three():
    cfg = _hard_cfg(0)[0]
    with pytest.raises(ValueError) as e:
        pkg("loss").LossTotal(dict(cfg, loss_sampling="hardest"))
    assert all(m in str(e.value) for m in ("compat", "device", "hard"))


def test_key_map_is_monotone():
    Lm = pkg("loss")
    tiny = np.float32(1e-45)                                  # the smallest denormal
    vals = np.array([-np.inf, -3.0e38, -1.0e30, -65504.0, -2.5, -1.0, -1e-3, -1.2e-38, -2 * tiny, -tiny, -0.0, 0.0, tiny, 2 * tiny,
                     1.2e-38, 1e-3, 1.0, 1.0000001, 2.5, 3.0e38, np.inf], dtype=np.float32)
    assert tiny > 0 and np.all(np.diff(vals) >= 0)            # sorted; -0.0 == +0.0 as floats
    o = Lm.float_order(vals).astype(np.int64)
    assert np.all(np.diff(o) >= 0)
    differ = vals[1:] != vals[:-1]
    assert np.all(np.diff(o)[differ] > 0)
    iz = int(np.flatnonzero(np.signbit(vals) & (vals == 0))[0])
    assert o[iz] < o[iz + 1] and vals[iz + 1] == 0 and not np.signbit(vals[iz + 1])      # ord(-0.0) < ord(+0.0)
    # random bit patterns (no NaN): the order of the floats is the order of the keys
    r = np.random.RandomState(0).randint(0, 1 << 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    i, j = r[:-1], r[1:]
    oi, oj = Lm.float_order(i).astype(np.int64), Lm.float_order(j).astype(np.int64)
    assert np.all((i < j) <= (oi < oj)) and np.all((i > j) <= (oi > oj))


def _brute(cls_b, window, want):
    """The definition, literally: candidates sorted by (-key, cell)."""
    HW = cls_b.shape[1]
    def ord32(x):
        u = int(np.float32(x).view(np.uint32))
        return (u ^ 0x80000000) if not (u & 0x80000000) else (~u & 0xFFFFFFFF)
    keyed = []
    win = set(window)
    for cell in range(HW):
        if cell in win:
            continue
        d0 = np.float32(cls_b[1, cell]) - np.float32(cls_b[0, cell])
        d1 = np.float32(cls_b[3, cell]) - np.float32(cls_b[2, cell])
        keyed.append((-max(ord32(d0), ord32(d1)), cell))
    return [c for _, c in sorted(keyed)[:want]]


@pytest.mark.parametrize("n_boxes", [0, 3, 20])
def test_host_statement_equals_brute_force(n_boxes):
    cfg, boxes, nb, cls, reg, H, W = _hard_cfg(n_boxes)
    Lm = pkg("loss")
    L = Lm.LossTotal(cfg)
    want = cfg["neg_sample_threshold"] + 1
    g = torch.Generator().manual_seed(4)
    variants = [cls, torch.round(cls * 8) / 8, torch.full_like(cls, 0.5), -cls * torch.rand(cls.shape, generator=g) * 1e3]
    for v in variants:
        for b in range(boxes.shape[0]):
            window = L.windows(boxes[b, :int(nb[b])].numpy(), H, W)[0]
            sc = v[b].reshape(4, H * W).numpy()
            got = Lm.hard_negatives(sc, window, want).tolist()
            assert got == _brute(sc, window, want)
            assert len(set(got)) == len(got) == want and not (set(got) & set(window))
    # fewer candidates than asked for: all of them, in order
    sc = cls[0].reshape(4, H * W).numpy()[:, :100]
    window = list(range(0, 100, 3))
    got = Lm.hard_negatives(sc, window, want).tolist()
    assert got == _brute(sc, window, want) and len(got) == 100 - len(window)
    assert Lm.hard_negatives(sc, list(range(100)), want).tolist() == []


def test_numpy_hash_equals_the_python_restatement():
    Lm = pkg("loss")
    for args in ((0, 0, 1, 0, 0), (12345678901234567, 3, 2, 511, 7), (M64, 15, 1, 1023, 0), (42, 1, 2, 128, 1000), (2 ** 63 + 5, 7, 2, 99999, 3)):
        assert int(Lm.sample_rand(args[0], args[1], args[2], [args[3]], args[4])[0]) == rand32(*args)
    idx = np.arange(300)
    assert Lm.sample_rand(77, 2, 1, idx).tolist() == [rand32(77, 2, 1, int(i), 0) for i in idx]


@pytest.mark.parametrize("n_boxes", [3, 20])
def test_positives_are_those_of_the_device_sampler(n_boxes):
    cfg, boxes, nb, cls, reg, H, W = _hard_cfg(n_boxes)
    L = pkg("loss").LossTotal(cfg)
    L.keep_samples = True
    for call in range(2):
        L(boxes, nb, cls, reg)
        pos, neg, counts = [t.numpy() for t in L.last_samples]
        seed = (cfg["loss_seed"] * 0x9E3779B1 + call) & M64
        for b in range(boxes.shape[0]):
            want_pos, _, n_entries = sampler_statement(L, boxes[b].numpy(), int(nb[b]), H, W, seed, b)
            assert [int(v) for v in pos[b] if v >= 0] == want_pos
            assert list(counts[b, :2]) == [len(want_pos), n_entries]
    assert L.calls == 2
    if n_boxes == 20:
        assert int(counts[0, 1]) > cfg["pos_sample_threshold"]


@pytest.mark.parametrize("reduction", ["last", "mean"])
def test_forward_backward_on_cpu_tensors(reduction):
    cfg, boxes, nb, cls, reg, H, W = _hard_cfg(20, loss_reduction=reduction)
    L = pkg("loss").LossTotal(cfg)
    L.keep_samples = True
    c, r = cls.clone().requires_grad_(True), reg.clone().requires_grad_(True)
    state = np.random.get_state()[1].copy()
    loss = L(boxes, nb, c, r)
    loss.backward()
    assert np.array_equal(np.random.get_state()[1], state)              # numpy's generator is not consumed
    assert np.isfinite(loss.item())
    pos, neg, counts = [t.numpy() for t in L.last_samples]
    B = boxes.shape[0]
    for b in range(B):
        listed = set(int(v) for v in pos[b] if v >= 0) | set(int(v) for v in neg[b] if v >= 0)
        hit = set(np.flatnonzero((c.grad[b].reshape(4, H * W) != 0).any(0).numpy()).tolist())
        if reduction == "last" and b != B - 1:
            assert not hit
        else:
            assert hit == listed
            window = set(L.windows(boxes[b, :int(nb[b])].numpy(), H, W)[0])
            assert set(np.flatnonzero((r.grad[b].reshape(14, H * W) != 0).any(0).numpy()).tolist()) <= window
            assert int(counts[b, 2]) == cfg["neg_sample_threshold"] + 1 and not (set(int(v) for v in neg[b]) & window)


def test_no_candidates_means_no_negative_term():
    """Every cell inside a window: the negative list is empty and the loss is the positive and regression terms alone."""
    z = load_golden("model_tiny.npz")
    cfg = dict(golden_cfg(z), loss_sampling="hard", loss_reduction="mean", positive_range=40)
    H, W = int(cfg["voxel_length"] / 4), int(cfg["voxel_width"] / 4)
    L = pkg("loss").LossTotal(cfg)
    L.keep_samples = True
    boxes = torch.zeros(1, cfg["max_num_bbox"], 9)
    x = 0.5 * (cfg["lidar_x_min"] + cfg["lidar_x_max"])
    y = 0.5 * (cfg["lidar_y_min"] + cfg["lidar_y_max"])
    boxes[0, 0] = torch.tensor([x, y, -1.0, 4.0, 1.8, 1.5, 0.3, 6, 1])
    g = torch.Generator().manual_seed(1)
    c = torch.rand(1, 4, H, W, generator=g).requires_grad_(True)
    r = (torch.rand(1, 14, H, W, generator=g) - 0.5).requires_grad_(True)
    loss = L(boxes, torch.tensor([1]), c, r)
    loss.backward()
    counts = L.last_samples[2].numpy()
    assert int(counts[0, 1]) == H * W and int(counts[0, 2]) == 0 and (L.last_samples[1].numpy() == -1).all()
    assert np.isfinite(loss.item()) and float(c.grad.abs().sum()) > 0

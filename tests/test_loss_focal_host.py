"""CPU suite: the host statement of `loss_sampling: focal` (loss.focal_terms / parse_focal_config / LossTotal on CPU tensors, DESIGN.md
section 16) -- what the device entry of csrc/loss.hip is compared with in tests/test_gpu_loss_focal.py."""
import numpy as np
import pytest
import torch

from _focal_util import B, case, positive_set, regression_input, scores, statement
from _util import pkg

PAIRS = [(0.25, 0.0), (0.25, 1.0), (0.25, 2.0), (0.5, 2.5)]


def _labels(rows):
    """cfg of the 64 x 48 map and one sample holding the given (x, y) boxes."""
    cfg, _, _, H, W = case("64x48-0")
    boxes = np.zeros((max(len(rows), 1), 9), np.float32)
    for k, (x, y) in enumerate(rows):
        boxes[k] = (x, y, -1.0, 4.0, 1.8, 1.5, 0.3 * k, 6, 1)
    return cfg, boxes, len(rows), H, W


@pytest.mark.parametrize("rows, entries, distinct", [
    ([(0.05, -9.55)], 9, 9),                            # a map corner: the 5 x 5 window is clipped to 3 x 3
    ([(10.0, 0.0), (10.8, 0.5)], 50, 50 - 12),          # centre cells (25, 24) and (27, 25): the windows share 3 x 4 cells
    ([(40.0, 3.0)], 0, 0),                              # off the grid: no window
    ([], 0, 0),
    ([(40.0, 3.0), (0.05, -9.55), (10.0, 0.0), (10.0, 0.0)], 9 + 50, 9 + 25),     # the same window twice
])
def test_positive_cells_equal_the_literal_set(rows, entries, distinct):
    cfg, boxes, nb, H, W = _labels(rows)
    assert cfg["positive_range"] == 5
    L = pkg("loss").LossTotal(cfg)
    cells = L.windows(boxes[:nb], H, W)[0]
    want, n_entries = positive_set(L, boxes, nb, H, W)
    assert set(cells) == want and len(cells) == n_entries == entries and len(want) == distinct
    # the count the loss reports, and N_b = max(1, |P_b|) in the value
    cls = scores("uniform", H, W)[:1]
    value, grad = pkg("loss").focal_terms(cls[0].reshape(4, H * W).numpy(), cells, 0.25, 2.0, 1e-12)
    Lc = pkg("loss").LossTotal(cfg)
    loss = Lc(torch.from_numpy(boxes)[None], torch.tensor([nb]), cls, regression_input(H, W)[:1])
    assert int(Lc.last_terms[0, 2]) == distinct and abs(float(Lc.last_terms[0, 0]) - value) <= 2e-6 * max(1.0, abs(value))
    assert np.isfinite(loss.item())
    pos = np.zeros(H * W, bool)
    pos[list(want)] = True
    for a in range(2):                                  # the gradient sits in the channel of the label, the other one gets 0
        assert (grad[2 * a][pos] == 0).all() and (grad[2 * a + 1][~pos] == 0).all()
        assert (grad[2 * a + 1][pos] < 0).all() and (grad[2 * a][~pos] < 0).all()


def _torch_focal(c, y, alpha, gamma):
    """The definition written with torch ops in float64 (no clamp: for q > eps)."""
    alpha_t = torch.where(y, torch.tensor(alpha, dtype=torch.float64), torch.tensor(1.0 - alpha, dtype=torch.float64))
    total = 0.0
    for a in range(2):
        q = torch.where(y, c[2 * a + 1], c[2 * a])
        factor = torch.ones_like(q) if gamma == 0 else (1.0 - q) ** gamma
        total = total + (-alpha_t * factor * torch.log(q)).sum()
    return total / max(1, int(y.sum()))


@pytest.mark.parametrize("alpha, gamma", PAIRS)
def test_closed_form_gradient_equals_autograd(alpha, gamma):
    HW = 600
    g = torch.Generator().manual_seed(int(10 * gamma) + 1)
    logits = torch.randn(2, 2, HW, generator=g, dtype=torch.float64) * 4.0
    c = torch.softmax(logits, 1).reshape(4, HW)                   # probabilities from ~1e-9 up, all above eps and below 1
    c = torch.cat((c, torch.rand(4, 100, generator=g, dtype=torch.float64) * 0.98 + 0.01), 1)
    HW = c.shape[1]
    cells = list(range(0, HW, 7)) + [3, 3, 14]                    # duplicates count once
    y = torch.zeros(HW, dtype=torch.bool)
    y[cells] = True
    value, grad = pkg("loss").focal_terms(c.numpy(), cells, alpha, gamma, 1e-12)
    ct = c.clone().requires_grad_(True)
    ref = _torch_focal(ct, y, alpha, gamma)
    ref.backward()
    assert float(c.min()) > 1e-12 and float(c.max()) < 1.0
    np.testing.assert_allclose(value, ref.item(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(grad, ct.grad.numpy(), rtol=1e-12, atol=0)
    assert np.count_nonzero(grad) == 2 * HW


def test_gamma_zero_is_the_weighted_log_loss():
    HW = 500
    c = torch.rand(4, HW, generator=torch.Generator().manual_seed(3), dtype=torch.float64).numpy() * 0.98 + 0.01
    cells = list(range(0, HW, 9))
    y = np.zeros(HW, bool)
    y[cells] = True
    value, grad = pkg("loss").focal_terms(c, cells, 0.5, 0.0, 1e-12)
    log_loss = sum(-np.log(np.where(y, c[2 * a + 1], c[2 * a])).sum() for a in range(2)) / len(cells)
    np.testing.assert_allclose(value, 0.5 * log_loss, rtol=1e-14)
    np.testing.assert_allclose(grad[1][y], -0.5 / (c[1][y] * len(cells)), rtol=1e-14)


@pytest.mark.parametrize("alpha, gamma", PAIRS)
def test_saturated_scores(alpha, gamma):
    """p_t = 1: value 0, finite gradient.  p_t = 0 and a denormal: the clamp, the gradient taken at eps."""
    Lm = pkg("loss")
    eps = 1e-12
    HW, cells = 8, [1, 2]
    y = np.zeros(HW, bool)
    y[cells] = True
    one = np.zeros((4, HW))
    for a in range(2):
        one[2 * a + 1][y] = 1.0
        one[2 * a][~y] = 1.0
    value, grad = Lm.focal_terms(one, cells, alpha, gamma, eps)
    assert value == 0.0 and np.isfinite(grad).all()
    if gamma == 0:
        assert grad[1][1] == -alpha / 2 and grad[0][0] == -(1 - alpha) / 2
    elif gamma > 1:
        assert not grad.any()
    for tiny in (0.0, float(np.float32(1e-42)), 1e-300):
        zero = 1.0 - one                                          # every p_t ...
        zero[one == 1.0] = tiny                                   # ... is 0 or the tiny value
        value, grad = Lm.focal_terms(zero, cells, alpha, gamma, eps)
        om = 1.0 - eps
        fl = -(om ** gamma if gamma else 1.0) * np.log(eps)
        g = -1.0 / eps if gamma == 0 else gamma * om ** (gamma - 1.0) * np.log(eps) - om ** gamma / eps
        want_value = 2 * (2 * alpha + (HW - 2) * (1 - alpha)) * fl / 2
        np.testing.assert_allclose(value, want_value, rtol=1e-13)
        np.testing.assert_allclose(grad[1][y], alpha * g / 2, rtol=1e-13)
        np.testing.assert_allclose(grad[2][~y], (1 - alpha) * g / 2, rtol=1e-13)
        assert np.isfinite(grad).all() and not grad[0][y].any() and not grad[3][~y].any()


def test_a_nan_score_stays_nan_at_its_cell_only():
    HW, cells = 50, [4, 5, 6]
    c = torch.rand(4, HW, generator=torch.Generator().manual_seed(5), dtype=torch.float64).numpy() * 0.9 + 0.05
    for ch, cell in ((1, 5), (2, 20)):                            # a positive cell's object score, a background cell's background score
        cn = c.copy()
        cn[ch, cell] = np.nan
        for gamma in (0.0, 1.0, 2.0):
            value, grad = pkg("loss").focal_terms(cn, cells, 0.25, gamma, 1e-12)
            assert np.isnan(value)
            bad = np.isnan(grad)
            assert bad[ch, cell] and bad.sum() == 1 and np.isfinite(grad[~bad]).all()
    cn = c.copy()
    cn[0, 5] = np.nan                                             # the channel the label does not read: no effect
    value, grad = pkg("loss").focal_terms(cn, cells, 0.25, 2.0, 1e-12)
    assert np.isfinite(value) and np.isfinite(grad).all()


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
@pytest.mark.parametrize("name", ["64x48-20", "16x8"])
def test_reductions_and_terms_on_cpu_tensors(name, reduction):
    cfg, boxes, nb, H, W = case(name, loss_reduction=reduction)
    cls, reg = scores("uniform", H, W), regression_input(H, W)
    L = pkg("loss").LossTotal(cfg)
    c, r = cls.clone().requires_grad_(True), reg.clone().requires_grad_(True)
    state = np.random.get_state()[1].copy()
    loss = L(boxes, nb, c, r)
    loss.backward()
    assert np.array_equal(np.random.get_state()[1], state) and L.calls == 0          # nothing is drawn
    want = statement(cfg, boxes, nb, cls, reg, H, W)
    # fp32 outputs of a float64 classification term and the fp32 torch regression term: the project's fp32-against-float64 bounds
    assert abs(loss.item() - want[0]) <= 2e-6 * max(1.0, abs(want[0]))
    np.testing.assert_allclose(c.grad.double().numpy(), want[1], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r.grad.double().numpy(), want[2], rtol=1e-5, atol=1e-7)
    t = L.last_terms.double().numpy()
    assert L.last_terms.shape == (B, 3) and L.last_terms.dtype == torch.float32
    assert np.array_equal(t[:, 2], want[3][:, 2])
    np.testing.assert_allclose(t[:, :2], want[3][:, :2], rtol=2e-6, atol=2e-6)
    gain = cfg["regress_loss_gain"]
    per = t[:, 0] + gain * t[:, 1]
    expect = {"last": per[-1], "sum": per.sum(), "mean": per.mean()}[reduction]
    assert abs(loss.item() - expect) <= 2e-6 * max(1.0, abs(expect))
    if reduction == "last":
        assert not t[:-1].any() and not c.grad[:-1].any() and not r.grad[:-1].any() and c.grad[-1].abs().sum() > 0
    else:
        assert (c.grad.reshape(B, 2, 2, -1) != 0).any(2).all()       # every cell of both anchors has a gradient
        if name == "64x48-20":
            n_entries = [positive_set(L, boxes[b].numpy(), int(nb[b]), H, W)[1] for b in range(B)]
            assert all(t[b, 2] < n_entries[b] for b in range(B))      # overlapping windows: cells counted once


def test_no_labels_is_all_background_with_unit_normaliser():
    cfg, boxes, nb, H, W = case("64x48-0", loss_reduction="sum")
    cls, reg = scores("uniform", H, W), regression_input(H, W)
    L = pkg("loss").LossTotal(cfg)
    loss = L(boxes, nb, cls, reg)
    c = cls.double().reshape(B, 2, 2, -1)
    want = float((-0.75 * (1 - c[:, :, 0]) ** 2 * torch.log(c[:, :, 0])).sum())
    assert abs(loss.item() - want) <= 2e-6 * want and not L.last_terms[:, 1:].any()
    # nbox beyond the label rows is clamped to them
    cfg, boxes, nb, H, W = case("16x8", loss_reduction="sum")
    boxes = boxes[:, :1].contiguous()                            # one label row, a box in every sample
    a = pkg("loss").LossTotal(cfg)(boxes, torch.tensor([8] * B), scores("uniform", H, W), regression_input(H, W))
    b = pkg("loss").LossTotal(cfg)(boxes, torch.tensor([1] * B), scores("uniform", H, W), regression_input(H, W))
    assert torch.equal(a, b) and np.isfinite(a.item())


@pytest.mark.parametrize("key, value", [
    ("focal_alpha", 0.0), ("focal_alpha", 1.0), ("focal_alpha", -0.1), ("focal_alpha", "0.25"), ("focal_alpha", float("nan")),
    ("focal_gamma", 0.5), ("focal_gamma", -1.0), ("focal_gamma", 0.999), ("focal_gamma", float("inf")), ("focal_gamma", True),
    ("focal_eps", 0.0), ("focal_eps", 2e-3), ("focal_eps", -1e-12), ("focal_eps", None),
])
def test_bad_focal_keys_raise(key, value):
    cfg = case("16x8")[0]
    Lm = pkg("loss")
    with pytest.raises(ValueError) as e:
        Lm.LossTotal(dict(cfg, **{key: value}))
    assert key in str(e.value)
    with pytest.raises(ValueError):
        Lm.parse_focal_config({key: value})
    for mode in ("compat", "device", "hard"):                     # the other modes never look at the keys
        L = Lm.LossTotal(dict(cfg, loss_sampling=mode, **{key: value}))
        assert L.focal is None and L.last_terms is None


def test_defaults_and_accepted_values():
    Lm = pkg("loss")
    assert Lm.parse_focal_config({}) == (0.25, 2.0, 1e-12)
    assert Lm.parse_focal_config({"focal_alpha": 0.5, "focal_gamma": 0, "focal_eps": 1e-3}) == (0.5, 0.0, 1e-3)
    assert Lm.parse_focal_config({"focal_gamma": 1}) == (0.25, 1.0, 1e-12)
    cfg = case("16x8")[0]
    L = Lm.LossTotal(cfg)
    assert L.sampling == "focal" and L.focal == (0.25, 2.0, 1e-12)
    with pytest.raises(ValueError) as e:
        Lm.LossTotal(dict(cfg, loss_sampling="focus"))
    assert "focal" in str(e.value)

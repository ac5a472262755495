"""CPU suite: the host statements of the rotated-IoU regression term (`iou_loss_gain`) -- loss.anchor_iou_terms,
loss.iou_value_grad, the config keys and LossTotal on CPU tensors -- what csrc/loss_iou.hip is compared with in tests/test_gpu_loss_iou.py."""
import numpy as np
import pytest
import torch

from _anchor_util import B, MAPS, assigned, case, config, terms_statement
from _focal_util import close, scores
from _iou_loss_util import KINDS, case_iou, close_iou, kinds_present, margin, pairs, regression, statement
from _util import pkg


@pytest.mark.parametrize("name", list(MAPS))
def test_the_committed_inputs_hold_every_kind_of_pair(name):
    n = kinds_present(name)
    print(name, n)
    assert all(v > 0 for v in n.values()), n


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("kind", KINDS)
def test_the_value_is_iou_pair(name, kind):
    """The statement's per-anchor IoU against evalkitti.iou_pair on the decoded boxes at 1e-13; the edge-clip form (the device's arithmetic)
    against it at 1e-12 where the pair keeps 1e-6 m from a change of topology; L, N and the IoU sum from the map."""
    Lm, EK = pkg("loss"), pkg("evalkitti")
    cfg, boxes, nb, H, W = case_iou(name, kind)
    targets, anc = assigned(name)
    reg = regression(name)
    for b, (j, p, q) in enumerate(pairs(name)):
        n = max(min(int(nb[b]), boxes.shape[1]), 0)
        L, n_pos, iou_sum, grad, iou_map = Lm.anchor_iou_terms(reg[b].reshape(14, H * W).numpy(), anc, boxes[b, :n].numpy(), targets[b][0], kind)
        want = np.array([EK.iou_pair(p[i], q[i])[0 if kind == "bev" else 1] for i in range(len(j))]).reshape(-1)
        got = iou_map.reshape(-1)
        assert n_pos == len(j) == targets[b][2][0] and np.count_nonzero(got) <= len(j)
        assert np.abs(got[j] - want).max(initial=0.0) <= 1e-13
        assert abs(iou_sum - want.sum()) <= 1e-12 and abs(L - (1.0 - want).sum() / max(1, n_pos)) <= 1e-13
        if len(j):
            edge, _ = Lm.iou_value_grad(p, q, kind)
            ok = margin(p, q, kind) >= 1e-6
            print("%s %s sample %d: %d pairs, max |edge clip - polygon clip| %.3g" % (name, kind, b, len(j), np.abs(edge - want)[ok].max()))
            assert ok.all() and np.abs(edge - want).max() <= 1e-12
        rows = np.zeros((2, 7, H * W), bool)
        rows.reshape(2, 7, -1)[j // (H * W), :, j % (H * W)] = True
        assert not grad.reshape(2, 7, -1)[~rows].any()                 # nothing but the positives' seven offsets gets a gradient


def test_the_gradient_equals_central_differences_of_the_value():
    """d L / d offset_c of every positive anchor of every map against central differences (step 1e-6) of the statement's own value, at
    1e-7 absolute.  Only IoU_j depends on anchor j's offsets, so the difference quotient of L by that offset is -(IoU_j(+h) - IoU_j(-h)) /
    (2 h max(1, N)) of the statement's per-anchor values: channel c of all positives moves at once, one pair of calls per channel.  Rows
    within 1e-3 m of a change of topology (a corner of one rectangle on an edge line of the other, two z faces level) are left out -- the
    value has a kink there --, and they are at most 10 % of the rows.

    The same rows, per pair and without the 1 / N: d IoU / d p of loss.iou_value_grad against central differences of ITS value (the edge
    clip relative to the label's centre) at 1e-7 as well; measured 4.1e-9.  (Per pair, the polygon clip's value is no reference at this
    step: its shoelace sums products of absolute coordinates, about 2000 m^2 at 70 m, and their rounding, 1e-13 in the IoU, is 1.7e-7 after
    the division by 2e-6 -- measured on the 96x80 map.)"""
    Lm = pkg("loss")
    h = 1e-6
    for kind in KINDS:
        rows = left_out = 0
        worst = worst_pair = 0.0
        for name in MAPS:
            cfg, boxes, nb, H, W = case_iou(name, kind)
            HW = H * W
            targets, anc = assigned(name)
            reg = regression(name).double().numpy().reshape(B, 14, HW)
            for b, (j, p, q) in enumerate(pairs(name)):
                if not len(j):
                    continue
                n = max(min(int(nb[b]), boxes.shape[1]), 0)
                call = lambda r: Lm.anchor_iou_terms(r, anc, boxes[b, :n].numpy(), targets[b][0], kind)
                _, n_pos, _, grad, _ = call(reg[b])
                a, cell = j // HW, j % HW
                keep = margin(p, q, kind) >= 1e-3
                rows += len(j)
                left_out += int((~keep).sum())
                _, gp = Lm.iou_value_grad(p, q, kind)
                for c in range(7):
                    up, dn = reg[b].copy(), reg[b].copy()
                    up[7 * a + c, cell] += h
                    dn[7 * a + c, cell] -= h
                    fd = -(call(up)[4].reshape(-1)[j] - call(dn)[4].reshape(-1)[j]) / (2 * h * max(1, n_pos))
                    worst = max(worst, float(np.abs(grad[7 * a + c, cell] - fd)[keep].max(initial=0.0)))
                    d = np.zeros(7)
                    d[c] = h
                    fd = (Lm.iou_value_grad(p + d, q, kind)[0] - Lm.iou_value_grad(p - d, q, kind)[0]) / (2 * h)
                    worst_pair = max(worst_pair, float(np.abs(gp[:, c] - fd)[keep].max(initial=0.0)))
        print("%s: %d rows, %d left out, worst |gradient - central difference| %.3g; per pair, edge clip: %.3g" % (kind, rows, left_out, worst, worst_pair))
        assert rows > 100 and left_out <= 0.1 * rows
        assert worst <= 1e-7 and worst_pair <= 1e-7


def test_disjoint_and_non_finite_rows():
    Lm = pkg("loss")
    q = np.array([[10.0, 2.0, -1.0, 4.0, 1.8, 1.5, 0.3]] * 4)
    p = q.copy()
    p[0, 0] += 20.0                       # far away
    p[1, 2] += 5.0                        # above: bird's-eye overlap only
    p[2, 3] = np.nan
    p[3, 6] = np.inf
    for kind in KINDS:
        iou, g = Lm.iou_value_grad(p, q, kind)
        assert iou[0] == 0 and not g[0].any()
        assert np.isnan(iou[2:]).all() and np.isnan(g[2:]).all()
        if kind == "3d":
            assert iou[1] == 0 and not g[1].any()
        else:
            assert abs(iou[1] - 1.0) <= 1e-15                      # same footprint: the z shift does not enter
    same, g = Lm.iou_value_grad(q[:1], q[:1], "3d")              # coincident edges: p's are kept, q's dropped, the area counted once
    assert abs(same[0] - 1.0) <= 1e-15


@pytest.mark.parametrize("key, value", [("iou_loss_gain", -0.5), ("iou_loss_gain", float("nan")), ("iou_loss_gain", float("inf")),
                                        ("iou_loss_gain", "2"), ("iou_loss_gain", True), ("iou_loss_gain", None), ("iou_loss_kind", "2d"),
                                        ("iou_loss_kind", 3), ("iou_loss_kind", None)])
def test_bad_keys_raise(key, value):
    with pytest.raises(ValueError):
        pkg("loss").LossTotal(config(16, 8, **{key: value}))


@pytest.mark.parametrize("sampling", ["compat", "device", "hard", "focal"])
def test_a_gain_needs_the_anchor_mode(sampling):
    with pytest.raises(ValueError):
        pkg("loss").LossTotal(config(16, 8, loss_sampling=sampling, iou_loss_gain=1.0))
    L = pkg("loss").LossTotal(config(16, 8, loss_sampling=sampling, iou_loss_gain=0, iou_loss_kind="bev"))         # off: any mode
    assert L.iou_gain == 0.0 and L.last_iou is None


def test_defaults():
    Lm = pkg("loss")
    L = Lm.LossTotal(config(16, 8))
    assert (L.iou_gain, L.iou_kind) == (0.0, "3d") and L.last_iou is None
    L = Lm.LossTotal(config(16, 8, iou_loss_gain=1, iou_loss_kind="bev"))
    assert (L.iou_gain, L.iou_kind) == (1.0, "bev") and isinstance(L.iou_gain, float)
    with pytest.raises(ValueError):
        Lm.anchor_iou_terms(np.zeros((14, 4)), np.ones((2, 7, 4)), np.zeros((0, 7)), np.full(8, -1), "2d")


def _run_cpu(cfg, boxes, nb, cls, reg, keep=False):
    L = pkg("loss").LossTotal(cfg)
    L.keep_samples = keep
    c1, r1 = cls.clone().requires_grad_(True), reg.clone().requires_grad_(True)
    loss = L(boxes, nb, c1, r1)
    loss.backward()
    return L, loss.detach(), c1.grad, r1.grad


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_without_a_gain_the_cpu_loss_is_bit_for_bit_what_it_was(reduction):
    name = "37x29"
    cfg, boxes, nb, H, W = case(name, loss_reduction=reduction)
    cls, reg = scores("softmax", H, W), regression(name)
    targets, anc = assigned(name)
    want = terms_statement(cfg, anc, boxes, nb, [t for t, _, _ in targets], cls, reg, H, W)
    base = _run_cpu(cfg, boxes, nb, cls, reg, keep=True)
    close(base[1].item(), base[2], base[3], base[0].last_terms, want)
    assert base[0].last_iou is None and len(base[0].last_samples) == 3
    for over in (dict(iou_loss_gain=0), dict(iou_loss_gain=0.0, iou_loss_kind="bev")):
        off = _run_cpu(dict(cfg, **over), boxes, nb, cls, reg, keep=True)
        assert off[0].last_iou is None and len(off[0].last_samples) == 3
        for a, b in zip(off[1:], base[1:]):
            assert torch.equal(a, b)
        assert torch.equal(off[0].last_terms, base[0].last_terms)


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
@pytest.mark.parametrize("kind", KINDS)
def test_with_a_gain_the_cpu_loss_is_the_anchor_terms_plus_the_iou_term(kind, reduction):
    name = "37x29"
    cfg, boxes, nb, H, W, cls, reg, want = statement(name, kind, "softmax", loss_reduction=reduction)
    L, loss, gc, gr = _run_cpu(cfg, boxes, nb, cls, reg, keep=True)
    print("loss %.9g want %.9g; iou terms %s" % (loss.item(), want[0], L.last_iou.tolist()))
    close(loss.item(), gc, gr, L.last_terms, want[:4])
    close_iou(L.last_iou, want[4])
    off = _run_cpu(dict(cfg, iou_loss_gain=0), boxes, nb, cls, reg)
    assert torch.equal(off[2], gc) and not torch.equal(off[3], gr) and loss.item() > off[1].item()       # the term moves reg alone
    target, best, counts, iou_map = L.last_samples
    assert iou_map.shape == (B, 2, H * W) and iou_map.dtype == torch.float64
    counted = [B - 1] if reduction == "last" else range(B)
    for b in counted:
        assert np.abs(iou_map[b].numpy() - want[5][b]).max() <= 1e-13
    if reduction == "last":
        assert not iou_map[:B - 1].any() and not L.last_iou[:B - 1].any()
    n = want[4][:, 1]
    mean = want[4][:, 0]
    assert ((mean >= 0) & (mean <= 1)).all() and n[B - 1] >= 1

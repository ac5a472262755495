"""CPU suite: the host statements of `loss_sampling: anchor` (assign.anchor_iou / anchor_targets, loss.anchor_terms, LossTotal on CPU
tensors) -- what the device entries of csrc/loss.hip are compared with in tests/test_gpu_loss_anchor.py."""
import math

import numpy as np
import pytest
import torch

from _anchor_util import B, MAPS, MARGIN, PITCH, SPECIAL, anchors_of, assigned, case, config, margins, terms_statement, yaw_condition
from _focal_util import regression_input, scores
from _util import pkg

POS, NEG = 0.6, 0.45


def _row(x, y, l, w, yaw):
    return np.array([x, y, -1.0, l, w, 1.5, yaw, 6, 1], np.float32)


def _small():
    """The 16 x 8 map: its config, anchors [2, 7, 128], and the row of anchor (a, cell)."""
    cfg = config(16, 8)
    anc = anchors_of(cfg)
    return cfg, anc, lambda a, cell: _row(anc[a, 0, cell], anc[a, 1, cell], anc[a, 3, cell], anc[a, 4, cell], anc[a, 6, cell])


def test_a_label_equal_to_an_anchor_is_that_anchors_target():
    cfg, anc, anchor = _small()
    A = pkg("assign")
    HW = 128
    for a, cell in ((0, 37), (1, 90)):
        rows = np.stack([anchor(1 - a, 5), anchor(a, cell)])
        target, best, counts = A.anchor_targets(anc, rows, POS, NEG)
        j = a * HW + cell
        assert abs(best[j] - 1.0) <= 1e-12 and best[j] >= best.max() - 1e-12 and target[j] == 1 and target[(1 - a) * HW + 5] == 0
        assert counts[0] == int((target >= 0).sum()) >= 2 and counts[2] == 0 and counts[3] == 0
        assert counts[1] == int((target == -2).sum()) and set(np.unique(target)) <= {-2, -1, 0, 1}


def test_a_diagonal_label_is_taught_by_its_forced_anchor_alone():
    cfg, anc, anchor = _small()
    A = pkg("assign")
    rows = _row(anc[0, 0, 60] + 0.3, anc[0, 1, 60] - 0.3, 4.8, 1.6, math.pi / 4 + 0.05)[None]
    I = A.anchor_iou(anc, rows)
    target, best, counts = A.anchor_targets(anc, rows, POS, NEG)
    assert 0 < best.max() < NEG                                     # no anchor reaches even the negative threshold ...
    assert counts.tolist() == [1, 0, 1, 0]                          # ... so exactly one anchor is positive, through forcing only
    assert int(np.flatnonzero(target >= 0)[0]) == int(I[:, 0].argmax()) and (np.delete(target, I[:, 0].argmax()) == -1).all()


def test_off_grid_and_void_labels():
    cfg, anc, anchor = _small()
    A = pkg("assign")
    good = anchor(0, 37)
    base = A.anchor_targets(anc, good[None], POS, NEG)
    far = _row(500.0, 3.0, 4.0, 2.0, 0.2)
    t, best, counts = A.anchor_targets(anc, np.stack([far, good]), POS, NEG)
    assert np.array_equal(t >= 0, base[0] >= 0) and (t[t >= 0] == 1).all() and np.array_equal(best, base[1]) and counts.tolist() == base[2].tolist()
    voids = [_row(np.nan, 0.0, 4.0, 2.0, 0.0), _row(5.0, 0.0, 0.0, 2.0, 0.0), _row(5.0, 0.0, 4.0, -1.0, 0.0), _row(5.0, 0.0, 4.0, 2.0, np.inf)]
    assert A.void_labels(np.stack(voids + [good])).tolist() == [True] * 4 + [False]
    t, best, counts = A.anchor_targets(anc, np.stack(voids + [good]), POS, NEG)
    assert np.array_equal(t >= 0, base[0] >= 0) and (t[t >= 0] == 4).all() and np.array_equal(best, base[1])
    assert counts.tolist() == base[2].tolist()[:3] + [4]
    t, best, counts = A.anchor_targets(anc, np.stack(voids), POS, NEG)          # void labels only: everything negative
    assert (t == -1).all() and not best.any() and counts.tolist() == [0, 0, 0, 4]
    t, best, counts = A.anchor_targets(anc, np.zeros((0, 9), np.float32), POS, NEG)
    assert (t == -1).all() and not best.any() and counts.tolist() == [0, 0, 0, 0]


def test_exact_ties_go_to_the_lower_label_and_the_lower_anchor():
    cfg, anc, anchor = _small()
    A = pkg("assign")
    # two identical label rows: the lower k wins in arg (threshold positives) and in forcing
    lab = _row(anc[0, 0, 61] + 0.05, anc[0, 1, 61] + 0.04, 4.1, 1.9, 0.03)
    t, best, counts = A.anchor_targets(anc, np.stack([_row(2.0, -1.0, 4.0, 2.0, 0.8), lab, lab]), POS, NEG)
    I = A.anchor_iou(anc, np.stack([lab, lab]))
    assert np.array_equal(I[:, 0], I[:, 1]) and (best >= POS).sum() >= 1
    assert set(t[t >= 0].tolist()) == {0, 1} and t[int(I[:, 0].argmax())] == 1
    # one anchor duplicated (cell 20 made a copy of cell 21), the label on top of it: the lower j is forced, the copy is a threshold positive
    dup = anc.copy()
    dup[:, :, 20] = dup[:, :, 21]
    lab = _row(dup[0, 0, 21] + 0.3, dup[0, 1, 21] + 0.2, 4.4, 1.7, 0.1)[None]
    I = A.anchor_iou(dup, lab)
    assert I[20, 0] == I[21, 0] == I.max()
    t, best, counts, forced = A.targets_from_iou(I, A.void_labels(lab), 0.99, NEG)
    assert forced.tolist() == [20] and t[20] == 0 and t[21] == -2 and counts[2] == 1


# name -> (sample, label rows taken): the unpruned statement clips EVERY pair in Python, so the larger maps take a few rows -- among them
# the off-grid and the void row of sample SPECIAL
PRUNE_CASES = {"16x8": [(0, 3), (1, 0), (SPECIAL, 4)], "37x29": [(0, 2), (SPECIAL, 3)], "96x80": [(0, 1), (SPECIAL, 2)]}


@pytest.mark.parametrize("name", list(PRUNE_CASES))
def test_pruning_changes_nothing(name):
    """prune=True against prune=False: target and counts equal, best bit for bit."""
    cfg, boxes, nb, H, W = case(name)
    A = pkg("assign")
    anc = anchors_of(cfg)
    for b, n in PRUNE_CASES[name]:
        rows = boxes[b, :n].numpy()
        got, want = A.anchor_targets(anc, rows, POS, NEG), A.anchor_targets(anc, rows, POS, NEG, prune=False)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
        assert n == 0 or got[1].max() > 0 or b == SPECIAL
        if n == min(int(nb[b]), boxes.shape[1]):
            ref = assigned(name)[0][b]
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])


def test_the_committed_cases_meet_their_input_conditions():
    """What tests/test_gpu_loss_anchor.py asserts before it compares decisions, checked here as well: margins, yaw gap, and that the
    three kinds of anchor (threshold positive, ignored, positive through forcing only) all occur."""
    kinds = np.zeros(3, np.int64)
    for name in MAPS:
        cfg, boxes, nb, H, W = case(name)
        anc = anchors_of(cfg)
        for b in range(B):
            n = min(int(nb[b]), boxes.shape[1])
            rows = boxes[b, :n].numpy()
            m, n_thr, n_ign, n_forced, n_labels = margins(anc, rows, POS, NEG)
            print(name, b, n, "margin %.3g" % m, n_thr, n_ign, n_forced, n_labels)
            assert m >= MARGIN and yaw_condition(cfg, rows)
            if n:
                assert n_thr > 0 and n_ign > 0
            kinds += (n_thr, n_ign, n_forced)
    assert (kinds > 0).all()
    counts = assigned("96x80")[0][SPECIAL][2]
    assert counts[3] == 1                                            # the void row; the off-grid row forces nothing:
    assert 0 not in set(assigned("96x80")[0][SPECIAL][0].tolist())


def _torch_terms(cls, reg, anc, boxes, target, alpha, gamma, eps):
    """The definitions 6 and 7 written with torch ops in float64, anchor by anchor (no clamp: for p_t > eps)."""
    HW = cls.shape[1]
    n_pos = max(1, int((target >= 0).sum()))
    lc = torch.zeros((), dtype=torch.float64)
    lr = torch.zeros((), dtype=torch.float64)
    for j in np.flatnonzero(target != -2).tolist():
        a, i = divmod(j, HW)
        y = target[j] >= 0
        p = cls[2 * a + int(y), i]
        lc = lc - (alpha if y else 1.0 - alpha) * (1.0 - p) ** gamma * torch.log(p)
        if y:
            an, bx = torch.from_numpy(anc[a, :, i]).double(), torch.from_numpy(boxes[target[j], :7]).double()
            diag = torch.sqrt(an[3] ** 2 + an[4] ** 2)
            d = bx[6] - an[6]
            enc = torch.stack(((bx[0] - an[0]) / diag, (bx[1] - an[1]) / diag, (bx[2] - an[2]) / an[5], torch.log(bx[3] / an[3]),
                               torch.log(bx[4] / an[4]), torch.log(bx[5] / an[5]), torch.atan2(torch.sin(d), torch.cos(d))))
            lr = lr + torch.nn.functional.smooth_l1_loss(reg[7 * a:7 * a + 7, i], enc, reduction="sum")
    return lc / n_pos, lr / (7 * n_pos)


@pytest.mark.parametrize("alpha, gamma", [(0.25, 2.0), (0.5, 1.0)])
def test_anchor_terms_equal_a_literal_restatement(alpha, gamma):
    cfg, boxes, nb, H, W = case("16x8")
    (target, _, counts), anc = assigned("16x8")[0][0], anchors_of(cfg)
    assert counts[0] > 0 and counts[1] > 0
    rows = boxes[0, :int(nb[0])].numpy()
    cls = scores("uniform", H, W)[0].reshape(4, H * W).double().requires_grad_(True)
    reg = (regression_input(H, W)[0].reshape(14, H * W).double() * 4).requires_grad_(True)        # |d| on both sides of 1
    lc, lr, n_pos, gc, gr = pkg("loss").anchor_terms(cls.detach().numpy(), reg.detach().numpy(), anc, rows, target, alpha, gamma, 1e-12)
    wc, wr = _torch_terms(cls, reg, anc, rows, target, alpha, gamma, 1e-12)
    assert n_pos == counts[0] and abs(lc - wc.item()) <= 1e-12 * abs(lc) and abs(lr - wr.item()) <= 1e-12 * abs(lr) and lr > 0
    (wgc,) = torch.autograd.grad(wc, cls)
    (wgr,) = torch.autograd.grad(wr, reg)
    assert np.allclose(gc, wgc.numpy(), rtol=1e-12, atol=0) and np.allclose(gr, wgr.numpy(), rtol=1e-12, atol=0)
    ign = (target == -2).reshape(2, H * W)
    for a in range(2):                                               # an ignored anchor: no gradient on either channel, none on its offsets
        assert not gc[2 * a:2 * a + 2][:, ign[a]].any() and not gr[7 * a:7 * a + 7][:, ign[a]].any()
        assert not gr[7 * a:7 * a + 7][:, (target < 0).reshape(2, H * W)[a]].any()


def test_anchor_terms_without_positives_and_with_a_nan_score():
    cfg, boxes, nb, H, W = case("16x8")
    anc = anchors_of(cfg)
    HW = H * W
    cls, reg = scores("uniform", H, W)[0].reshape(4, HW).numpy(), regression_input(H, W)[0].reshape(14, HW).numpy()
    target = np.full(2 * HW, -1)
    target[:7] = -2
    lc, lr, n_pos, gc, gr = pkg("loss").anchor_terms(cls, reg, anc, np.zeros((0, 9), np.float32), target, 0.25, 2.0, 1e-12)
    want = sum((-0.75 * (1 - cls[2 * a].astype(np.float64)) ** 2 * np.log(cls[2 * a].astype(np.float64)))[7 if a == 0 else 0:].sum() for a in range(2))
    assert n_pos == 0 and lr == 0 and not gr.any() and abs(lc - want) <= 1e-12 * want            # N_b = 0: cls_b over 1
    bad = cls.copy()
    bad[2, 11] = np.nan
    lc, lr, n_pos, gc, gr = pkg("loss").anchor_terms(bad, reg, anc, np.zeros((0, 9), np.float32), target, 0.25, 2.0, 1e-12)
    assert np.isnan(lc) and np.isnan(gc[2, 11]) and int(np.isnan(gc).sum()) == 1


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_loss_total_on_cpu_tensors_equals_the_statement(reduction):
    cfg, boxes, nb, H, W = case("37x29", loss_reduction=reduction)
    targets, anc = assigned("37x29")
    cls, reg = scores("softmax", H, W), regression_input(H, W)
    want = terms_statement(cfg, anc, boxes, nb, [t for t, _, _ in targets], cls, reg, H, W)
    L = pkg("loss").LossTotal(cfg)
    L.keep_samples = True
    c1, r1 = cls.clone().requires_grad_(True), reg.clone().requires_grad_(True)
    loss = L(boxes, nb, c1, r1)
    loss.backward()
    assert abs(loss.item() - want[0]) <= 2e-6 * max(1.0, abs(want[0])) and L.calls == 0
    assert np.allclose(c1.grad.double().numpy(), want[1], rtol=1e-6, atol=1e-9) and np.allclose(r1.grad.double().numpy(), want[2], rtol=1e-6, atol=1e-9)
    assert np.allclose(L.last_terms.double().numpy(), want[3], rtol=1e-6, atol=0)
    t, best, counts = L.last_samples
    for b in range(B):
        assert np.array_equal(t[b].reshape(-1).numpy(), targets[b][0]) and np.array_equal(counts[b].numpy(), targets[b][2])
        assert np.array_equal(best[b].reshape(-1).numpy(), targets[b][1])
    if reduction == "last":
        assert not c1.grad[:B - 1].any() and not r1.grad[:B - 1].any() and not L.last_terms[:B - 1].any()


@pytest.mark.parametrize("key, value", [("assign_pos_iou", 1.5), ("assign_pos_iou", 0.3), ("assign_neg_iou", 0.0), ("assign_neg_iou", -0.1),
                                        ("assign_neg_iou", 0.7), ("assign_pos_iou", float("nan")), ("assign_neg_iou", float("inf")),
                                        ("assign_pos_iou", "0.6"), ("assign_neg_iou", True), ("focal_alpha", 1.0), ("focal_gamma", 0.5)])
def test_bad_keys_raise(key, value):
    with pytest.raises(ValueError):
        pkg("loss").LossTotal(config(16, 8, **{key: value}))


def test_defaults_and_accepted_edges():
    L = pkg("loss").LossTotal(config(16, 8))
    assert L.sampling == "anchor" and L.assign_iou == (0.6, 0.45) and L.focal == (0.25, 2.0, 1e-12) and L.calls == 0
    assert pkg("loss").LossTotal(config(16, 8, assign_pos_iou=1, assign_neg_iou=1.0)).assign_iou == (1.0, 1.0)
    cfg = config(16, 8)
    cfg["anchor_bbox_feature"] = dict(cfg["anchor_bbox_feature"], width=0.0)
    with pytest.raises(ValueError):
        pkg("loss").LossTotal(cfg)
    assert pkg("loss").LossTotal(dict(cfg, loss_sampling="focal")).sampling == "focal"          # only the anchor mode needs the area
    assert abs(float(np.diff(anchors_of(config(16, 8))[0, 0, ::8]).mean()) - PITCH) < 1e-6

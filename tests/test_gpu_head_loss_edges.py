"""The end of the network at its edges: the four loss entries of csrc/loss.hip and the two head kernels of csrc/elementwise.hip
against float64 statements (oracle/loss_ref.py::loss_from_lists, pinned to the reference's golden numbers in the CPU suite; the
head restated here from oracle/model_ref.py) -- on a grid larger than one trip of the workgroup, with saturated scores, residuals
on both sides of the Smooth-L1 knee, heading differences that wrap, clipped and overlapping windows, an empty sample, cells that
occur three times, lists longer than the LDS copy of the deterministic kernel and the capacity boundary of the device sampler.

Every share the inputs are built for is asserted on the statement's float64 values, so another seed cannot quietly turn an edge
case back into a benign one.  Bounds: the project's own for fp32 loss kernels (loss 2e-6 * max(1, |loss|); gradients rtol 1e-5,
atol 1e-7: tests/test_gpu_model.py, tests/test_gpu_loss_sampling.py), here against float64; fp32 arithmetic on the same terms
stays two orders of magnitude inside them."""
import functools
import math

import numpy as np
import pytest
import torch

from _loss_util import assign_lists, flat_lists
from _util import M64, from_dev, golden_cfg, load_golden, pkg, q, rnd, to_dev
from oracle import loss_ref, model_ref
from test_gpu_loss_sampling import _setup, sampler_statement

pytestmark = pytest.mark.gpu
TOL = {0: 1e-5, 1: 1e-2, 2: 2e-3}        # tests/test_gpu_elementwise.py
H, W, B = 64, 48, 3
NBOX = (20, 7, 0)                         # the empty sample: no positives, no regression rows
LIST_SEED = 3


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _cfg():
    return _setup(0)[0]                   # 256 x 192 voxels over 25.6 m x 19.2 m, stride 4: a 64 x 48 map of 0.4 m cells


@functools.lru_cache(maxsize=None)
def _scores():
    """cls: uniform in +-30 with about 2 % at +-90 (the soft-max saturates: exp(-180) is 0 in fp32); reg: uniform in +-3."""
    g = torch.Generator().manual_seed(5)
    cls = (torch.rand(B, 4, H, W, generator=g) * 2 - 1) * 30
    u = torch.rand(B, 4, H, W, generator=g)
    cls = torch.where(u < 0.01, torch.full_like(cls, 90.0), cls)
    cls = torch.where(u > 0.99, torch.full_like(cls, -90.0), cls)
    reg = (torch.rand(B, 14, H, W, generator=g) * 2 - 1) * 3
    return cls, reg


def _rand_boxes(g, n, max_box):
    """n boxes anywhere on the map: yaw in +-6, l / w / h in 0.5 .. 8."""
    bx = torch.zeros(max_box, 9)
    u = torch.rand(n, 7, generator=g)
    bx[:n, 0] = 1.0 + u[:, 0] * 23.0
    bx[:n, 1] = -9.0 + u[:, 1] * 18.0
    bx[:n, 2] = -2.0 + u[:, 2] * 2.0
    bx[:n, 3:6] = 0.5 + u[:, 3:6] * 7.5
    bx[:n, 6] = (u[:, 6] * 2 - 1) * 6.0
    bx[:n, 7], bx[:n, 8] = 6, 1
    return bx


@functools.lru_cache(maxsize=None)
def _boxes():
    g = torch.Generator().manual_seed(5)
    boxes = torch.stack([_rand_boxes(g, n, _cfg()["max_num_bbox"]) for n in NBOX])
    for b in (0, 1):
        boxes[b, 1, 0], boxes[b, 1, 1] = 0.05, -9.55                                   # the grid corner: a clipped window
        boxes[b, 3, 0], boxes[b, 3, 1] = boxes[b, 2, 0] + 0.4, boxes[b, 2, 1]          # 0.4 m (one cell) from box 2: overlapping windows
    return boxes, torch.tensor(NBOX)


def _repeats(cells):
    """Number of distinct cells that occur more than once in a list."""
    _, n = np.unique(np.asarray(cells, dtype=np.int64), return_counts=True)
    return int((n > 1).sum())


def _check_terms(terms, what):
    """The conditions the inputs are built for, on the statement's float64 values."""
    d, dyaw = terms["d"].abs(), terms["dyaw"]
    lin = float((d >= 1.0).double().mean())
    wrapped = float(((dyaw > math.pi) | (dyaw <= -math.pi)).double().mean())
    margin = float((dyaw.abs() - math.pi).abs().min())
    print("%s: %d Smooth-L1 entries, %.1f %% linear; %d heading differences, %.1f %% wrapped, margin to +-pi %.4f"
          % (what, d.numel(), 100 * lin, dyaw.numel(), 100 * wrapped, margin))
    assert 0.2 <= lin <= 0.8, "both Smooth-L1 branches: %.3f linear" % lin
    assert wrapped >= 0.2, "wrapped heading differences: %.3f" % wrapped
    assert margin >= 1e-3, "a heading difference %.2e from +-pi: fp32 may wrap it the other way" % margin


def _check(what, loss, gcls, greg, want):
    """loss within 2e-6 * max(1, |loss|), gradients within rtol 1e-5 / atol 1e-7 of the float64 statement; figures printed first."""
    wl, wc, wr = want[:3]
    gc, gr = gcls.detach().cpu().double(), greg.detach().cpu().double()
    el = abs(float(loss) - wl.item())
    ec = (gc - wc).abs() - 1e-5 * wc.abs()
    er = (gr - wr).abs() - 1e-5 * wr.abs()
    print("%s: loss %.9g (want %.9g, off %.3g, bound %.3g); cls grad off %.3g of max %.3g; reg grad off %.3g of max %.3g"
          % (what, float(loss), wl.item(), el, 2e-6 * max(1.0, abs(wl.item())), float((gc - wc).abs().max()), float(wc.abs().max()),
             float((gr - wr).abs().max()), float(wr.abs().max())))
    assert float(wc.abs().max()) > 1e-4                              # one missing list entry would move a gradient by about that much
    assert el <= 2e-6 * max(1.0, abs(wl.item())), what
    assert float(ec.max()) <= 1e-7, "%s: cls gradient" % what
    assert float(er.max()) <= 1e-7, "%s: reg gradient" % what


def _assign_lists(cfg, boxes, nb, pos_neg=None):
    """Per sample the five lists of oracle/loss_ref.py::loss_from_lists from LossTotal.assign (host side, numpy's generator as it
    stands); pos_neg: take the positive and negative cells from there instead (the device sampler's).  Weights as fp32, the way
    the kernels hold them."""
    return assign_lists(pkg("loss").LossTotal(dict(cfg, loss_sampling="compat")), boxes, nb, H, W, pos_neg)[:2]


# ------------------------------------------------------------------------------------------------------------------ list kernel
@functools.lru_cache(maxsize=None)
def _list_statement(reduction):
    cfg = _cfg()
    cls, reg = _scores()
    boxes, nb = _boxes()
    np.random.seed(LIST_SEED)
    lists, bxs = _assign_lists(cfg, boxes, nb)
    anc = model_ref.anchors(cfg)
    out = loss_ref.loss_from_lists(cls, reg, anc, lists, bxs, cfg["regress_loss_gain"], reduction, return_terms=True)
    return out, lists


@pytest.mark.parametrize("form", ["separate", "base"])
@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_list_kernel_against_fp64_statement(reduction, form):
    """dcf_loss_fwd_bwd through LossTotal (compat mode, CUDA tensors): HW = 3072 cells (three trips of the 1024 threads over the
    regression entries), samples with 20, 7 and 0 boxes, lists from LossTotal.assign under the same numpy seed."""
    cfg = dict(_cfg(), loss_sampling="compat", loss_reduction=reduction)
    cls, reg = _scores()
    boxes, nb = _boxes()
    want, lists = _list_statement("mean" if reduction == "last" else reduction)
    _check_terms(want[3], "list kernel inputs")                      # ('last' is the empty sample: the shares come from the whole batch)
    for b in (0, 1):                                                 # several cells occur more than once per list
        assert _repeats(lists[b][0]) >= 2 and _repeats(lists[b][1]) >= 1 and _repeats(lists[b][2]) >= 10, [_repeats(v) for v in lists[b][:3]]
    assert len(lists[2][0]) == 0 and len(lists[2][2]) == 0 and len(lists[2][1]) == cfg["neg_sample_threshold"] + 1
    want = _list_statement(reduction)[0]
    L = pkg("loss").LossTotal(cfg).cuda()
    np.random.seed(LIST_SEED)
    if form == "separate":
        c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
        loss = L(boxes, nb, c1, r1)
        loss.backward()
        gc, gr = c1.grad, r1.grad
    else:
        base = torch.zeros(B, 32, H, W)
        base[:, 0:4], base[:, 4:18] = cls, reg
        base = base.cuda().requires_grad_(True)
        loss = L(boxes, nb, base[:, 0:4], base[:, 4:18])
        loss.backward()
        gc, gr = base.grad[:, 0:4], base.grad[:, 4:18]
        assert float(base.grad[:, 18:].abs().max()) == 0.0
    _check("%s %s" % (reduction, form), loss.item(), gc, gr, want)


# ------------------------------------------------------------------------------------------------------------------ hand-built lists
@functools.lru_cache(maxsize=None)
def _hand_lists():
    """Sample 0: 1500 + 700 classification entries and 2100 regression rows (more than the 2048 the deterministic kernel stages in
    LDS: it scans global memory instead); sample 1: short lists (the LDS copy), in the same launch; sample 2: negatives only.
    In samples 0 and 1 one cell is three times among the positives, one three times among the negatives, one in both lists, and
    one regression cell belongs to three boxes."""
    rs = np.random.RandomState(17)
    boxes, nb = _boxes()
    windows, _ = _assign_lists(_cfg(), boxes, nb)                    # the regression rows of the real windows, drawn from with replacement
    lists = []
    for b, (npos, nneg, nrow) in enumerate(((1500, 700, 2100), (40, 30, 50), (0, 5, 0))):
        pos, neg = rs.randint(0, H * W, npos), rs.randint(0, H * W, nneg)
        pick = rs.randint(0, max(len(windows[b][2]), 1), nrow)
        rows, row_box = np.asarray(windows[b][2], dtype=np.int64)[pick], np.asarray(windows[b][3], dtype=np.int64)[pick]
        if npos:
            a, c, d, e = 1000 + b, 2000 + b, 2500 + b, H * W - 1 - b      # planted cells (H * W - 1: the last cell of the map)
            pos, neg = np.where(np.isin(pos, (a, c, d)), 7, pos), np.where(np.isin(neg, (a, c, d)), 8, neg)
            pos[[0, npos // 2, npos - 1]] = a                             # three times among the positives
            neg[[1, nneg // 2, nneg - 1]] = c                             # three times among the negatives
            pos[3], neg[4] = d, d                                         # once in each list
            rows[[2, nrow // 2, nrow - 1]] = e                            # one regression cell, three boxes
            row_box[[2, nrow // 2, nrow - 1]] = [0, 1, 2]
            assert (pos == a).sum() == 3 and (neg == c).sum() == 3 and (pos == d).sum() == 1 and (neg == d).sum() == 1
        per_box = np.bincount(row_box, minlength=1)
        row_w = (1.0 / (per_box[row_box] * 14)).astype(np.float32)       # the per-box mean
        lists.append((pos.tolist(), neg.tolist(), rows.tolist(), row_box.tolist(), row_w))
    assert len(lists[0][0]) + len(lists[0][1]) > 2048 and len(lists[0][2]) > 2048
    cfg = _cfg()
    cls, reg = _scores()
    bxs = [boxes[b, :int(nb[b]), :7].numpy() for b in range(B)]
    want = loss_ref.loss_from_lists(cls, reg, model_ref.anchors(cfg), lists, bxs, cfg["regress_loss_gain"], "mean", return_terms=True)
    return lists, want


@pytest.mark.parametrize("deterministic", [False, True])
def test_hand_built_lists_long_and_repeated(deterministic):
    """dcf_loss_fwd_bwd / dcf_loss_fwd_bwd_det through LossTotal._forward_hip with explicit lists: the global-scan fallback of the
    deterministic kernel (lists longer than its LDS copy) and its LDS path in one launch, cells occurring three times."""
    lists, want = _hand_lists()
    _check_terms(want[3], "hand-built lists")
    cfg = dict(_cfg(), loss_sampling="compat", loss_reduction="mean", deterministic=deterministic)
    cls, reg = _scores()
    boxes, nb = _boxes()
    L = pkg("loss").LossTotal(cfg).cuda()
    assert L.deterministic == deterministic
    ints, floats, plan = flat_lists(lists, [boxes[b, :int(nb[b]), :7].numpy() for b in range(B)])
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    loss = L._forward_hip(c1, r1, L.anchor_set.reshape(2, 7, H * W), ints, floats, plan, B, H, W)
    loss.backward()
    _check("hand-built, deterministic %s" % deterministic, loss.item(), c1.grad, r1.grad, want)


# ------------------------------------------------------------------------------------------------------------------ sampled kernel
_SAMPLED = {}


def _sampled_case(cfg, boxes, nb, key):
    """Run dcf_loss_sample_fwd_bwd(_det) with keep_samples; the statement is fed the lists the kernel returns plus assign's
    regression rows, computed once per (inputs, regress_type, reduction) and shared by the deterministic twin (same seed: it
    must draw the same lists)."""
    cls, reg = _scores()
    L = pkg("loss").LossTotal(cfg).cuda()
    L.keep_samples = True
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    loss = L(boxes, nb, c1, r1)
    loss.backward()
    pos, neg, counts = [t.cpu().numpy() for t in L.last_samples]
    pos_neg = [([int(v) for v in pos[b] if v >= 0], [int(v) for v in neg[b]]) for b in range(B)]
    for b in range(B):
        assert int(counts[b, 0]) == len(pos_neg[b][0]) and list(pos[b][:len(pos_neg[b][0])]) == pos_neg[b][0]
    if key not in _SAMPLED:
        lists, bxs = _assign_lists(cfg, boxes, nb, pos_neg)
        want = loss_ref.loss_from_lists(cls, reg, model_ref.anchors(cfg), lists, bxs, cfg["regress_loss_gain"], cfg["loss_reduction"],
                                        return_terms=True)
        _SAMPLED[key] = (pos_neg, want)
    assert _SAMPLED[key][0] == pos_neg
    return L, loss, c1.grad, r1.grad, pos_neg, counts, _SAMPLED[key][1]


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("reduction", ["last", "mean"])
@pytest.mark.parametrize("regress_type", [0, 1])
def test_sampled_kernel_against_fp64_statement(regress_type, reduction, deterministic):
    cfg = dict(_cfg(), loss_sampling="device", loss_seed=77, regress_type=regress_type, loss_reduction=reduction, deterministic=deterministic)
    boxes, nb = _boxes()
    if reduction == "last":                       # the sample that counts must not be the empty one
        boxes, nb = boxes.flip(0).contiguous(), nb.flip(0).contiguous()
    L, loss, gc, gr, pos_neg, counts, want = _sampled_case(cfg, boxes, nb, ("edges", regress_type, reduction))
    if regress_type == 0:                         # (centre rows only: 14 residuals per box, the shares are those of regress_type 0)
        _check_terms(want[3], "sampled kernel inputs")
    assert int(counts[:, 1].max()) > cfg["pos_sample_threshold"] and int(counts[:, 1].min()) == 0
    _check("sampled regress_type %d %s deterministic %s" % (regress_type, reduction, deterministic), loss.item(), gc, gr, want)


def _capacity_boxes():
    """64 boxes per sample on an 8 x 8 lattice of cells, whole 4 x 4 windows: 64 * 16 = 1024 entries, the kernel's capacity.
    Sample 1 has one box in the grid corner instead (a clipped window: 1012 entries); sample 2 has one box moved one cell
    (0.4 m) from its neighbour (overlapping windows)."""
    g = torch.Generator().manual_seed(10)
    boxes = torch.stack([_rand_boxes(g, 64, 64) for _ in range(B)])
    for b in range(B):
        for k in range(64):
            cx, cy = 4 + 7 * (k // 8), 3 + 6 * (k % 8)                       # window cx-2 .. cx+1, cy-2 .. cy+1: inside 64 x 48
            boxes[b, k, 0], boxes[b, k, 1] = (cx + 0.5) * 0.4, -9.6 + (cy + 0.5) * 0.4
    boxes[1, 5, 0], boxes[1, 5, 1] = 0.05, -9.55
    boxes[2, 9, 0], boxes[2, 9, 1] = boxes[2, 8, 0] + 0.4, boxes[2, 8, 1]
    return boxes, torch.tensor([64, 64, 64])


@pytest.mark.parametrize("deterministic", [False, True])
def test_sampled_kernel_at_capacity(deterministic):
    """max_num_bbox 64, positive_range 4 (an even span: the window is cx-2 .. cx+1): 64 * 4 * 4 = 1024 = LS_MAXE window entries,
    the subset branch picks 128 of them.  Lists bit for bit the Python restatement of the sampler; loss and gradients against
    the float64 statement."""
    cfg = dict(_cfg(), loss_sampling="device", loss_seed=77, max_num_bbox=64, positive_range=4, loss_reduction="mean", deterministic=deterministic)
    boxes, nb = _capacity_boxes()
    L, loss, gc, gr, pos_neg, counts, want = _sampled_case(cfg, boxes, nb, ("capacity", 0, "mean"))
    cap = cfg["pos_sample_threshold"]
    assert (counts[:, 1] > cap).all() and (counts[:, 0] == cap).all()
    assert int(counts[0, 1]) == 1024 and int(counts[1, 1]) == 1024 - 12 and int(counts[2, 1]) == 1024
    seed = (cfg["loss_seed"] * 0x9E3779B1 + 0) & M64
    for b in range(B):
        want_pos, want_neg, n_entries = sampler_statement(L, boxes[b].numpy(), 64, H, W, seed, b)
        assert pos_neg[b][0] == want_pos and pos_neg[b][1] == want_neg and n_entries == int(counts[b, 1])
    _check_terms(want[3], "capacity inputs")
    _check("capacity, deterministic %s" % deterministic, loss.item(), gc, gr, want)


def test_sampled_kernel_over_capacity_raises_without_launching():
    """max_num_bbox 64 with positive_range 5 is 1600 window entries, more than the kernel holds: an error, and nothing written."""
    Hm = pkg("_hip")
    cfg = dict(_cfg(), loss_sampling="device", loss_seed=77, max_num_bbox=64, positive_range=5, loss_reduction="mean")
    boxes, nb = _capacity_boxes()
    cls, reg = _scores()
    L = pkg("loss").LossTotal(cfg).cuda()
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    with pytest.raises(Hm.DcfError):
        L(boxes, nb, c1, r1)
    # the C entries themselves, on buffers holding a sentinel: they come back untouched
    anc = L.anchor_set.cuda().reshape(2, 7, H * W)
    cap, nneg = cfg["pos_sample_threshold"], cfg["neg_sample_threshold"] + 1
    for det in (False, True):
        loss = torch.full((1,), -7.0, device="cuda")
        gc, gr = torch.full_like(c1, -7.0), torch.full_like(r1, -7.0)
        outs = [torch.full((B, cap), -7, dtype=torch.int32, device="cuda"), torch.full((B, nneg), -7, dtype=torch.int32, device="cuda"),
                torch.full((B, 2), -7, dtype=torch.int32, device="cuda")]
        args = (c1.detach(), c1.stride(0), r1.detach(), r1.stride(0), anc, boxes.cuda(), nb.to(torch.int32).cuda(), 64, 9, B, H, W,
                float(L._xs), float(L._xo), float(L._ys), float(L._yo), 4.0, 5, 0, cap, nneg, 12345, 3.0, 2, loss, gc, gc.stride(0),
                gr, gr.stride(0), outs[0], outs[1], outs[2])
        with pytest.raises(Hm.DcfError):
            if det:
                Hm.call("dcf_loss_sample_fwd_bwd_det", *(args + (torch.empty(B, device="cuda"), Hm.stream_ptr())))
            else:
                Hm.call("dcf_loss_sample_fwd_bwd", *(args + (Hm.stream_ptr(),)))
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in [loss, gc, gr] + outs)


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_B, HEAD_H, HEAD_W = 3, 17, 15        # 765 pixels: three workgroups of 256, the last one ragged; b = p / hw splits inside a workgroup
GROUPS_FWD = {"probabilities": [0, 1, 2, 3], "box x/y/z": [18, 19, 20, 25, 26, 27], "box l/w/h": [21, 22, 23, 28, 29, 30], "heading": [24, 31]}
GROUPS_BWD = {"logits": [0, 1, 2, 3], "x/y/z offsets": [4, 5, 6, 11, 12, 13], "l/w/h offsets": [7, 8, 9, 14, 15, 16], "heading offsets": [10, 17]}


@functools.lru_cache(maxsize=None)
def _head_anchors():
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    anc = model_ref.anchors(dict(cfg, voxel_length=4 * HEAD_H, voxel_width=4 * HEAD_W))
    assert tuple(anc.shape) == (14, HEAD_H, HEAD_W) and anc.dtype == torch.float32
    return anc


@functools.lru_cache(maxsize=None)
def _head_case(dtype, Cp):
    """(head quantised to the storage type, upstream gradient, float64 forward, float64 gradient of the first 18 channels)."""
    anc = _head_anchors()
    shape = (HEAD_B, 1, HEAD_H, HEAD_W)
    head = rnd((HEAD_B, Cp, HEAD_H, HEAD_W), 60 + Cp)                         # channels >= 18: padding the kernels must ignore
    head[:, 0:4] = rnd((HEAD_B, 4, HEAD_H, HEAD_W), 61, -30.0, 30.0)
    u = rnd((HEAD_B, 4, HEAD_H, HEAD_W), 62, 0.0, 1.0)
    head[:, 0:4] = torch.where(u < 0.01, torch.full_like(u, 60.0), torch.where(u > 0.99, torch.full_like(u, -60.0), head[:, 0:4]))
    for a in range(2):
        head[:, 4 + 7 * a:7 + 7 * a] = rnd((HEAD_B, 3, HEAD_H, HEAD_W), 63 + a, -1.5, 1.5)
        head[:, 7 + 7 * a:10 + 7 * a] = rnd((HEAD_B, 3, HEAD_H, HEAD_W), 65 + a, -4.0, 4.0)
        r6 = rnd(shape, 67 + a, -5.0, 5.0)
        yaw = anc[7 * a + 6].double()
        for _ in range(8):                 # keep r6 + anchor yaw, as stored, 5e-3 away from +-pi: there fp32 may wrap the other way
            near = ((q(r6, dtype).double() + yaw).abs() - math.pi).abs() < 5e-3
            r6 = torch.where(near, r6 + 0.0625, r6)
        head[:, 10 + 7 * a:11 + 7 * a] = r6
    head = q(head, dtype)
    hv = head[:, :18].double().requires_grad_(True)
    cls = torch.cat((torch.softmax(hv[:, 0:2], 1), torch.softmax(hv[:, 2:4], 1)), 1)
    reg = hv[:, 4:18]
    ref = torch.cat((cls, reg, model_ref.decode(reg, anc.double())), 1)
    R = rnd((HEAD_B, 32, HEAD_H, HEAD_W), 70)
    ref.backward(R.double())
    t = torch.cat([head[:, 10 + 7 * a].double() + anc[7 * a + 6].double() for a in range(2)])
    wrapped = float(((t > math.pi) | (t <= -math.pi)).double().mean())
    margin = float((t.abs() - math.pi).abs().min())
    print("head dtype %d Cp %d: %.1f %% of r6 + yaw wrapped, margin to +-pi %.4f" % (dtype, Cp, 100 * wrapped, margin))
    assert wrapped >= 0.2 and margin >= 1e-3
    assert bool(((hv[:, 0] - hv[:, 1]).abs() > 60).any())                     # saturated pairs: 1 - exp(-60) is 1 in fp32
    return head, R, ref.detach(), hv.grad


@pytest.mark.parametrize("Cp", [20, 32, 36])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_head_against_fp64_statement(dtype, Cp):
    """dcf_head_fwd / dcf_head_bwd against softmax pairs + model_ref.decode + concat in float64 (backward: autograd), inputs
    quantised to the storage type first; every channel group normalised by ITS OWN maximum (a probability cannot hide behind a
    box coordinate of 25).  Forward 1e-5 per group (fp32 arithmetic on identical inputs), the raw offsets equal; backward
    TOL[dtype] per group (the gradient is stored in the compute type)."""
    ops, Hm = pkg("ops"), pkg("_hip")
    head, R, ref, ghv = _head_case(dtype, Cp)
    anc = _head_anchors().cuda()
    hd = to_dev(head, dtype)
    pred = ops.head_fwd(dtype, hd, anc)
    got = pred.cpu().double()
    assert torch.equal(pred[:, 4:18].cpu(), head[:, 4:18])
    for name, ch in GROUPS_FWD.items():
        err = float((got[:, ch] - ref[:, ch]).abs().max() / ref[:, ch].abs().max())
        print("forward %s: %.3g" % (name, err))
        assert err < 1e-5, "forward %s: %g" % (name, err)
    assert float((got[:, 24].abs().max())) <= math.pi + 1e-6 and float(got[:, 0:4].min()) >= 0.0
    ghead = torch.full_like(hd, float("nan"))                                 # the C entry on a buffer full of NaN: every channel is written
    Hm.call("dcf_head_bwd", dtype, hd, Cp, anc, pred, R.cuda(), ghead, HEAD_B, HEAD_H, HEAD_W, Hm.stream_ptr())
    gh = from_dev(ghead)
    assert not bool(torch.isnan(gh).any())
    assert float(gh[:, 18:].abs().max()) == 0.0
    for name, ch in GROUPS_BWD.items():
        err = float((gh[:, ch].double() - ghv[:, ch]).abs().max() / ghv[:, ch].abs().max())
        print("backward %s: %.3g" % (name, err))
        assert err < TOL[dtype], "backward %s: %g" % (name, err)

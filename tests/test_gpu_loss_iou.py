"""The rotated-IoU regression term of `loss_sampling: anchor` (`iou_loss_gain`; csrc/loss_iou.hip k_loss_anchor_iou /
k_loss_anchor_iou_fold) against the float64 statement (loss.anchor_iou_terms on top of loss.anchor_terms; tests/_iou_loss_util.statement): loss,
gradients and both read-outs at the project's bounds for fp32 loss kernels (tests/_focal_util.close), the per-anchor fp64 IoU at 1e-12; the
entry alone on hand-written targets and pattern-filled buffers; the reductions; repeatability; a NaN offset; rejected arguments; the train step.

The device clips edges where the statement's value clips polygons, and its cos / sin may differ from libm's in the last bit, so before anything
is compared the inputs are shown -- from the statement -- to keep every pair 1e-6 m from a change of topology (tests/_iou_loss_util.margin): a
condition on the inputs, asserted."""
import numpy as np
import pytest
import torch

from _anchor_util import B, MAPS, SPECIAL, anchors_of, assigned
from _focal_util import close, regression_input
from _iou_loss_util import GAIN, KINDS, case_iou, close_iou, encoded, iou_statement, kinds_present, margin, pairs, regression, statement
from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu


def _run(cfg, boxes, nb, cls, reg, boxes_dev=False, L=None, keep=False):
    if L is None:
        L = pkg("loss").LossTotal(cfg).cuda()
    L.keep_samples = keep
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    loss = L(boxes.cuda() if boxes_dev else boxes, nb.cuda() if boxes_dev else nb, c1, r1)
    loss.backward()
    return L, loss, c1.grad, r1.grad, L.last_terms.clone(), None if L.last_iou is None else L.last_iou.clone()


def _input_conditions(name, kind):
    n = kinds_present(name)
    assert all(v > 0 for v in n.values()), n
    m = min(float(margin(p, q, kind).min()) for j, p, q in pairs(name) if len(j))
    print("%s %s: kinds %s, least margin %.3g m" % (name, kind, n, m))
    assert m >= 1e-6


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("kind", KINDS)
def test_iou_loss_equals_the_host_statement(name, kind):
    _input_conditions(name, kind)
    cfg, boxes, nb, H, W, cls, reg, want = statement(name, kind)
    L, loss, gc, gr, terms, iou = _run(cfg, boxes, nb, cls, reg, keep=True)
    print("loss %.9g want %.9g; iou terms %s want %s" % (loss.item(), want[0], iou.cpu().tolist(), want[4].tolist()))
    close(loss.item(), gc, gr, terms, want[:4])
    close_iou(iou, want[4])
    assert iou.dtype == torch.float32 and iou.is_cuda and L.calls == 0
    target, best, counts, iou_map = L.last_samples
    assert iou_map.shape == (B, 2, H * W) and iou_map.dtype == torch.float64
    err = np.abs(iou_map.cpu().numpy() - want[5]).max()
    print("max |per-anchor IoU - statement| %.3g" % err)
    assert err <= 1e-12
    assert torch.equal(counts[:, 0].float(), iou[:, 1]) and not iou_map[target < 0].any()
    # the same inputs with the term off: the classification gradient keeps its bits, the regression gradient moves at the positives only
    L0, loss0, gc0, gr0, terms0, iou0 = _run(dict(cfg, iou_loss_gain=0.0), boxes, nb, cls, reg, keep=True)
    assert iou0 is None and len(L0.last_samples) == 3 and torch.equal(gc0, gc) and torch.equal(terms0, terms)
    moved = (gr != gr0).reshape(B, 2, 7, H * W)
    assert moved.any() and not moved[(target < 0).reshape(B, 2, 1, H * W).expand(B, 2, 7, H * W)].any()
    assert loss.item() > loss0.item()


def _hand_case(kind):
    """37x29, reduction sum: one positive in sample 0 (anchor 1), none in sample 1, one in sample 2; a target beyond the label rows and one
    below -2 count as ignored.  The two positives regress their label within noise, so their gradients are not zero."""
    cfg, boxes, nb, H, W = case_iou("37x29", kind, loss_reduction="sum")
    HW = H * W
    anc = anchors_of(cfg)
    targets = np.full((B, 2 * HW), -1, dtype=np.int32)
    targets[:, ::7] = -2
    where = ((0, 1, 500, 3), (SPECIAL, 0, 17, 2))                    # (sample, anchor, cell, label row)
    for b, a, cell, k in where:
        targets[b, a * HW + cell] = k
    targets[2, 18], targets[2, 19] = 64, -3
    reg = regression_input(H, W).reshape(B, 14, HW).clone()
    g = np.random.default_rng(5)
    for b, a, cell, k in where:
        enc = encoded(anc[a][:, cell:cell + 1], boxes[b, k].numpy()[None])[:, 0]
        reg[b, 7 * a:7 * a + 7, cell] = torch.from_numpy(enc + 0.05 * g.standard_normal(7)).float()
    counts = np.zeros((B, 4), np.int32)
    counts[:, 0] = (1, 0, 1)
    return cfg, boxes, H, W, anc, targets, counts, reg.reshape(B, 14, H, W).contiguous(), where


@pytest.mark.parametrize("kind", KINDS)
def test_the_entry_alone_changes_the_positives_elements_only(kind):
    """ops.loss_anchor_iou on hand-written targets: greg starts as a pattern, loss as a number, the workspace and the read-outs as NaN.  Only
    the 7 x N elements of the positive anchors change, by the statement's gradient; loss grows by the statement's term; a sample without
    positives contributes an exact 0."""
    cfg, boxes, H, W, anc, targets, counts, reg, where = _hand_case(kind)
    HW = H * W
    ops, Lm = pkg("ops"), pkg("loss")
    nb_all = torch.tensor([boxes.shape[1]] * B)
    want_loss, want_g, want_terms, want_map = iou_statement(cfg, anc, boxes, nb_all, list(targets), reg, H, W)
    assert margin(*[np.concatenate(v) for v in zip(*[(p, q) for _, p, q in _hand_pairs(anc, boxes, targets, reg, HW)])], kind).min() >= 1e-6
    dev = torch.device("cuda")
    ws, iou_terms, iou_map = ops.loss_anchor_iou_workspace(B, H, W, dev, iou_map=True)
    ws.fill_(float("nan")); iou_terms.fill_(float("nan")); iou_map.fill_(float("nan"))
    pattern = (torch.arange(B * 14 * HW, dtype=torch.float32).reshape(B, 14, H, W) % 251.0 - 125.0) * 1e-3
    greg, loss = pattern.clone().to(dev), torch.full((1,), 0.25, device=dev)
    ops.loss_anchor_iou(reg.cuda(), torch.from_numpy(anc).cuda(), boxes.cuda(), torch.from_numpy(targets).cuda().reshape(B, 2, HW),
                        torch.from_numpy(counts).cuda(), Lm.IOU_KIND[kind], GAIN, Lm.REDUCTION["sum"], loss, greg, iou_terms, ws, iou_map=iou_map)
    got = greg.cpu()
    changed = (got != pattern).reshape(B, 2, 7, HW)
    mask = torch.zeros(B, 2, 7, HW, dtype=torch.bool)
    for b, a, cell, k in where:
        mask[b, a, :, cell] = True
    print("loss %.9g want %.9g; iou terms %s; changed %d" % (loss.item(), 0.25 + want_loss, iou_terms.cpu().tolist(), int(changed.sum())))
    assert torch.equal(got[~mask.reshape(got.shape)], pattern[~mask.reshape(got.shape)])            # every other element keeps its bits
    moving = torch.from_numpy(want_g != 0).reshape(B, 2, 7, HW)          # bird's-eye: z and h carry no gradient, so 5 of each 7 move
    assert int(moving.sum()) == (14 if kind == "3d" else 10) and torch.equal(changed, moving)
    delta = got.double().numpy() - pattern.double().numpy()
    inside = mask.reshape(got.shape).numpy()
    # the sum with the pattern is rounded to fp32 once more: half an ulp of 0.125 on top of the gradient bound
    assert (np.abs(delta - want_g)[inside] <= (1e-7 + 1e-5 * np.abs(want_g) + 2.0 ** -27)[inside]).all()
    assert abs(loss.item() - (0.25 + want_loss)) <= 2e-6 * max(1.0, abs(0.25 + want_loss))
    close_iou(iou_terms, want_terms)
    assert iou_terms[1].tolist() == [0.0, 0.0] and want_terms[:, 1].tolist() == [1, 0, 1]
    assert np.abs(iou_map.cpu().numpy() - want_map).max() <= 1e-12 and int((iou_map != 0).sum()) == 2


def _hand_pairs(anc, boxes, targets, reg, HW):
    Lm = pkg("loss")
    out = []
    for b in range(B):
        t = targets[b].astype(np.int64).copy()
        t[(t < 0) | (t >= boxes.shape[1])] = -1
        j = np.flatnonzero(t >= 0)
        a, cell = j // HW, j % HW
        r = reg[b].reshape(14, HW).double().numpy()
        p, _ = Lm.decode_offsets(np.stack([r[7 * a + c, cell] for c in range(7)]), anc[a, :, cell].T)
        out.append((j, p.T, boxes[b, t[j], :7].double().numpy()))
    return out


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_iou_reductions_and_labels_on_the_device(reduction):
    cfg, boxes, nb, H, W, cls, reg, want = statement("96x80", "3d", loss_reduction=reduction)
    L, loss, gc, gr, terms, iou = _run(cfg, boxes, nb, cls, reg)
    close(loss.item(), gc, gr, terms, want[:4])
    close_iou(iou, want[4])
    if reduction == "last":
        assert not gr[:B - 1].any() and not iou[:B - 1].any() and float(iou[B - 1, 1]) >= 1
    on_dev = _run(cfg, boxes, nb, cls, reg, boxes_dev=True, L=L)          # the same module again: its buffers are reused
    for a, b in zip(on_dev[1:], (loss, gc, gr, terms, iou)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("deterministic", [False, True])
def test_two_calls_are_bit_identical(deterministic):
    cfg, boxes, nb, H, W, cls, reg, want = statement("96x80", "3d", "softmax")
    runs = [_run(dict(cfg, deterministic=deterministic), boxes, nb, cls, reg) for _ in range(2)]
    for a, b in zip(runs[0][1:], runs[1][1:]):                   # loss, gcls, greg, terms, iou terms
        assert torch.equal(a, b)
    close(runs[0][1].item(), runs[0][2], runs[0][3], runs[0][4], want[:4])
    close_iou(runs[0][5], want[4])


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_offset_reaches_the_loss_and_its_own_anchor_only(kind):
    name = "96x80"
    cfg, boxes, nb, H, W, cls, reg, want = statement(name, kind)
    HW = H * W
    clean = _run(cfg, boxes, nb, cls, reg)
    target = assigned(name)[0][1][0]
    j = int(np.flatnonzero(target >= 0)[3])
    a, cell = divmod(j, HW)
    for ch in (0, 4, 6):                                          # a centre, a size and the yaw offset
        bad = reg.clone()
        bad.reshape(B, 14, HW)[1, 7 * a + ch, cell] = float("nan")
        L, loss, gc, gr, terms, iou = _run(cfg, boxes, nb, cls, bad)
        assert torch.isnan(loss).all() and torch.isnan(iou[1, 0]) and torch.isfinite(iou[[0, 2]]).all() and torch.equal(iou[:, 1], clean[5][:, 1])
        nan = torch.isnan(gr).reshape(B, 2, 7, HW)
        own = torch.zeros_like(nan)
        own[1, a, :, cell] = True
        assert bool(nan[own].all()) and not bool(nan[~own].any())
        assert torch.equal(gr.reshape(B, 2, 7, HW)[~own], clean[3].reshape(B, 2, 7, HW)[~own]) and torch.equal(gc, clean[2])


def test_rejected_arguments_launch_nothing():
    Hm, ops, Lm = pkg("_hip"), pkg("ops"), pkg("loss")
    cfg, boxes, nb, H, W = case_iou("16x8")
    dev = torch.device("cuda")
    HW = H * W
    anc = torch.from_numpy(anchors_of(cfg)).cuda()
    bx = boxes.cuda()
    lib = Hm.lib()
    assert lib.dcf_loss_anchor_iou_workspace_bytes(0, H, W) == 0 and lib.dcf_loss_anchor_iou_workspace_bytes(1, 1 << 15, 1 << 15) == 0
    assert lib.dcf_loss_anchor_iou_workspace_bytes(B, H, W) == B * 8 * 2 * -(-2 * HW // 2048)
    ws, iou_terms, iou_map = ops.loss_anchor_iou_workspace(B, H, W, dev, iou_map=True)
    ws.fill_(-77.0); iou_terms.fill_(-77.0); iou_map.fill_(-77.0)
    odd = torch.full((2 * iou_map.numel() + 2,), -77.0, device=dev)      # odd[1:]: 4 bytes off an 8-byte boundary, room for either buffer
    reg = regression("16x8").cuda()
    gr, loss = torch.full_like(reg, -77.0), torch.full((1,), -77.0, device=dev)
    tg = torch.from_numpy(np.stack([t for t, _, _ in assigned("16x8")[0]])).to(torch.int32).cuda().reshape(B, 2, HW)
    cn = torch.from_numpy(np.stack([c for _, _, c in assigned("16x8")[0]])).to(torch.int32).cuda()

    def call(r=reg, anchors=anc, labels=bx, max_box=boxes.shape[1], stride=9, t=tg, n=cn, Hh=H, Ww=W, kind=0, gain=2.0, red=1, out=loss, g=gr,
             tm=iou_terms, mp=iou_map, w=ws):
        return lib.dcf_loss_anchor_iou_fwd_bwd(*[Hm._ptr(v) for v in (r, 14 * HW, anchors, labels, max_box, stride, t, n, B, Hh, Ww, kind, gain, red, out,
                                                                       g, 14 * HW, tm, mp, w, Hm.stream_ptr())])

    for kw in (dict(max_box=0), dict(max_box=65), dict(stride=6), dict(Hh=1 << 15, Ww=1 << 15), dict(Hh=0), dict(kind=2), dict(kind=-1), dict(red=3),
               dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(r=None), dict(anchors=None), dict(labels=None), dict(t=None),
               dict(n=None), dict(out=None), dict(g=None), dict(tm=None), dict(w=None), dict(w=odd[1:]), dict(mp=odd[1:])):
        assert call(**kw) == -1 and lib.dcf_last_error().decode().startswith("dcf_loss_anchor_iou_fwd_bwd"), kw
    torch.cuda.synchronize()
    assert (gr == -77).all() and loss.item() == -77 and (iou_terms == -77).all() and (iou_map == -77).all() and (ws == -77).all() and (odd == -77).all()
    assert call() == 0 and call(mp=None) == 0                      # the same call with nothing wrong; the map is optional
    torch.cuda.synchronize()
    assert (iou_terms[:, 1] == cn[:, 0]).all() and not (gr == -77).all()


@pytest.mark.parametrize("over", [dict(deterministic=False, loss_scale="none"), dict(deterministic=True, loss_scale="dynamic", grad_accum_steps=2),
                                  dict(hip_graphs="auto", iou_loss_kind="bev")], ids=["plain", "guarded-accum", "graphs-bev"])
def test_train_step_with_the_iou_term(over):
    """Train.one_step with loss_sampling: anchor and the term on, on the tiny model: a finite loss, the read-out's shape and range, and the
    loss equal to the terms plus gain * (1 - mean IoU) when there is a positive anchor."""
    z = load_golden("model_tiny.npz")
    lz = load_golden("loss.npz")
    cfg = golden_cfg(z)
    iou_gain = 1.5
    cfg.update(dtype="f32", loss_sampling="anchor", iou_loss_gain=iou_gain, **over)
    T = pkg("train")
    det = pkg("detfill")
    u = det.uniform((1, 32, 64, 32), 4242, 0.0, 1.0)
    x = torch.from_numpy(u.astype(np.float32)).cuda()
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device="cuda")
    boxes, nbx = torch.from_numpy(lz["bboxes"])[:1], torch.from_numpy(lz["nbox"])[:1]
    gain = cfg["regress_loss_gain"]
    tr = T.Train(cfg)
    det.fill_state_dict(tr.model)
    start = tr.model.flat_params.clone()
    assert tr.loss_iou() is None                               # nothing computed yet
    for _ in range(2):
        tr.one_step(x, img, boxes, nbx)
        terms, iou = tr.loss_terms(), tr.loss_iou()
        assert iou.shape == (1, 2) and iou.is_cuda and iou.data_ptr() != tr.loss_total.last_iou.data_ptr()
        mean, n = float(iou[0, 0]), int(iou[0, 1])
        assert 0.0 <= mean <= 1.0 and n == int(terms[0, 2]) and n >= 1
        want = float(terms[-1, 0]) + gain * float(terms[-1, 1]) + iou_gain * (1.0 - mean)          # loss_reduction: last (the default)
        print("loss %.7g, terms + gain * (1 - mean IoU) %.7g; mean IoU %.4f over %d anchors" % (tr.loss_value.item(), want, mean, n))
        assert abs(tr.loss_value.item() - want) <= 1e-6 * max(1.0, abs(want))
    assert np.isfinite(tr.loss_value.item()) and not torch.equal(start, tr.model.flat_params)
    off = T.Train(dict(cfg, iou_loss_gain=0))
    assert off.loss_iou() is None and off.loss_total.last_iou is None

"""loss_sampling: anchor (IoU-based anchor assignment; csrc/loss.hip k_assign_* / k_loss_anchor / k_anchor_fold): the
device's targets and counts exactly, best to 1e-12 (the bound tests/test_gpu_eval_ranked.py uses for fp64 geometry), against the host
statement (assign.anchor_targets); loss, gradients and the terms read-out against the float64 statement (loss.anchor_terms) at the
project's bounds for fp32 loss kernels (tests/_focal_util.close); NaN propagation; hand-written targets; the reductions; repeatability;
rejected arguments; the train step.

The device's cos / sin may differ from libm's in the last bit, so before any decision is compared the inputs are shown -- from the host
statement -- to leave every decision a margin of 1e-9 (tests/_anchor_util.margins): a condition on the inputs, asserted."""
import numpy as np
import pytest
import torch

from _anchor_util import B, MAPS, MARGIN, SPECIAL, anchors_of, assigned, case, margins, statement, terms_statement, yaw_condition
from _focal_util import PATTERNS, close, regression_input, scores
from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(name, pattern, **over):
    """The float64 statement of one case, computed once."""
    key = (name, pattern, tuple(sorted(over.items())))
    if key not in _WANT:
        cfg, boxes, nb, H, W = case(name, **over)
        cls, reg = scores(pattern, H, W), regression_input(H, W)
        _WANT[key] = (cfg, boxes, nb, H, W, cls, reg, statement(name, cls, reg, **over))
    return _WANT[key]


def _run(cfg, boxes, nb, cls, reg, boxes_dev=False, L=None, keep=False):
    if L is None:
        L = pkg("loss").LossTotal(cfg).cuda()
    L.keep_samples = keep
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    loss = L(boxes.cuda() if boxes_dev else boxes, nb.cuda() if boxes_dev else nb, c1, r1)
    loss.backward()
    return L, loss, c1.grad, r1.grad, L.last_terms.clone()


def _input_conditions(name):
    cfg, boxes, nb, H, W = case(name)
    anc = anchors_of(cfg)
    pos_iou, neg_iou = pkg("assign").parse_assign_config(cfg)
    kinds = np.zeros(3, np.int64)
    for b in range(B):
        rows = boxes[b, :min(int(nb[b]), boxes.shape[1])].numpy()
        m, n_thr, n_ign, n_forced, _ = margins(anc, rows, pos_iou, neg_iou)
        print("%s sample %d: margin %.3g, threshold positives %d, ignored %d, forced only %d" % (name, b, m, n_thr, n_ign, n_forced))
        assert m >= MARGIN and yaw_condition(cfg, rows)
        kinds += (n_thr, n_ign, n_forced)
    assert (kinds > 0).all()                    # all three kinds of anchor occur on every map


@pytest.mark.parametrize("name", list(MAPS))
def test_assignment_equals_the_host_statement(name):
    _input_conditions(name)
    cfg, boxes, nb, H, W = case(name)
    want, anc = assigned(name)
    ops = pkg("ops")
    dev = torch.device("cuda")
    pos_iou, neg_iou = pkg("assign").parse_assign_config(cfg)
    ws, target, counts, best = ops.assign_anchors_workspace(B, H, W, boxes.shape[1], dev, best=True)
    target.fill_(-77); counts.fill_(-77); best.fill_(-77.0); ws.fill_(0x5A5A5A5A)          # nothing depends on the buffers' contents
    args = (torch.from_numpy(anc).cuda(), boxes.cuda(), nb.to(torch.int32).cuda(), H, W, pos_iou, neg_iou)
    ops.assign_anchors_iou(*args, target, counts, ws, best=best)
    for b in range(B):
        t, bst, cnt = want[b]
        assert np.array_equal(target[b].reshape(-1).cpu().numpy(), t), (name, b)
        assert np.array_equal(counts[b].cpu().numpy(), cnt), (counts[b].tolist(), cnt.tolist())
        err = np.abs(best[b].reshape(-1).cpu().numpy() - bst).max()
        print("sample %d: counts %s, max |best - statement| %.3g" % (b, cnt.tolist(), err))
        assert err <= 1e-12
    assert want[SPECIAL][2][3] == 1 and int(counts[:, 0].max()) > 0
    if int(nb.max()) > boxes.shape[1]:          # nbox beyond the label rows is clamped to them
        t2, c2 = torch.empty_like(target), torch.empty_like(counts)
        ops.assign_anchors_iou(args[0], args[1], args[2].clamp(max=boxes.shape[1]), H, W, pos_iou, neg_iou, t2, c2, ws)
        assert torch.equal(t2, target) and torch.equal(c2, counts)
    # a second call, without best: bit for bit
    t2, c2 = torch.empty_like(target), torch.empty_like(counts)
    ops.assign_anchors_iou(*args, t2, c2, ws)
    assert torch.equal(t2, target) and torch.equal(c2, counts)


@pytest.mark.parametrize("name, pattern", [(n, p) for n in MAPS for p in PATTERNS])
def test_anchor_loss_equals_the_host_statement(name, pattern):
    cfg, boxes, nb, H, W, cls, reg, want = _want(name, pattern)
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, cls, reg, keep=True)
    print("loss %.9g want %.9g; terms %s" % (loss.item(), want[0], terms.cpu().tolist()))
    close(loss.item(), gc, gr, terms, want)
    assert L.calls == 0 and terms.shape == (B, 3) and terms.dtype == torch.float32 and terms.is_cuda
    target, best, counts = L.last_samples
    assert target.shape == (B, 2, H * W) and best.dtype == torch.float64 and torch.equal(counts[:, 0].float(), terms[:, 2])
    for b in range(B):
        assert np.array_equal(target[b].reshape(-1).cpu().numpy(), assigned(name)[0][b][0])
    ign = (target == -2).reshape(B, 2, 1, H, W)
    assert not gc.reshape(B, 2, 2, H, W)[ign.expand(B, 2, 2, H, W)].any() and not gr.reshape(B, 2, 7, H, W)[ign.expand(B, 2, 7, H, W)].any()
    assert float(gr.abs().sum()) > 0 and not gr.reshape(B, 2, 7, H, W)[(target < 0).reshape(B, 2, 1, H, W).expand(B, 2, 7, H, W)].any()
    if pattern == "saturated":
        assert float(gc.abs().max()) > 1e9                                         # the clamp's bounded push at p_t = 0


@pytest.mark.parametrize("alpha, gamma", [(0.25, 0.0), (0.5, 2.5)])
def test_anchor_loss_other_exponents(alpha, gamma):
    cfg, boxes, nb, H, W, cls, reg, want = _want("37x29", "saturated", focal_alpha=alpha, focal_gamma=gamma)
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, cls, reg)
    close(loss.item(), gc, gr, terms, want)


def test_a_nan_score_reaches_the_loss_and_its_own_gradient_only():
    name = "96x80"
    cfg, boxes, nb, H, W, cls, reg, want = _want(name, "uniform")
    HW = H * W
    target = assigned(name)[0][1][0]
    jp, jn = int(np.flatnonzero(target >= 0)[0]), int(np.flatnonzero(target == -1)[-1])
    for j, y in ((jp, 1), (jn, 0)):              # a positive anchor's object score; a negative anchor's background score
        a, cell = divmod(j, HW)
        ch = 2 * a + y
        bad = cls.clone()
        bad.reshape(B, 4, HW)[1, ch, cell] = float("nan")
        L, loss, gc, gr, terms = _run(cfg, boxes, nb, bad, reg)
        assert torch.isnan(loss).all() and torch.isnan(terms[1, 0]) and torch.isfinite(terms[[0, 2]]).all() and torch.isfinite(terms[1, 1:]).all()
        nan = torch.isnan(gc).reshape(B, 4, HW)
        assert bool(nan[1, ch, cell]) and int(nan.sum()) == 1 and torch.isfinite(gr).all()
        keep = ~nan.reshape(gc.shape).cpu().numpy()
        got = gc.cpu().double().numpy()
        assert (np.abs(got - want[1])[keep] <= (1e-7 + 1e-5 * np.abs(want[1]))[keep]).all()
    ji = int(np.flatnonzero(target == -2)[0])      # an ignored anchor reads its scores but they enter nothing
    a, cell = divmod(ji, HW)
    bad = cls.clone()
    bad.reshape(B, 4, HW)[1, 2 * a:2 * a + 2, cell] = float("nan")
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, bad, reg)
    close(loss.item(), gc, gr, terms, want)


@pytest.mark.parametrize("kind", ["ignored", "negative", "one positive"])
def test_hand_written_targets_and_every_gradient_element_is_stored(kind):
    """ops.loss_anchor on a target map written by hand; the gradient buffers start as garbage (no zero fill is needed), the workspace too."""
    cfg, boxes, nb, H, W = case("37x29", loss_reduction="sum")
    HW = H * W
    anc = anchors_of(cfg)
    cls, reg = scores("uniform", H, W), regression_input(H, W)
    targets = np.full((B, 2 * HW), -2 if kind == "ignored" else -1, dtype=np.int32)
    if kind == "one positive":
        targets[0, HW + 500] = 3
        targets[2, 17] = 0
        targets[2, 18] = 64                        # outside [-2, max_box): counts as ignored on both sides
    counts = np.zeros((B, 4), np.int32)
    counts[:, 0] = (targets >= 0).sum(1) - (targets >= boxes.shape[1]).sum(1)
    want = terms_statement(cfg, anc, boxes, torch.tensor([boxes.shape[1]] * B), list(targets), cls, reg, H, W)
    ops, Lm = pkg("ops"), pkg("loss")
    alpha, gamma, eps = Lm.parse_focal_config(cfg)
    dev = torch.device("cuda")
    ws, terms = ops.loss_anchor_workspace(B, H, W, dev)
    ws.fill_(float("nan")); terms.fill_(float("nan"))
    gc, gr = torch.full((B, 4, H, W), 1e30, device=dev), torch.full((B, 14, H, W), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    c1, r1 = cls.cuda(), reg.cuda()
    ops.loss_anchor(c1, r1, torch.from_numpy(anc).cuda(), boxes.cuda(), torch.from_numpy(targets).cuda().reshape(B, 2, HW),
                    torch.from_numpy(counts).cuda(), alpha, gamma, eps, float(cfg["regress_loss_gain"]), Lm.REDUCTION["sum"], loss, gc, gr, terms, ws)
    close(loss.item(), gc, gr, terms, want)
    if kind == "ignored":
        assert loss.item() == 0 and not gc.any() and not gr.any() and not terms.any()
    if kind == "negative":
        assert loss.item() > 0 and not gr.any() and not terms[:, 1:].any() and not gc[:, 1::2].any()
    if kind == "one positive":
        assert terms[:, 2].tolist() == [1, 0, 1] and int((gr != 0).sum()) == 14 and int((gc[:, 1::2] != 0).sum()) == 2


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_anchor_reductions_and_labels_on_the_device(reduction):
    cfg, boxes, nb, H, W, cls, reg, want = _want("96x80", "uniform", loss_reduction=reduction)
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, cls, reg)
    close(loss.item(), gc, gr, terms, want)
    if reduction == "last":
        assert not gc[:B - 1].any() and not gr[:B - 1].any() and not terms[:B - 1].any() and float(gc[B - 1].abs().sum()) > 0
    on_dev = _run(cfg, boxes, nb, cls, reg, boxes_dev=True, L=L)          # the same module again: its buffers are reused
    for a, b in zip(on_dev[1:], (loss, gc, gr, terms)):
        assert torch.equal(a, b)
    assert L.calls == 0


@pytest.mark.parametrize("deterministic", [False, True])
def test_two_calls_are_bit_identical(deterministic):
    cfg, boxes, nb, H, W, cls, reg, want = _want("96x80", "softmax")
    runs = [_run(dict(cfg, deterministic=deterministic), boxes, nb, cls, reg) for _ in range(2)]
    for a, b in zip(runs[0][1:], runs[1][1:]):                   # loss, gcls, greg, terms
        assert torch.equal(a, b)
    close(runs[0][1].item(), runs[0][2], runs[0][3], runs[0][4], want)


def test_rejected_arguments_launch_nothing():
    Hm, ops, Lm = pkg("_hip"), pkg("ops"), pkg("loss")
    cfg, boxes, nb, H, W = case("16x8")
    dev = torch.device("cuda")
    HW = H * W
    anc = torch.from_numpy(anchors_of(cfg)).cuda()
    bx, nbd = boxes.cuda(), nb.to(torch.int32).cuda()
    ws, target, counts, _ = ops.assign_anchors_workspace(B, H, W, boxes.shape[1], dev)
    target.fill_(-77); counts.fill_(-77)
    lib = Hm.lib()
    assert lib.dcf_assign_anchors_workspace_bytes(B, H, W, 0) == 0 and lib.dcf_assign_anchors_workspace_bytes(B, H, W, 65) == 0
    assert lib.dcf_assign_anchors_workspace_bytes(1, 1 << 15, 1 << 15, 8) == 0 and lib.dcf_loss_anchor_workspace_bytes(1, 1 << 15, 1 << 15) == 0

    def assign(anchors=anc, labels=bx, n=nbd, max_box=boxes.shape[1], Hh=H, Ww=W, pos=0.6, neg=0.45, t=target, c=counts, w=ws):
        return lib.dcf_assign_anchors_iou(*[Hm._ptr(v) for v in (anchors, labels, n, max_box, 9, B, Hh, Ww, pos, neg, t, None, c, w, Hm.stream_ptr())])

    for kw in (dict(max_box=0), dict(max_box=65), dict(Hh=1 << 15, Ww=1 << 15), dict(pos=0.4, neg=0.45), dict(neg=0.0), dict(pos=1.5),
               dict(pos=float("nan")), dict(anchors=None), dict(labels=None), dict(n=None), dict(t=None), dict(c=None), dict(w=None)):
        assert assign(**kw) == -1 and lib.dcf_last_error().decode().startswith("dcf_assign_anchors_iou"), kw
    alpha, gamma, eps = Lm.parse_focal_config(cfg)
    lws, terms = ops.loss_anchor_workspace(B, H, W, dev)
    cls, reg = scores("uniform", H, W).cuda(), regression_input(H, W).cuda()
    gc, gr, loss = torch.full_like(cls, -77.0), torch.full_like(reg, -77.0), torch.full((1,), -77.0, device=dev)
    tg, cn = torch.full((B, 2, HW), -1, dtype=torch.int32, device=dev), torch.zeros((B, 4), dtype=torch.int32, device=dev)

    def terms_call(c=cls, r=reg, anchors=anc, labels=bx, max_box=boxes.shape[1], t=tg, n=cn, Hh=H, Ww=W, out=loss, g1=gc, g2=gr, tm=terms, w=lws):
        return lib.dcf_loss_anchor_fwd_bwd(*[Hm._ptr(v) for v in (c, 4 * HW, r, 14 * HW, anchors, labels, max_box, 9, t, n, B, Hh, Ww, alpha, gamma,
                                                                   eps, 3.0, 1, out, g1, 4 * HW, g2, 14 * HW, tm, w, Hm.stream_ptr())])

    for kw in (dict(max_box=0), dict(max_box=65), dict(Hh=1 << 15, Ww=1 << 15), dict(c=None), dict(r=None), dict(anchors=None), dict(labels=None),
               dict(t=None), dict(n=None), dict(out=None), dict(g1=None), dict(g2=None), dict(tm=None), dict(w=None)):
        assert terms_call(**kw) == -1 and lib.dcf_last_error().decode().startswith("dcf_loss_anchor_fwd_bwd"), kw
    torch.cuda.synchronize()
    assert (target == -77).all() and (counts == -77).all() and (gc == -77).all() and (gr == -77).all() and loss.item() == -77
    with pytest.raises(Hm.DcfError):              # through the module: more label rows than the entry takes
        Lm.LossTotal(cfg).cuda()(torch.zeros(B, 65, 9), torch.tensor([65] * B), cls.clone().requires_grad_(True), reg.clone().requires_grad_(True))
    assert assign() == 0 and terms_call() == 0    # the same calls with nothing wrong


@pytest.mark.parametrize("deterministic, loss_scale", [(False, "none"), (True, "dynamic")])
def test_train_step_with_anchor_loss(deterministic, loss_scale):
    """Train.one_step with loss_sampling: anchor on the tiny model: finite loss, parameters move, at least one positive anchor, no
    generator consumed, the read-out agrees with the loss."""
    z = load_golden("model_tiny.npz")
    lz = load_golden("loss.npz")
    cfg = golden_cfg(z)
    cfg.update(dtype="f32", loss_sampling="anchor", deterministic=deterministic, loss_scale=loss_scale)
    T = pkg("train")
    det = pkg("detfill")
    u = det.uniform((1, 32, 64, 32), 4242, 0.0, 1.0)
    x = torch.from_numpy(u.astype(np.float32)).cuda()
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device="cuda")
    boxes, nbx = torch.from_numpy(lz["bboxes"])[:1], torch.from_numpy(lz["nbox"])[:1]
    gain = cfg["regress_loss_gain"]
    np.random.seed(11)
    rng = np.random.get_state()[1].copy()
    tr = T.Train(cfg)
    det.fill_state_dict(tr.model)
    start = tr.model.flat_params.clone()
    assert tr.loss_terms() is None                            # nothing computed yet
    for _ in range(2):
        tr.one_step(x, img, boxes, nbx)
        terms = tr.loss_terms()
        want = float(terms[-1, 0]) + gain * float(terms[-1, 1])          # loss_reduction: last (the default)
        assert abs(tr.loss_value.item() - want) <= 1e-6 * max(1.0, abs(want))
        assert terms.shape == (1, 3) and int(terms[0, 2]) >= 1
    assert np.isfinite(tr.loss_value.item()) and not torch.equal(start, tr.model.flat_params)
    assert tr.loss_total.calls == 0
    assert np.array_equal(np.random.get_state()[1], rng)

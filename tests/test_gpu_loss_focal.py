"""loss_sampling: focal (dense focal classification; csrc/loss.hip k_loss_focal / k_focal_fold): value, gradients
and the terms read-out against the float64 host statement (loss.focal_terms + the regression term in float64) at the project's bounds
for fp32 loss kernels against float64 (tests/test_gpu_head_loss_edges.py: loss 2e-6 * max(1, |loss|), gradients rtol 1e-5 / atol 1e-7),
|P_b| exactly; NaN propagation; the deterministic entry; the reductions; the train step."""
import numpy as np
import pytest
import torch

from _focal_util import B, MAPS, PATTERNS, case, close, positive_set, regression_input, scores, statement
from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(name, pattern, **over):
    """The float64 statement of one case, computed once."""
    key = (name, pattern, tuple(sorted(over.items())))
    if key not in _WANT:
        cfg, boxes, nb, H, W = case(name, **over)
        cls, reg = scores(pattern, H, W), regression_input(H, W)
        _WANT[key] = (cfg, boxes, nb, H, W, cls, reg, statement(cfg, boxes, nb, cls, reg, H, W))
    return _WANT[key]


def _run(cfg, boxes, nb, cls, reg, boxes_dev=False, L=None):
    if L is None:
        L = pkg("loss").LossTotal(cfg).cuda()
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    loss = L(boxes.cuda() if boxes_dev else boxes, nb.cuda() if boxes_dev else nb, c1, r1)
    loss.backward()
    return L, loss, c1.grad, r1.grad, L.last_terms.clone()


CASES = [(n, p) for n in MAPS if n != "352x400" for p in PATTERNS] + [("352x400", "softmax")]


@pytest.mark.parametrize("name, pattern", CASES)
def test_focal_equals_the_host_statement(name, pattern):
    cfg, boxes, nb, H, W, cls, reg, want = _want(name, pattern, loss_reduction="mean")
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, cls, reg)
    print("loss %.9g want %.9g; terms %s" % (loss.item(), want[0], terms.cpu().tolist()))
    close(loss.item(), gc, gr, terms, want)
    assert L.calls == 0 and terms.shape == (B, 3) and terms.dtype == torch.float32 and terms.is_cuda
    n_entries = [positive_set(L, boxes[b].numpy(), int(nb[b]), H, W)[1] for b in range(B)]
    if name == "64x48-0":
        assert not terms[:, 1:].any() and not gr.any()
    if name == "64x48-20":
        assert all(0 < int(terms[b, 2]) < n_entries[b] for b in range(B))          # overlapping windows: cells counted once
    if pattern == "saturated":
        assert float(gc.abs().max()) > 1e9                                         # the clamp's bounded push at p_t = 0


@pytest.mark.parametrize("alpha, gamma", [(0.25, 0.0), (0.25, 1.0), (0.5, 2.5)])
@pytest.mark.parametrize("pattern", ["softmax", "saturated"])
def test_focal_other_exponents(pattern, alpha, gamma):
    cfg, boxes, nb, H, W, cls, reg, want = _want("37x29", pattern, loss_reduction="mean", focal_alpha=alpha, focal_gamma=gamma)
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, cls, reg)
    close(loss.item(), gc, gr, terms, want)


@pytest.mark.parametrize("name", ["37x29", "96x80"])
def test_a_nan_score_reaches_the_loss_and_its_own_gradient_only(name):
    cfg, boxes, nb, H, W, cls, reg, want = _want(name, "uniform", loss_reduction="mean")
    L0 = pkg("loss").LossTotal(cfg)
    pos = sorted(positive_set(L0, boxes[1].numpy(), int(nb[1]), H, W)[0])
    for ch, cell in ((1, pos[0]), (2, H * W - 1)):               # a positive cell's object score; the last cell's background score
        assert (cell in pos) == (ch % 2 == 1)
        bad = cls.clone()
        bad.reshape(B, 4, H * W)[1, ch, cell] = float("nan")
        L, loss, gc, gr, terms = _run(cfg, boxes, nb, bad, reg)
        assert torch.isnan(loss).all() and torch.isnan(terms[1, 0]) and torch.isfinite(terms[[0, 2]]).all()
        nan = torch.isnan(gc).reshape(B, 4, H * W)
        assert bool(nan[1, ch, cell]) and int(nan.sum()) == 1 and torch.isfinite(gr).all()
        keep = ~nan.reshape(gc.shape).cpu().numpy()
        ref = want[1]
        got = gc.cpu().double().numpy()
        assert (np.abs(got - ref)[keep] <= (1e-7 + 1e-5 * np.abs(ref))[keep]).all()


def test_focal_deterministic_entry():
    cfg, boxes, nb, H, W, cls, reg, want = _want("64x48-20", "softmax", loss_reduction="mean")
    det = [_run(dict(cfg, deterministic=True), boxes, nb, cls, reg) for _ in range(2)]
    for a, b in zip(det[0][1:], det[1][1:]):                     # loss, gcls, greg, terms: bit for bit
        assert torch.equal(a, b)
    close(det[0][1].item(), det[0][2], det[0][3], det[0][4], want)
    plain = [_run(cfg, boxes, nb, cls, reg) for _ in range(2)]
    for run in plain:                                            # the plain entry: only greg goes through atomics
        assert torch.equal(run[1], det[0][1]) and torch.equal(run[2], det[0][2]) and torch.equal(run[4], det[0][4])
        close(run[1].item(), run[2], run[3], run[4], want)
    assert float(det[0][3].abs().sum()) > 0


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_focal_reductions_and_labels_on_the_device(reduction):
    cfg, boxes, nb, H, W, cls, reg, want = _want("96x80", "uniform", loss_reduction=reduction)
    L, loss, gc, gr, terms = _run(cfg, boxes, nb, cls, reg)
    close(loss.item(), gc, gr, terms, want)
    if reduction == "last":
        assert not gc[:B - 1].any() and not gr[:B - 1].any() and not terms[:B - 1].any() and float(gc[B - 1].abs().sum()) > 0
    on_dev = _run(cfg, boxes, nb, cls, reg, boxes_dev=True, L=L)          # the same module again: its buffers are reused
    assert torch.equal(on_dev[1], loss) and torch.equal(on_dev[2], gc) and torch.equal(on_dev[4], terms)
    close(on_dev[1].item(), on_dev[2], on_dev[3], on_dev[4], want)
    assert L.calls == 0


def test_focal_regression_maps_are_those_of_the_device_sampler():
    cfg, boxes, nb, H, W, cls, reg, want = _want("64x48-20", "uniform", loss_reduction="mean")
    for regress_type in (0, 1):
        c2 = dict(cfg, regress_type=regress_type)
        gr = _run(c2, boxes, nb, cls, reg)[3]
        Ld = pkg("loss").LossTotal(dict(c2, loss_sampling="device")).cuda()
        r2 = reg.cuda().requires_grad_(True)
        Ld(boxes, nb, cls.cuda().requires_grad_(True), r2).backward()
        assert torch.allclose(gr, r2.grad, rtol=1e-5, atol=1e-7) and float(gr.abs().sum()) > 0
    # nbox beyond the label rows is clamped to them
    few = boxes[:, :1].contiguous()
    a = _run(cfg, few, torch.tensor([9] * B), cls, reg)
    b = _run(cfg, few, torch.tensor([1] * B), cls, reg)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.isfinite(a[1]).all()


def test_focal_rejected_shapes():
    """More than 64 boxes, or max_box * span^2 > 1024, raise as they do in device mode."""
    Hm = pkg("_hip")
    cfg, boxes, nb, H, W, cls, reg, want = _want("64x48-20", "uniform", loss_reduction="mean")
    for rows, span in ((65, 5), (64, 5), (20, 8)):
        L = pkg("loss").LossTotal(dict(cfg, positive_range=span)).cuda()
        many = torch.zeros(B, rows, 9)
        many[:, :, :7] = boxes[0, 1, :7]
        with pytest.raises(Hm.DcfError):
            L(many, torch.tensor([rows] * B), cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True))


@pytest.mark.parametrize("deterministic, loss_scale", [(False, "none"), (True, "none"), (False, "dynamic")])
def test_train_step_with_focal_loss(deterministic, loss_scale):
    """Train.one_step with loss_sampling: focal on the tiny model: finite loss, parameters move, no generator consumed, the read-out
    agrees with the loss; with deterministic: true two trainers agree bit for bit after two steps."""
    z = load_golden("model_tiny.npz")
    lz = load_golden("loss.npz")
    cfg = golden_cfg(z)
    cfg.update(dtype="f32", loss_sampling="focal", deterministic=deterministic, loss_scale=loss_scale)
    T = pkg("train")
    det = pkg("detfill")
    u = det.uniform((1, 32, 64, 32), 4242, 0.0, 1.0)
    x = torch.from_numpy(u.astype(np.float32)).cuda()
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device="cuda")
    boxes, nbx = torch.from_numpy(lz["bboxes"])[:1], torch.from_numpy(lz["nbox"])[:1]
    gain = cfg["regress_loss_gain"]
    np.random.seed(11)
    rng = np.random.get_state()[1].copy()
    runs = []
    for rep in range(2 if deterministic else 1):
        tr = T.Train(cfg)
        det.fill_state_dict(tr.model)
        start = tr.model.flat_params.clone()
        assert tr.loss_terms() is None                            # nothing computed yet
        out = []
        for _ in range(2):
            tr.one_step(x, img, boxes, nbx)
            terms = tr.loss_terms()
            out.append((tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone(), terms))
            want = float(terms[-1, 0]) + gain * float(terms[-1, 1])          # loss_reduction: last (the default)
            assert abs(tr.loss_value.item() - want) <= 1e-6 * max(1.0, abs(want))
            assert terms.shape == (1, 3) and int(terms[0, 2]) > 0
        assert np.isfinite(out[-1][0].item()) and not torch.equal(start, out[-1][2])
        assert tr.loss_total.calls == 0
        runs.append(out)
    assert np.array_equal(np.random.get_state()[1], rng)
    if deterministic:
        for a, b in zip(runs[0], runs[1]):
            assert all(torch.equal(x1, x2) for x1, x2 in zip(a, b))

"""loss_sampling: hard (hard negative mining; csrc/loss.hip k_hard_*): the device lists bit for bit against the
host statement of the selection (loss.hard_negatives -- integer work on both sides), their properties, and loss / gradients against
the list-driven kernel (dcf_loss_fwd_bwd) fed the same lists, at the bounds tests/test_gpu_loss_sampling.py uses between the same two
kernels for the device sampler (loss 2e-6 relative, gradients rtol 1e-5 / atol 1e-7: the arithmetic on the lists is the same)."""
import numpy as np
import pytest
import torch

from _loss_util import assign_lists
from _util import M64, golden_cfg, load_golden, pkg
from test_gpu_loss_sampling import _setup, sampler_statement

pytestmark = pytest.mark.gpu

B = 3
# name -> (H, W, boxes per sample, out-of-grid first box)
MAPS = {
    "64x48-0": (64, 48, 0, False),
    "64x48-3": (64, 48, 3, True),
    "64x48-20": (64, 48, 20, True),        # more window entries than pos_sample_threshold: the cut drops window cells
    "37x29": (37, 29, 5, True),            # a multiple of no wave, workgroup or digit size
    "16x8": (16, 8, 3, False),             # fewer candidates than neg_count
    "16x12": (16, 12, 3, False),           # candidates exceed neg_count by fewer than 64
    "96x80": (96, 80, 6, True),            # several workgroups per sample
    "352x400": (352, 400, 6, True),        # more than 64 x 1024 cells: the chunk of a workgroup grows, keys far beyond LDS
}
PATTERNS = ["uniform", "quantised", "constant", "anchor0", "anchor1", "negative", "zeros", "windows"]


def _case(name):
    H, W, n_boxes, far = MAPS[name]
    cfg, boxes, nb, _, _, _, _ = _setup(n_boxes, far=far)
    cfg = dict(cfg, voxel_length=4 * H, voxel_width=4 * W, loss_sampling="hard")
    return cfg, boxes, nb, H, W


def _scores(pattern, H, W, windows, seed=0):
    """cls [B,4,H,W] of one score pattern; windows[b] = the window entries (cells) of sample b."""
    g = torch.Generator().manual_seed(1000 + seed)
    HW = H * W
    cls = torch.rand(B, 4, HW, generator=g)
    if pattern == "quantised":                       # multiples of 1/8: 17 distinct d values, long ties that straddle the cut
        cls = torch.round(cls * 8) / 8
    elif pattern == "constant":                      # one key everywhere: the first candidates by index
        cls = torch.full((B, 4, HW), 0.25)
    elif pattern in ("anchor0", "anchor1"):          # the hard cells show in one anchor only
        a = 0 if pattern == "anchor0" else 1
        cls = cls * 0.1
        hard = torch.rand(B, HW, generator=g) < 0.3
        cls[:, 2 * a + 1] += hard.float() * (2.0 + torch.rand(B, HW, generator=g))
        cls[:, 2 * (1 - a)] += 1.0
    elif pattern == "negative":                      # every d negative, magnitudes over six decades
        mag = 10.0 ** (torch.rand(B, 4, HW, generator=g) * 6 - 3)
        cls = torch.where(torch.tensor([False, True, False, True]).view(1, 4, 1), -mag, mag)
    elif pattern == "zeros":                         # d = -0.0 (s1 = -0.0, s0 = +0.0) beside d = +0.0 (s1 = s0)
        minus = torch.rand(B, 2, HW, generator=g) < 0.6
        cls = torch.full((B, 4, HW), 0.3)
        for a in range(2):
            cls[:, 2 * a][minus[:, a]] = 0.0
            cls[:, 2 * a + 1][minus[:, a]] = -0.0
    elif pattern == "windows":                       # the globally highest keys sit inside windows (cells the cut dropped included)
        for b in range(B):
            if len(windows[b]):
                idx = torch.tensor(sorted(set(windows[b])))
                cls[b, 1, idx] += 100.0
                cls[b, 3, idx] += 50.0
    return cls.reshape(B, 4, H, W).contiguous()


_SHARED = {}


def _shared(name):
    """Per map, computed once: config, labels, window entries per sample, the positive
    lists `loss_sampling: device` returns for the same seed, and the regression head input."""
    if name in _SHARED:
        return _SHARED[name]
    cfg, boxes, nb, H, W = _case(name)
    Lm = pkg("loss")
    Lh = Lm.LossTotal(cfg)
    windows = [Lh.windows(boxes[b, :int(nb[b])].numpy(), H, W)[0] for b in range(B)]
    reg = torch.rand(B, 14, H, W, generator=torch.Generator().manual_seed(9)) - 0.5
    Ld = Lm.LossTotal(dict(cfg, loss_sampling="device")).cuda()
    Ld.keep_samples = True
    Ld(boxes, nb, torch.rand(B, 4, H, W).cuda(), reg.cuda())
    dev_pos, _, dev_counts = [t.cpu().numpy() for t in Ld.last_samples]
    _SHARED[name] = (cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts)
    return _SHARED[name]


def _statement(name, cls, call=0):
    """(pos, neg, window entries) per sample from the host statement."""
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    Lm = pkg("loss")
    L = Lm.LossTotal(cfg)
    seed = (cfg["loss_seed"] * 0x9E3779B1 + call) & M64
    out = []
    for b in range(B):
        pos, _, n_entries = sampler_statement(L, boxes[b].numpy(), int(nb[b]), H, W, seed, b)
        assert n_entries == len(windows[b])
        neg = Lm.hard_negatives(cls[b].reshape(4, H * W).numpy(), windows[b], cfg["neg_sample_threshold"] + 1)
        out.append((pos, [int(v) for v in neg], n_entries))
    return out


def _list_kernel(name, cls, lists, reduction="mean", deterministic=False):
    """dcf_loss_fwd_bwd on the given lists: (loss, dL/dcls, dL/dreg)."""
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    Lc = pkg("loss").LossTotal(dict(cfg, loss_sampling="compat", loss_reduction=reduction, deterministic=deterministic)).cuda()
    ints, floats, plan = assign_lists(Lc, boxes, nb, H, W, lists)[2]
    c2, r2 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    anc = Lc.anchor_set.cuda().reshape(2, 7, H * W)
    ref = Lc._forward_hip(c2, r2, anc, ints, floats, plan, B, H, W)
    ref.backward()
    return ref.item(), c2.grad, r2.grad


def _run_hard(name, cls, keep=True, boxes_dev=False, L=None, **over):
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    if L is None:
        L = pkg("loss").LossTotal(dict(cfg, **over)).cuda()
    L.keep_samples = keep
    c1, r1 = cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    loss = L(boxes.cuda() if boxes_dev else boxes, nb.cuda() if boxes_dev else nb, c1, r1)
    loss.backward()
    samples = [t.cpu().numpy() for t in L.last_samples] if keep else None
    return L, loss, c1.grad, r1.grad, samples


def _close(loss, gc, gr, ref):
    assert abs(loss.item() - ref[0]) <= 2e-6 * max(1.0, abs(ref[0])), (loss.item(), ref[0])
    assert torch.allclose(gc, ref[1], rtol=1e-5, atol=1e-7) and torch.allclose(gr, ref[2], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(MAPS))
def test_hard_lists_equal_the_host_statement(name, pattern):
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    Lm = pkg("loss")
    cls = _scores(pattern, H, W, windows)
    L, loss, gc, gr, (pos, neg, counts) = _run_hard(name, cls)
    want = _statement(name, cls)
    cap, nneg = cfg["pos_sample_threshold"], cfg["neg_sample_threshold"] + 1
    assert neg.shape == (B, nneg) and counts.shape == (B, 3)
    for b in range(B):
        want_pos, want_neg, n_entries = want[b]
        got_pos = [int(v) for v in pos[b] if v >= 0]
        n_neg = int(counts[b, 2])
        got_neg = [int(v) for v in neg[b][:n_neg]]
        win = set(windows[b])
        n_cand = H * W - len(win)
        # --- the lists equal the statement; -1 in unused slots
        assert got_neg == want_neg, (b, got_neg[:8], want_neg[:8])
        assert got_pos == want_pos
        assert n_neg == min(nneg, n_cand) and list(neg[b][n_neg:]) == [-1] * (nneg - n_neg)
        assert int(counts[b, 0]) == len(want_pos) == min(n_entries, cap) and int(counts[b, 1]) == n_entries
        # --- no duplicates, in range, no window cell (cells the positive cut dropped included)
        assert len(set(got_neg)) == n_neg and all(0 <= v < H * W for v in got_neg) and not (set(got_neg) & win)
        # --- order: key descending, then cell ascending; nothing left out scores higher than the last one taken
        keys = Lm.hard_keys(cls[b].reshape(4, H * W).numpy()).astype(np.int64)
        order = [(-int(keys[v]), v) for v in got_neg]
        assert order == sorted(order)
        if n_neg < n_cand:
            rest = np.array(sorted(set(range(H * W)) - win - set(got_neg)))
            assert (-int(keys[rest].max()), int(rest[np.argmax(keys[rest])])) > order[-1]
        # --- the positives are those of loss_sampling: device on the same seed and call
        assert list(pos[b]) == list(dev_pos[b]) and list(counts[b, :2]) == list(dev_counts[b])
    if name == "16x8":
        assert (counts[:, 2] < nneg).all()
    if name == "16x12":
        assert all(0 < H * W - len(set(windows[b])) - nneg < 64 for b in range(B))
    if name == "64x48-20":
        assert int(counts[0, 1]) > cap
    if pattern == "windows" and name != "64x48-0":
        kmax = max(int(Lm.hard_keys(cls[b].reshape(4, H * W).numpy()).max()) for b in range(B))
        assert all(int(Lm.hard_keys(cls[b].reshape(4, H * W).numpy())[neg[b][0]]) < kmax for b in range(B) if windows[b])
    # --- loss and gradients: the list-driven kernel on the same lists
    _close(loss, gc, gr, _list_kernel(name, cls, want))


@pytest.mark.parametrize("reduction", ["last", "sum", "mean"])
def test_hard_reductions(reduction):
    name = "64x48-3"
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    cls = _scores("uniform", H, W, windows, seed=1)
    want = _statement(name, cls)
    ref = _list_kernel(name, cls, want, reduction=reduction)
    for keep in (True, False):
        L, loss, gc, gr, samples = _run_hard(name, cls, keep=keep, loss_reduction=reduction)
        _close(loss, gc, gr, ref)
        if keep:                                      # every sample is mined when the lists are asked for, whatever the reduction
            assert [[int(v) for v in samples[1][b][:samples[2][b, 2]]] for b in range(B)] == [w[1] for w in want]
        if reduction == "last":
            assert float(gc[:B - 1].abs().sum()) == 0.0 and float(gr[:B - 1].abs().sum()) == 0.0 and float(gc[B - 1].abs().sum()) > 0.0


@pytest.mark.parametrize("pattern", ["uniform", "quantised"])
def test_hard_deterministic_entry(pattern):
    name = "64x48-20"                                 # overlapping windows: cells repeat in the positive list
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    cls = _scores(pattern, H, W, windows, seed=2)
    runs = [_run_hard(name, cls, deterministic=True) for _ in range(2)]
    for a, b in zip(runs[0][1:4], runs[1][1:4]):
        assert torch.equal(a, b)
    plain = _run_hard(name, cls)
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][4], plain[4]))
    _close(plain[1], plain[2], plain[3], (runs[0][1].item(), runs[0][2], runs[0][3]))
    assert float(runs[0][2].abs().sum()) > 0 and float(runs[0][3].abs().sum()) > 0


def test_hard_negatives_ignore_the_call_count_and_labels_may_live_on_the_device():
    name = "64x48-20"
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    cls = _scores("uniform", H, W, windows, seed=3)
    L, _, _, _, first = _run_hard(name, cls)
    _, _, _, _, second = _run_hard(name, cls, L=L)
    assert L.calls == 2
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
    assert int(first[2][0, 1]) > cfg["pos_sample_threshold"] and not np.array_equal(first[0][0], second[0][0])
    want = _statement(name, cls, call=1)
    assert [[int(v) for v in second[0][b] if v >= 0] for b in range(B)] == [w[0] for w in want]
    _, _, _, _, on_dev = _run_hard(name, cls, boxes_dev=True)
    assert all(np.array_equal(x, y) for x, y in zip(first, on_dev))


def test_hard_rejected_shapes():
    """More than 64 boxes, or neg_count > 512, raise as they do in device mode."""
    Hm = pkg("_hip")
    name = "64x48-3"
    cfg, boxes, nb, H, W, windows, reg, dev_pos, dev_counts = _shared(name)
    cls = _scores("uniform", H, W, windows)
    for mode in ("hard", "device"):
        L = pkg("loss").LossTotal(dict(cfg, loss_sampling=mode, neg_sample_threshold=512)).cuda()
        with pytest.raises(Hm.DcfError):
            L(boxes, nb, cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True))
        L = pkg("loss").LossTotal(dict(cfg, loss_sampling=mode)).cuda()
        many = torch.zeros(B, 65, 9)
        many[:, :, :7] = boxes[0, 0, :7]
        with pytest.raises(Hm.DcfError):
            L(many, torch.tensor([65] * B), cls.cuda().requires_grad_(True), reg.cuda().requires_grad_(True))


@pytest.mark.parametrize("deterministic", [False, True])
def test_train_step_with_hard_mining(deterministic):
    """Train.one_step with loss_sampling: hard on the tiny model (a 16 x 8 map: fewer candidates than neg_count): finite loss,
    parameters move, numpy's generator untouched; with deterministic: true the steps repeat bit for bit from the restored state."""
    z = load_golden("model_tiny.npz")
    lz = load_golden("loss.npz")
    cfg = golden_cfg(z)
    cfg.update(dtype="f32", loss_sampling="hard", loss_seed=3, deterministic=deterministic)
    T = pkg("train")
    det = pkg("detfill")
    tr = T.Train(cfg)
    det.fill_state_dict(tr.model)
    u = det.uniform((1, 32, 64, 32), 4242, 0.0, 1.0)
    x = torch.from_numpy(u.astype(np.float32)).cuda()
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device="cuda")
    boxes, nbx = torch.from_numpy(lz["bboxes"])[:1], torch.from_numpy(lz["nbox"])[:1]
    tr.loss_total.keep_samples = True
    state = dict(p=tr.model.flat_params.clone(), b=tr.model._bufflat.clone(), m=tr.optimizer.m.clone(), v=tr.optimizer.v.clone(),
                 n=tr.optimizer.step_count, calls=tr.loss_total.calls)
    np.random.seed(11)
    rng = np.random.get_state()[1].copy()
    runs = []
    for rep in range(2 if deterministic else 1):
        tr.model.flat_params.copy_(state["p"]); tr.model._bufflat.copy_(state["b"]); tr.optimizer.m.copy_(state["m"]); tr.optimizer.v.copy_(state["v"])
        tr.optimizer.step_count, tr.loss_total.calls = state["n"], state["calls"]
        out = []
        for _ in range(2):
            tr.one_step(x, img, boxes, nbx)
            out.append((tr.loss_value.detach().clone(), tr.model.flat_grads.clone(), tr.model.flat_params.clone()))
        runs.append(out)
    assert np.array_equal(np.random.get_state()[1], rng)
    counts = tr.loss_total.last_samples[2].cpu()
    assert 0 < int(counts[0, 2]) < cfg["neg_sample_threshold"] + 1          # the short-candidate rule ran
    assert np.isfinite(runs[0][-1][0].item()) and not torch.equal(state["p"], runs[0][-1][2])
    if deterministic:
        for a, b in zip(runs[0], runs[1]):
            assert all(torch.equal(x1, x2) for x1, x2 in zip(a, b))

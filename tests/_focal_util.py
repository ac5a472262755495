"""Shared by tests/test_loss_focal_host.py and tests/test_gpu_loss_focal.py: the maps, the score patterns and the float64 statement of
`loss_sampling: focal` (loss.focal_terms for the classification term, the torch regression term evaluated in float64)."""
import numpy as np
import torch

from _util import pkg
from test_gpu_loss_sampling import _setup

B = 3
# name -> (H, W, boxes per sample, out-of-grid first box); the shapes of tests/test_gpu_loss_hard.py, for the same reasons
MAPS = {
    "64x48-0": (64, 48, 0, False),         # no positive cells
    "64x48-20": (64, 48, 20, True),        # overlapping windows: |P_b| differs from the entry count
    "37x29": (37, 29, 5, True),            # a multiple of nothing
    "16x8": (16, 8, 3, False),             # smaller than a workgroup
    "96x80": (96, 80, 6, True),            # several workgroups per sample
    "352x400": (352, 400, 6, True),        # more than 64 x 1024 cells: the chunk of a workgroup grows
}
PATTERNS = ["softmax", "uniform", "saturated"]


def case(name, **over):
    H, W, n_boxes, far = MAPS[name]
    cfg, boxes, nb, _, _, _, _ = _setup(n_boxes, far=far)
    cfg = dict(cfg, voxel_length=4 * H, voxel_width=4 * W, loss_sampling="focal", **over)
    return cfg, boxes, nb, H, W


def positive_set(L, boxes, nb, H, W):
    """P_b restated literally: a set over the reference's window loop (fp32 centre arithmetic, truncation, clipping at the border)."""
    c = L.config
    f32 = np.float32
    rs, span = c["anchor_bbox_feature"]["reduced_scale"], c["positive_range"]
    half = span // 2
    cells = set()
    entries = 0
    for k in range(nb):
        cx = int((f32(boxes[k, 0]) * f32(L._xs) + f32(L._xo)) / f32(rs))
        cy = int((f32(boxes[k, 1]) * f32(L._ys) + f32(L._yo)) / f32(rs))
        if not (0 <= cx <= H - 1 and 0 <= cy <= W - 1):
            continue
        for dx in range(span):
            for dy in range(span):
                px, py = cx - half + dx, cy - half + dy
                if 0 <= px <= H - 1 and 0 <= py <= W - 1:
                    cells.add(px * W + py)
                    entries += 1
    return cells, entries


def scores(pattern, H, W, seed=0):
    """cls [B,4,H,W] fp32: per anchor a pair (background, object) of probabilities."""
    g = torch.Generator().manual_seed(2000 + seed)
    HW = H * W
    if pattern == "softmax":                         # softmax pairs of normal logits x 4: probabilities from 1e-7 to 1 - 1e-7
        cls = torch.softmax(torch.randn(B, 2, 2, HW, generator=g) * 4.0, dim=2).reshape(B, 4, HW)
    elif pattern == "uniform":                       # (1 - u, u)
        u = torch.rand(B, 2, HW, generator=g)
        cls = torch.stack((1.0 - u, u), 2).reshape(B, 4, HW)
    elif pattern == "saturated":                     # exact 0, exact 1 and a denormal among ordinary values: the clamp branch both ways
        u = torch.rand(B, 2, HW, generator=g)
        pick = torch.randint(0, 4, (B, 2, HW), generator=g)
        p1 = torch.where(pick == 0, torch.zeros(()), torch.where(pick == 1, torch.ones(()), torch.where(pick == 2, torch.full((), 1e-42), u)))
        cls = torch.stack((1.0 - p1, p1), 2).reshape(B, 4, HW)
    else:
        raise KeyError(pattern)
    return cls.reshape(B, 4, H, W).contiguous()


def regression_input(H, W):
    return torch.rand(B, 14, H, W, generator=torch.Generator().manual_seed(9)) - 0.5


def statement(cfg, boxes, nb, cls, reg, H, W):
    """The float64 statement: (loss, dL/dcls [B,4,H,W], dL/dreg [B,14,H,W], terms [B,3]) as float64 arrays, for cfg's reduction."""
    Lm = pkg("loss")
    L = Lm.LossTotal(cfg)
    alpha, gamma, eps = L.focal
    gain = float(cfg["regress_loss_gain"])
    red = cfg.get("loss_reduction", "last")
    nB = cls.shape[0]
    anc = L.anchor_set.double().reshape(2, 7, H * W)
    gc, gr = np.zeros((nB, 4, H * W)), np.zeros((nB, 14, H * W))
    terms = np.zeros((nB, 3))
    total = 0.0
    w = 1.0 / nB if red == "mean" else 1.0
    for b in ([nB - 1] if red == "last" else range(nB)):
        n = min(int(nb[b]), boxes.shape[1])
        bx = boxes[b, :n].float().numpy()
        cells, rows, row_box, row_w = L.windows(bx, H, W)
        value, grad = Lm.focal_terms(cls[b].reshape(4, H * W).numpy(), cells, alpha, gamma, eps)
        gc[b] = grad * w
        lr = 0.0
        if rows:
            rb = reg[b].double().clone().requires_grad_(True)
            term = L._reg_term(rb, anc, torch.tensor(rows), torch.tensor(row_box), torch.tensor(row_w, dtype=torch.float64),
                               torch.from_numpy(bx[:, :7]).double(), H, W)
            gr[b] = torch.autograd.grad(term, rb)[0].reshape(14, H * W).numpy() * (gain * w)
            lr = term.item()
        terms[b] = (value, lr, len(set(cells)))
        total += w * (value + gain * lr)
    return total, gc.reshape(nB, 4, H, W), gr.reshape(nB, 14, H, W), terms


def close(loss, gc, gr, terms, want):
    """The project's bounds for fp32 loss kernels against float64 (tests/test_gpu_head_loss_edges.py): loss 2e-6 * max(1, |loss|),
    gradients rtol 1e-5 / atol 1e-7; |P_b| exactly, the two term values at the loss bound."""
    w_loss, w_gc, w_gr, w_terms = want
    assert abs(loss - w_loss) <= 2e-6 * max(1.0, abs(w_loss)), (loss, w_loss)
    for got, ref in ((gc, w_gc), (gr, w_gr)):
        got = got.detach().cpu().double().numpy()
        err = np.abs(got - ref) - (1e-7 + 1e-5 * np.abs(ref))
        assert np.isfinite(got).all() and err.max() <= 0, (float(err.max()), float(np.abs(ref).max()))
    t = terms.detach().cpu().double().numpy()
    assert np.array_equal(t[:, 2], w_terms[:, 2]), (t[:, 2], w_terms[:, 2])
    assert (np.abs(t[:, :2] - w_terms[:, :2]) <= 2e-6 * np.maximum(1.0, np.abs(w_terms[:, :2]))).all(), (t, w_terms)

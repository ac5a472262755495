"""Shared by tests/test_loss_anchor_host.py and tests/test_gpu_loss_anchor.py: the maps, the label sets, the input conditions (decision
margins) and the float64 statement of `loss_sampling: anchor` (assign.anchor_targets + loss.anchor_terms)."""
import math

import numpy as np
import torch

from _focal_util import B
from _util import golden_cfg, load_golden, pkg

PITCH = 0.75                # metres per cell: near the product's, so that anchors reach the thresholds and not only the forcing rule
MARGIN = 1e-9               # every decision of the statement must be at least this far from flipping (the device's cos / sin may
                            # differ from libm's in the last bit: 1e-16 relative on the corners, far below this)
YAW_GAP = 1e-3              # label yaws stay this far from anchor_yaw +- pi, where atan2(sin d, cos d) jumps

# name -> (H, W, label rows per sample = max_box, nbox per sample, seed)
MAPS = {
    "16x8": (16, 8, 4, (3, 0, 4), 3),                  # smaller than a workgroup; a sample without labels
    "37x29": (37, 29, 8, (5, 11, 5), 1),               # a multiple of nothing; nbox beyond the label rows
    "96x80": (96, 80, 64, (5, 64, 6), 2),              # several workgroups per sample; max_box labels, some overlapping
}
SPECIAL = 2                 # the sample whose first two rows are an off-grid label and a void one


def config(H, W, **over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg = dict(cfg, voxel_length=4 * H, voxel_width=4 * W, lidar_x_min=0.0, lidar_x_max=PITCH * (H - 1), lidar_y_min=-PITCH * (W - 1) / 2,
               lidar_y_max=PITCH * (W - 1) / 2, loss_sampling="anchor", loss_reduction="mean")
    cfg.update(over)
    return cfg


def random_labels(g, n, H, W):
    """n rows (x, y, z, l, w, h, yaw, class, 1): centres inside the grid, l in [3.2, 5], w in [1.6, 2.4], yaw uniform in (-pi, pi) but
    for YAW_GAP around -pi/2 and +-pi."""
    u = torch.rand(n, 5, generator=g, dtype=torch.float64)
    rows = torch.zeros(n, 9)
    rows[:, 0] = (0.5 + u[:, 0] * (PITCH * (H - 1) - 1.0)).float()
    rows[:, 1] = ((u[:, 1] - 0.5) * (PITCH * (W - 1) - 1.0)).float()
    rows[:, 2] = -1.0
    rows[:, 3] = (3.2 + 1.8 * u[:, 2]).float()
    rows[:, 4] = (1.6 + 0.8 * u[:, 3]).float()
    rows[:, 5] = 1.5
    yaw = (u[:, 4] * 2.0 - 1.0) * (math.pi - 2 * YAW_GAP)
    yaw = torch.where((yaw + math.pi / 2).abs() < 2 * YAW_GAP, yaw + 4 * YAW_GAP, yaw)
    rows[:, 6] = yaw.float()
    rows[:, 7], rows[:, 8] = 6, 1
    return rows


def case(name, **over):
    """(cfg, boxes [B, max_box, 9], nbox [B], H, W).  Every sample's rows are random labels; in the 64-label sample row 9 repeats row 4
    (an exact tie between two labels, by construction); sample SPECIAL starts with a label far off the grid and a void one (NaN x)."""
    H, W, max_box, nbox, seed = MAPS[name]
    g = torch.Generator().manual_seed(4000 + seed)
    boxes = torch.zeros(B, max_box, 9)
    for b in range(B):
        boxes[b] = random_labels(g, max_box, H, W)
        if nbox[b] == 64:
            boxes[b, 9] = boxes[b, 4]
    boxes[SPECIAL, 0, :2] = torch.tensor([PITCH * (H - 1) + 40.0, 3.0])
    boxes[SPECIAL, 1, 0] = float("nan")
    return config(H, W, max_num_bbox=max_box, **over), boxes, torch.tensor(nbox), H, W


def anchors_of(cfg):
    L = pkg("loss").LossTotal(cfg)
    _, _, h, w = L.anchor_set.shape
    return L.anchor_set.reshape(2, 7, h * w).numpy()


def margins(anchors, rows, pos_iou, neg_iou):
    """The input conditions of one sample, from the host statement: (smallest decision margin, threshold positives, ignored, positive
    through forcing only, forced labels) -- the distances of best(j) to the two thresholds, of every forced anchor's IoU to the runner-up
    anchor's, and of best(j) to the IoU of the next label for every non-negative anchor.  Label rows identical to the winner are left out
    of the last: they tie exactly on both sides."""
    A = pkg("assign")
    I = A.anchor_iou(anchors, rows)
    target, best, counts, forced = A.targets_from_iou(I, A.void_labels(rows), pos_iou, neg_iou)
    m = min(float(np.abs(best - pos_iou).min()), float(np.abs(best - neg_iou).min()))
    rows = np.asarray(rows, dtype=np.float32)
    for k in range(I.shape[1]):
        if forced[k] >= 0:
            col = np.sort(I[:, k])
            m = min(m, float(col[-1] - col[-2]))
    for j in np.flatnonzero(best >= neg_iou):
        arg = int(I[j].argmax())
        others = [k for k in range(I.shape[1]) if k != arg and not np.array_equal(rows[k, :7], rows[arg, :7], equal_nan=True)]
        if others:
            m = min(m, float(best[j] - I[j, others].max()))
    return m, int((best >= pos_iou).sum()), int(counts[1]), int(counts[2]), int((forced >= 0).sum())


def yaw_condition(cfg, rows):
    """Every label yaw at least YAW_GAP away from anchor_yaw +- pi for both anchors."""
    for anchor_yaw in (0.0, 3.1415926 / 2):
        for jump in (anchor_yaw + math.pi, anchor_yaw - math.pi):
            d = np.abs(np.asarray(rows, dtype=np.float64)[:, 6] - jump)
            if d.size and not np.nanmin(d) >= YAW_GAP:
                return False
    return True


_ASSIGNED = {}


def assigned(name):
    """The statement's assignment of every sample of a case, computed once: [(target, best, counts)] * B, and the anchors."""
    if name not in _ASSIGNED:
        cfg, boxes, nb, H, W = case(name)
        anc = anchors_of(cfg)
        pos_iou, neg_iou = pkg("assign").parse_assign_config(cfg)
        out = []
        for b in range(B):
            n = max(min(int(nb[b]), boxes.shape[1]), 0)
            out.append(pkg("assign").anchor_targets(anc, boxes[b, :n].numpy(), pos_iou, neg_iou))
        _ASSIGNED[name] = (out, anc)
    return _ASSIGNED[name]


def terms_statement(cfg, anc, boxes, nb, targets, cls, reg, H, W):
    """The float64 statement of the terms on given targets: (loss, dL/dcls [B,4,H,W], dL/dreg [B,14,H,W], terms [B,3]) for cfg's
    reduction -- the layout tests/_focal_util.close compares."""
    Lm = pkg("loss")
    alpha, gamma, eps = Lm.parse_focal_config(cfg)
    gain, red = float(cfg["regress_loss_gain"]), cfg.get("loss_reduction", "last")
    nB, HW = cls.shape[0], H * W
    gc, gr, terms = np.zeros((nB, 4, HW)), np.zeros((nB, 14, HW)), np.zeros((nB, 3))
    total = 0.0
    w = 1.0 / nB if red == "mean" else 1.0
    for b in ([nB - 1] if red == "last" else range(nB)):
        n = max(min(int(nb[b]), boxes.shape[1]), 0)
        lc, lr, n_pos, g1, g2 = Lm.anchor_terms(cls[b].reshape(4, HW).numpy(), reg[b].reshape(14, HW).numpy(), anc, boxes[b, :n].numpy(),
                                                targets[b], alpha, gamma, eps)
        gc[b], gr[b], terms[b] = g1 * w, g2 * (gain * w), (lc, lr, n_pos)
        total += w * (lc + gain * lr)
    return total, gc.reshape(nB, 4, H, W), gr.reshape(nB, 14, H, W), terms


def statement(name, cls, reg, **over):
    cfg, boxes, nb, H, W = case(name, **over)
    assigned_b, anc = assigned(name)
    return terms_statement(cfg, anc, boxes, nb, [t for t, _, _ in assigned_b], cls, reg, H, W)

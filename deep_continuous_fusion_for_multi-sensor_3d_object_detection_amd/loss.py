"""Drop-in counterpart of the reference's loss.py (LossTotal) -- the train-step harness row.

Same constructor and call surface: LossTotal(config)(bboxes [B,max,9], num_boxes [B],
cls [B,4,h,w], reg [B,14,h,w]) -> [1] loss tensor.  Target assignment is host-side Python
driven by numpy's global RNG exactly like loss.py:74-127 (so np.random.seed pins it); the
device half (gathers, cross-entropy, Smooth-L1 and their gradients) is ONE HIP launch for CUDA tensors
(csrc/loss.hip, dcf_loss_fwd_bwd -- SURVEY.md §8(f) row N1); CPU tensors (the host-logic tests) go through
the same arithmetic as a handful of torch ops.

`loss_sampling: device` moves the target assignment onto the device too (csrc/loss.hip, dcf_loss_sample_fwd_bwd: windows,
subset, negatives, terms and gradients in one launch, a stateless counter hash seeded by `loss_seed` and the call count
instead of numpy's generator) -- no host loop, no index lists over PCIe; `compat` (default) is the mode pinned to the reference.

`loss_sampling: hard` is the device mode with hard negative mining: positives as in `device`, negatives = the
`neg_sample_threshold + 1` cells outside every positive window that the head currently scores most like an object (an exact
top-k over the score map, csrc/loss.hip k_hard_*; no randomness in the negatives).  hard_negatives() below is the host statement
of that selection; CPU tensors take it, so the mode also runs without a device.

`loss_sampling: focal` samples nothing: every cell of both anchors enters the classification term, weighted by the focal factor
alpha_t * (1 - p_t)^gamma and normalised by the number of distinct positive cells (csrc/loss.hip, k_loss_focal: one pass over the score
map, one thread per cell, no atomics in the classification half); the regression rows are those of the other modes.  focal_terms() below
is the host statement (float64); CPU tensors take it.  LossTotal.last_terms then holds (cls_b, reg_b, |P_b|) per sample.

`loss_sampling: anchor` uses the two anchors of a cell as anchors: every (anchor, cell) pair gets a target of its own by rotated
bird's-eye IoU with the labels (positive from assign_pos_iou, negative below assign_neg_iou, ignored in between, the best anchor of every
label forced positive; assign.py is the host statement, csrc/loss.hip k_assign_* the device's), the focal term runs over the anchors
that are not ignored and the regression over the positive ones (anchor_terms() below; k_loss_anchor).  No windows, nothing drawn.

`iou_loss_gain` > 0 (anchor mode only) adds gain * mean over the positive anchors of (1 - rotated IoU of the decoded box with its label)
per sample: anchor_iou_terms() / iou_value_grad() below are the host statements, csrc/loss_iou.hip the device's (one lane per positive
anchor, compacted in index order; no atomics).  LossTotal.last_iou then holds (mean IoU of the positives, N_b) per sample.

Reference quirks are kept behind `loss_reduction: last` (default): cross-entropy on already
soft-maxed scores (loss.py:17-20,139), 129 negatives (:125), only the last sample of the
batch contributes (:71).  'sum' / 'mean' accumulate over the batch instead.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .model import AnchorBoundingBoxFeature


REDUCTION = {"last": 0, "sum": 1, "mean": 2}       # the kernels' reduction codes (csrc/loss.hip)


class _FusedLoss(torch.autograd.Function):
    """loss = one launch of csrc/loss.hip on the head outputs; the same launch leaves dL/d(head outputs) in dense maps, which
    backward hands to autograd scaled by the incoming gradient.  With `base` = the [B,32,h,w] head tensor that cls / reg are views
    of, the gradient goes straight to it (no slice-backward kernels).  launch(loss, gcls, greg) makes the library call: the list-driven
    entry or one of the sampled ones, with whatever else that entry takes."""

    @staticmethod
    def forward(ctx, base, cls, reg, launch):
        loss = torch.zeros(1, dtype=torch.float32, device=cls.device)
        if base is not None:
            g = torch.zeros_like(base)
            gcls, greg = g, g[:, 4:]
        else:
            g = gcls, greg = torch.zeros_like(cls), torch.zeros_like(reg)
        launch(loss, gcls, greg)
        ctx.g, ctx.split = g, base is None
        return loss

    @staticmethod
    def backward(ctx, go):
        g = ctx.g
        if ctx.split:
            return None, g[0] * go, g[1] * go, None
        return g * go, None, None, None


def pack_lists(samples):
    """The layout dcf_loss_fwd_bwd reads, from per-sample (pos, neg, rows, row_box, row_w, boxes[:, :7]) -- arrays or lists:
    ints (int64)    = B x {off_int, npos, nneg, nrow, off_float, nbox}, then per sample: positive, negative, regression cells, box
                      of each regression cell;
    floats (float32) = per sample: weight of each regression cell, then nbox x 7 box parameters.
    Offsets count from the start of each buffer."""
    B = len(samples)
    head = np.empty((B, 6), np.int64)
    parts_i, parts_f = [head.reshape(-1)], []
    o, of = 6 * B, 0
    for b, (pos, neg, rows, row_box, row_w, boxes) in enumerate(samples):
        pos, neg, rows, row_box = [np.asarray(v, dtype=np.int64) for v in (pos, neg, rows, row_box)]
        row_w, bx = np.asarray(row_w, dtype=np.float32), np.asarray(boxes, dtype=np.float32).reshape(-1)
        head[b] = (o, pos.size, neg.size, rows.size, of, bx.size // 7)
        parts_i += [pos, neg, rows, row_box]
        parts_f += [row_w, bx]
        o += pos.size + neg.size + 2 * rows.size
        of += row_w.size + bx.size
    return np.concatenate(parts_i), np.concatenate(parts_f) if parts_f else np.zeros(0, np.float32)


def _mix64(z):
    """dcf_mix64 of csrc/dcf_common.h on uint64 arrays (numpy wraps modulo 2^64)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_rand(seed, sample, stream, index, attempt=0):
    """dcf_loss_sample_rand for an array of indices: uint32 array (tests/test_cabi.py pins the library's function to the same hash)."""
    idx = np.asarray(index, dtype=np.uint64)
    ctr = np.uint64((sample << 44) | (stream << 40) | (attempt << 20)) | idx
    with np.errstate(over="ignore"):
        return (_mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ _mix64(ctr)) >> np.uint64(32)).astype(np.uint32)


def float_order(d):
    """The order-preserving map from fp32 to uint32 (ord of `loss_sampling: hard`): flips the sign bit of a non-negative float and
    all bits of a negative one, so unsigned comparison of the results follows the order of the floats (-0.0 below +0.0)."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def hard_keys(cls_sample):
    """key(cell) of one sample: cls_sample float32 [4, HW] -> uint32 [HW]; one fp32 subtraction per anchor, the worse anchor counts."""
    c = np.ascontiguousarray(cls_sample, dtype=np.float32)
    k = np.maximum(float_order(c[1] - c[0]), float_order(c[3] - c[2]))
    return np.maximum(k, np.uint32(1))           # (0 marks a window cell on the device; the two keys this moves are NaN patterns)


def hard_negatives(cls_sample, window_cells, neg_count):
    """The host statement of the mined negative list of one sample: the candidates (cells in no positive window) ordered by key
    descending, ties by cell ascending; the first min(neg_count, candidates) of them.  int64 array."""
    keys = hard_keys(cls_sample)
    cand = np.ones(keys.shape[0], dtype=bool)
    if len(window_cells):
        cand[np.asarray(window_cells, dtype=np.int64)] = False
    cells = np.flatnonzero(cand)
    order = np.lexsort((cells, -keys[cells].astype(np.int64)))
    return cells[order[:neg_count]].astype(np.int64)


def parse_focal_config(config):
    """(focal_alpha, focal_gamma, focal_eps) of `loss_sampling: focal`, validated: alpha in (0, 1); gamma 0 or >= 1 (in between,
    (1-p)^(gamma-1) of the gradient is unbounded at p = 1); eps in (0, 1e-3]."""
    alpha, gamma, eps = (config.get("focal_alpha", 0.25), config.get("focal_gamma", 2.0), config.get("focal_eps", 1e-12))
    for key, v in (("focal_alpha", alpha), ("focal_gamma", gamma), ("focal_eps", eps)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError("%s must be a finite number (got %r)" % (key, v))
    if not 0.0 < alpha < 1.0:
        raise ValueError("focal_alpha must lie in (0, 1) (got %r)" % (alpha,))
    if not (gamma == 0 or gamma >= 1.0):
        raise ValueError("focal_gamma must be 0 or >= 1 (got %r)" % (gamma,))
    if not 0.0 < eps <= 1e-3:
        raise ValueError("focal_eps must lie in (0, 1e-3] (got %r)" % (eps,))
    return float(alpha), float(gamma), float(eps)


def focal_terms(cls_b, P_b, alpha, gamma, eps):
    """The host statement of the focal classification term of one sample, in float64: cls_b [4, HW] scores, P_b = the positive
    cells -> (value, gradient [4, HW]).  For anchor a and cell i with y = (i in P_b): p_t = cls_b[2a+y, i], alpha_t = alpha if y else
    1 - alpha, q = eps where p_t < eps else p_t (a NaN stays NaN), FL = -alpha_t (1-q)^gamma ln q; value = sum FL / max(1, |P_b|).
    The gradient is taken at q, also where the clamp acted; the other channel of the pair gets 0."""
    c = np.asarray(cls_b, dtype=np.float64)
    HW = c.shape[1]
    y = np.zeros(HW, dtype=bool)
    cells = sorted(set(int(v) for v in P_b))
    if cells:
        y[np.array(cells, dtype=np.int64)] = True
    inv_n = 1.0 / max(1, len(cells))
    alpha_t = np.where(y, alpha, 1.0 - alpha)
    grad = np.zeros((4, HW), dtype=np.float64)
    value = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(2):
            pt = np.where(y, c[2 * a + 1], c[2 * a])
            q = np.where(pt < eps, eps, pt)
            lnq = np.log(q)
            if gamma == 0:
                fl, g = -alpha_t * lnq, -alpha_t / q
            else:
                om = 1.0 - q
                fl = -alpha_t * om ** gamma * lnq
                g = alpha_t * gamma * om ** (gamma - 1.0) * lnq - alpha_t * om ** gamma / q
            value += fl.sum()
            grad[2 * a + 1] = np.where(y, g, 0.0) * inv_n
            grad[2 * a] = np.where(y, 0.0, g) * inv_n
    return value * inv_n, grad


def anchor_terms(cls_b, reg_b, anchors, boxes, target, alpha, gamma, eps):
    """The host statement of the terms of `loss_sampling: anchor` for one sample, in float64: cls_b [4, HW], reg_b [14, HW], anchors
    [2, 7, HW], boxes [n, >= 7], target int [2 * HW] (label row, -1 negative, -2 ignored; anything else counts as ignored) ->
    (cls value, reg value without the gain, N = positive anchors, d cls value / d cls_b [4, HW], d reg value / d reg_b [14, HW]).
    Classification over the anchors j = a * HW + i with target != -2: y = target >= 0, p_t = cls_b[2a + y, i], the focal term and
    gradient of focal_terms (same clamp), divided by max(1, N).  Regression over the positive anchors: Smooth-L1 of reg_b[7a + c, i]
    minus the encoded offset of box target(j) against anchor (a, i) (the encoding of LossTotal._reg_term), divided by 7 max(1, N)."""
    c, r = np.asarray(cls_b, dtype=np.float64), np.asarray(reg_b, dtype=np.float64)
    an, bx = np.asarray(anchors, dtype=np.float64), np.asarray(boxes, dtype=np.float64).reshape(-1, np.shape(boxes)[-1] if np.ndim(boxes) > 1 else 7)
    HW = c.shape[1]
    t = np.asarray(target, dtype=np.int64).reshape(2, HW).copy()
    t[(t < -2) | (t >= len(bx))] = -2
    n_pos = int((t >= 0).sum())
    inv_n = 1.0 / max(1, n_pos)
    gcls, greg = np.zeros((4, HW)), np.zeros((14, HW))
    cls_value = reg_value = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(2):
            y, used = t[a] >= 0, t[a] != -2
            alpha_t = np.where(y, alpha, 1.0 - alpha)
            pt = np.where(y, c[2 * a + 1], c[2 * a])
            q = np.where(pt < eps, eps, pt)
            lnq = np.log(q)
            if gamma == 0:
                fl, g = -alpha_t * lnq, -alpha_t / q
            else:
                om = 1.0 - q
                fl = -alpha_t * om ** gamma * lnq
                g = alpha_t * gamma * om ** (gamma - 1.0) * lnq - alpha_t * om ** gamma / q
            cls_value += fl[used].sum()
            gcls[2 * a + 1] = np.where(y, g, 0.0) * inv_n
            gcls[2 * a] = np.where(used & ~y, g, 0.0) * inv_n
            cells = np.flatnonzero(y)
            if cells.size:
                A, ref = an[a][:, cells], bx[t[a][cells], :7].T           # [7, m] each
                diag = np.sqrt(A[3] ** 2 + A[4] ** 2)
                dyaw = ref[6] - A[6]
                enc = np.stack(((ref[0] - A[0]) / diag, (ref[1] - A[1]) / diag, (ref[2] - A[2]) / A[5], np.log(ref[3] / A[3]),
                                np.log(ref[4] / A[4]), np.log(ref[5] / A[5]), np.arctan2(np.sin(dyaw), np.cos(dyaw))))
                d = r[7 * a:7 * a + 7][:, cells] - enc
                ad = np.abs(d)
                reg_value += np.where(ad < 1.0, 0.5 * d * d, ad - 0.5).sum()
                greg[7 * a:7 * a + 7, cells] = np.where(ad < 1.0, d, np.sign(d)) * (inv_n / 7.0)
    return cls_value * inv_n, reg_value * (inv_n / 7.0), n_pos, gcls, greg


IOU_KIND = {"3d": 0, "bev": 1}                     # the kernel's kind codes (csrc/loss_iou.hip)


def parse_iou_loss_config(config):
    """(iou_loss_gain, iou_loss_kind), validated: the gain a finite number >= 0 (absent or 0: the term is off), the kind '3d' or 'bev';
    a gain > 0 needs `loss_sampling: anchor` (the term runs over that mode's per-anchor targets; there is no fallback)."""
    from . import cfgcheck
    gain = cfgcheck.number("iou_loss_gain", config.get("iou_loss_gain", 0.0), nonneg=True)
    kind = config.get("iou_loss_kind", "3d")
    if not isinstance(kind, str) or kind not in IOU_KIND:
        raise ValueError("iou_loss_kind must be '3d' or 'bev' (got %r)" % (kind,))
    if gain > 0 and config.get("loss_sampling", "compat") != "anchor":
        raise ValueError("iou_loss_gain > 0 needs loss_sampling: anchor (got loss_sampling: %r)" % (config.get("loss_sampling", "compat"),))
    return gain, kind


def decode_offsets(r, an):
    """The head's box decode (csrc/elementwise.hip, k_head_fwd) in float64, without the yaw wrap: r [7, m] offsets, an [7, m] anchors ->
    (boxes [7, m] = x, y, z, l, w, h, yaw; chain [7, m] = d box_c / d r_c = diag, diag, a5, l, w, h, 1)."""
    r, an = np.asarray(r, dtype=np.float64), np.asarray(an, dtype=np.float64)
    diag = np.sqrt(an[3] ** 2 + an[4] ** 2)
    with np.errstate(over="ignore", invalid="ignore"):
        l, w, h = np.exp(r[3]) * an[3], np.exp(r[4]) * an[4], np.exp(r[5]) * an[5]
        box = np.stack((r[0] * diag + an[0], r[1] * diag + an[1], r[2] * an[5] + an[2], l, w, h, r[6] + an[6]))
    return box, np.stack((diag, diag, an[5], l, w, h, np.ones_like(diag)))


def _rects(x, y, l, w, yaw):
    """evalgeom.bev_rect for arrays: corners [m, 4, 2], counter-clockwise, corner k = (sl, sw)[k] half-sizes along / across the heading."""
    c, s = np.cos(yaw), np.sin(yaw)
    hl, hw = l / 2, w / 2
    out = np.empty(x.shape + (4, 2))
    for k, (sl, sw) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
        out[:, k, 0] = x + sl * hl * c - sw * hw * s
        out[:, k, 1] = y + sl * hl * s + sw * hw * c
    return out


def _edges_inside(P, Q, closed):
    """Every edge k of the rectangles P [m, 4, 2] (corner k to k + 1) clipped parametrically against the four half-planes of Q: (t0, t1)
    [m, 4] each, the piece inside is A + t (B - A) for t in [t0, t1], empty when t1 <= t0.  Strictly left of an edge of Q is inside, the
    side values and the crossing parameter sa / (sa - sb) are those of evalgeom._clip_convex; with `closed` an edge that lies ON a line
    of Q (both side values exactly 0) stays, so that of two coincident edges one is kept (P's) and one dropped (Q's).  A NaN compares
    false everywhere: the edge is empty."""
    A, Bv = P, np.roll(P, -1, axis=1)
    t0, t1 = np.zeros(P.shape[:2]), np.ones(P.shape[:2])
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(4):
            a, b = Q[:, j, None, :], Q[:, (j + 1) % 4, None, :]
            ex, ey = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
            sa = ex * (A[..., 1] - a[..., 1]) - ey * (A[..., 0] - a[..., 0])
            sb = ex * (Bv[..., 1] - a[..., 1]) - ey * (Bv[..., 0] - a[..., 0])
            ina, inb = sa > 0, sb > 0
            t = sa / (sa - sb)
            t1 = np.where(ina & ~inb, np.minimum(t1, t), t1)
            t0 = np.where(inb & ~ina, np.maximum(t0, t), t0)
            out = ~ina & ~inb
            if closed:
                out &= ~((sa == 0) & (sb == 0))
            t1 = np.where(out, -1.0, t1)
    return t0, t1


def iou_value_grad(p, q, kind="3d"):
    """The edge-clip form of the rotated IoU of boxes p [m, 7] against q [m, 7] (x, y, z, l, w, h, yaw; z at mid-height) and its derivative
    by p, in float64: (iou [m], d iou / d p [m, 7]).  This is the arithmetic of csrc/loss_iou.hip; its value agrees with
    evalkitti.iou_pair (the polygon clip) to rounding wherever no edge of one rectangle lies on the line of an edge of the other.

    Coordinates are taken relative to q's centre.  Each of p's edges is clipped in q and each of q's edges in p (_edges_inside); the
    pieces are the boundary of the intersection, so I = half the sum of cross(a, b) over the pieces = half the sum of (t1 - t0) cross(A, B)
    over the edges.  p's edge k has the outward normal n_k = (s, -c), (c, s), (-s, c), (-c, -s) (c, s = cos, sin of p's yaw), length
    len_k = (t1 - t0) times l (k = 0, 2: the sides) or w (k = 1, 3: front and rear) and midpoint m_k:
        dI/dx = sum n_kx len_k, dI/dy = sum n_ky len_k, dI/dyaw = sum len_k (n_ky (m_kx - x) - n_kx (m_ky - y)),
        dI/dl = (len_1 + len_3) / 2, dI/dw = (len_0 + len_2) / 2.
    zo = max(0, min(tops) - max(bottoms)); d zo/dz = [p's top is the lower] - [p's bottom is the higher], d zo/dh = half their sum, both 0
    when zo = 0.  I3 = I zo, U = l w h + V_q - I3, d iou = (dI3 U - I3 dU) / U^2 with dU = d(l w h) - dI3; 'bev': zo = 1 and areas for
    volumes.  A disjoint pair has iou 0 and seven exact zeros; a row with a non-finite p or q has NaN everywhere."""
    if kind not in IOU_KIND:
        raise ValueError("kind must be '3d' or 'bev' (got %r)" % (kind,))
    p, q = np.asarray(p, dtype=np.float64).reshape(-1, 7), np.asarray(q, dtype=np.float64).reshape(-1, 7)
    m = p.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x, y = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1]
        l, w, h, yaw = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
        c, s = np.cos(yaw), np.sin(yaw)
        P, Q = _rects(x, y, l, w, yaw), _rects(np.zeros(m), np.zeros(m), q[:, 3], q[:, 4], q[:, 6])
        cross = lambda R: R[:, :, 0] * np.roll(R, -1, axis=1)[:, :, 1] - R[:, :, 1] * np.roll(R, -1, axis=1)[:, :, 0]
        pt0, pt1 = _edges_inside(P, Q, closed=True)
        qt0, qt1 = _edges_inside(Q, P, closed=False)
        pd, qd = np.maximum(0.0, pt1 - pt0), np.maximum(0.0, qt1 - qt0)
        I = 0.5 * ((pd * cross(P)).sum(1) + (qd * cross(Q)).sum(1))
        length = pd * np.stack((l, w, l, w), 1)
        tm = 0.5 * (pt0 + pt1)[..., None]
        mid = P + tm * (np.roll(P, -1, axis=1) - P)                       # [m, 4, 2]
        nx, ny = np.stack((s, c, -s, -c), 1), np.stack((-c, s, c, -s), 1)
        dI = np.zeros((m, 7))
        dI[:, 0], dI[:, 1] = (nx * length).sum(1), (ny * length).sum(1)
        dI[:, 3], dI[:, 4] = 0.5 * (length[:, 1] + length[:, 3]), 0.5 * (length[:, 0] + length[:, 2])
        dI[:, 6] = (length * (ny * (mid[:, :, 0] - x[:, None]) - nx * (mid[:, :, 1] - y[:, None]))).sum(1)
        dS = np.zeros((m, 7))                                             # d (l w) or d (l w h)
        if kind == "bev":
            zo, dzo = np.ones(m), np.zeros((m, 7))
            size, vq = l * w, q[:, 3] * q[:, 4]
            dS[:, 3], dS[:, 4] = w, l
        else:
            top_p, bot_p, top_q, bot_q = p[:, 2] + h / 2, p[:, 2] - h / 2, q[:, 2] + q[:, 5] / 2, q[:, 2] - q[:, 5] / 2
            zo = np.maximum(0.0, np.minimum(top_p, top_q) - np.maximum(bot_p, bot_q))
            lower_top, higher_bot = ((top_p < top_q) & (zo > 0)).astype(np.float64), ((bot_p > bot_q) & (zo > 0)).astype(np.float64)
            dzo = np.zeros((m, 7))
            dzo[:, 2], dzo[:, 5] = lower_top - higher_bot, 0.5 * (lower_top + higher_bot)
            size, vq = l * w * h, q[:, 3] * q[:, 4] * q[:, 5]
            dS[:, 3], dS[:, 4], dS[:, 5] = w * h, l * h, l * w
        I3 = I * zo
        dI3 = dI * zo[:, None] + I[:, None] * dzo
        U = size + vq - I3
        iou = I3 / U
        grad = (dI3 * U[:, None] - I3[:, None] * (dS - dI3)) / (U * U)[:, None]
    bad = ~(np.isfinite(p).all(1) & np.isfinite(q).all(1))
    iou[bad], grad[bad] = np.nan, np.nan
    return iou, grad


def anchor_iou_terms(reg_b, anchors, boxes, target, kind="3d"):
    """The host statement of the IoU regression term (`iou_loss_gain`) for one sample, in float64: reg_b [14, HW],
    anchors [2, 7, HW], boxes [n, >= 7], target int [2 * HW] as in anchor_terms -> (L = sum over the positive anchors of (1 - IoU(p_j, q_j))
    / max(1, N), N, the sum of the IoUs, d L / d reg_b [14, HW], the per-anchor IoU [2, HW], 0 where the anchor is not positive).
    q_j = the label row target(j); p_j = decode_offsets of the anchor's seven offsets.  The VALUE of every IoU is
    evalkitti.iou_pair(p, q)[1] ('3d') or [0] ('bev') itself; the derivative is iou_value_grad's, chained to the offsets."""
    from . import evalkitti
    if kind not in IOU_KIND:
        raise ValueError("kind must be '3d' or 'bev' (got %r)" % (kind,))
    r, an = np.asarray(reg_b, dtype=np.float64), np.asarray(anchors, dtype=np.float64)
    bx = np.asarray(boxes, dtype=np.float64).reshape(-1, np.shape(boxes)[-1] if np.ndim(boxes) > 1 else 7)
    HW = r.shape[1]
    t = np.asarray(target, dtype=np.int64).reshape(2, HW).copy()
    t[(t < -2) | (t >= len(bx))] = -2
    n_pos = int((t >= 0).sum())
    inv_n = 1.0 / max(1, n_pos)
    grad, iou_map = np.zeros((14, HW)), np.zeros((2, HW))
    value = total = 0.0
    for a in range(2):
        cells = np.flatnonzero(t[a] >= 0)
        if not cells.size:
            continue
        p, chain = decode_offsets(r[7 * a:7 * a + 7][:, cells], an[a][:, cells])
        q = bx[t[a][cells], :7]
        _, g = iou_value_grad(p.T, q, kind)
        iou = np.array([evalkitti.iou_pair(p[:, i], q[i])[0 if kind == "bev" else 1] for i in range(cells.size)])
        iou[~(np.isfinite(p).all(0) & np.isfinite(q).all(1))] = np.nan
        with np.errstate(invalid="ignore"):
            value += (1.0 - iou).sum()
            total += iou.sum()
            grad[7 * a:7 * a + 7, cells] = -(g.T * chain) * inv_n
        iou_map[a, cells] = iou
    return value * inv_n, n_pos, total, grad, iou_map


class LossTotal(nn.Module):
    def __init__(self, config):
        super(LossTotal, self).__init__()
        self.config = config
        self.regress_type = config["regress_type"]
        self.reduction = config.get("loss_reduction", "last")
        self.sampling = config.get("loss_sampling", "compat")
        if self.sampling not in ("compat", "device", "hard", "focal", "anchor"):
            raise ValueError("loss_sampling must be compat, device, hard, focal or anchor (got %r)" % (self.sampling,))
        self.focal = parse_focal_config(config) if self.sampling in ("focal", "anchor") else None      # (alpha, gamma, eps)
        self.assign_iou = None             # anchor: (assign_pos_iou, assign_neg_iou)
        if self.sampling == "anchor":
            from .assign import parse_assign_config
            self.assign_iou = parse_assign_config(config)
        self.iou_gain, self.iou_kind = parse_iou_loss_config(config)      # the rotated-IoU regression term (anchor only; 0: off)
        self.last_iou = None               # iou_loss_gain > 0: [B,2] fp32 = (mean IoU of the positive anchors, N_b) of the last call
        self.last_terms = None             # focal: [B,3] fp32 = (cls_b, reg_b without the gain, |P_b|) of the last call, unweighted
                                           # (anchor: the third column is N_b, the positive anchors)
        from .model import parse_deterministic_config
        self.deterministic = parse_deterministic_config(config)      # both device entries then sum in one fixed order (csrc/loss.hip, DET)
        self.seed = int(config.get("loss_seed", 0))
        self.calls = 0                     # device sampling: the call count enters the hash, so every step draws fresh lists
                                           # (saved with the checkpoint: Train.save_checkpoint / load_checkpoint)
        self.last_samples = None           # device sampling with keep_samples: (pos [B,cap], neg [B,n], counts [B,2]) of the last call
                                           # (hard: counts [B,3] = selected positives, window entries, selected negatives; neg -1 padded)
        self.keep_samples = False
        anc = AnchorBoundingBoxFeature(config)()
        self.register_buffer("anchor_set", anc.reshape(2, 7, anc.shape[1], anc.shape[2]), persistent=False)
        if self.sampling == "anchor" and not bool((torch.isfinite(self.anchor_set[:, [0, 1, 3, 4, 6]]).all() and (self.anchor_set[:, 3:5] > 0).all())):
            raise ValueError("loss_sampling: anchor needs finite anchors of positive length and width (an IoU against a zero-area anchor is undefined)")
        L, W = config["voxel_length"], config["voxel_width"]
        self._xs = int(L / (config["lidar_x_max"] - config["lidar_x_min"]))
        self._ys = int(W / (config["lidar_y_max"] - config["lidar_y_min"]))
        self._xo = int(-config["lidar_x_min"] * self._xs)
        self._yo = int(-config["lidar_y_min"] * self._ys)

    # ------------------------------------------------------------------ host-side sampling
    def assign(self, boxes, H, W):
        """Positive window / negative sampling of loss.py:74-127 for one sample (boxes: [n,>=2] CPU)."""
        c = self.config
        rs = c["anchor_bbox_feature"]["reduced_scale"]
        span = c["positive_range"]
        half = int(span / 2)
        positives, regress, owner = [], [], []
        centres = boxes[:, :2].tolist() if hasattr(boxes, "tolist") else [(float(b[0]), float(b[1])) for b in boxes]
        f32 = np.float32
        for bx, by in centres:
            members = []
            # the reference does this arithmetic on 0-dim fp32 tensors (loss.py:85-86): one fp32 rounding per operation, then
            # truncation -- in double precision a centre within fp32 rounding of a cell boundary lands one cell lower
            cx = int((f32(bx) * f32(self._xs) + f32(self._xo)) / f32(rs))
            cy = int((f32(by) * f32(self._ys) + f32(self._yo)) / f32(rs))
            if 0 <= cx <= H - 1 and 0 <= cy <= W - 1:
                for dx in range(span):
                    for dy in range(span):
                        px, py = cx - half + dx, cy - half + dy
                        if px < 0 or px > H - 1 or py < 0 or py > W - 1:
                            continue
                        positives.append([px, py])
                        if self.regress_type == 0 or (px == cx and py == cy):
                            members.append(len(regress))
                            regress.append([px, py])
            owner.append(members)
        np.random.shuffle(positives)
        positives = positives[:c["pos_sample_threshold"]] if len(positives) > c["pos_sample_threshold"] else positives
        # same draws and the same rejections as the reference's `[x, y] in list` test (loss.py:117-126), with a set lookup
        taken = set((p[0], p[1]) for p in positives)
        # ... and drawn in batches: randint([H, W], size=(m, 2)) consumes the legacy generator exactly like m pairs of
        # scalar calls (checked in tests/test_host_logic.py); a batch never holds more pairs than are still missing, so
        # no draw goes unused and the stream stays where the reference's loop leaves it
        negatives = []
        want = c["neg_sample_threshold"] + 1
        while len(negatives) < want:
            for x, y in np.random.randint([H, W], size=(want - len(negatives), 2)).tolist():
                if (x, y) not in taken:
                    negatives.append([x, y])
        return positives, negatives, regress, owner

    def windows(self, boxes, H, W):
        """The positive windows of one sample, no randomness: (window entries as cell codes px * W + py in the reference's order --
        box, dx, dy; overlapping windows give a cell twice --, regression cells, box of each, weight of each).  boxes: float32
        ndarray [n, >= 2]."""
        c = self.config
        rs, span = c["anchor_bbox_feature"]["reduced_scale"], c["positive_range"]
        half = int(span / 2)
        f32 = np.float32
        nb = len(boxes)
        # loss.py:85-86 on fp32 scalars: one rounding per operation, then truncation toward zero
        if nb:
            cxs = ((boxes[:, 0] * f32(self._xs) + f32(self._xo)) / f32(rs)).astype(np.int64).tolist()
            cys = ((boxes[:, 1] * f32(self._ys) + f32(self._yo)) / f32(rs)).astype(np.int64).tolist()
        else:
            cxs = cys = []
        cells, rows, row_box, row_w = [], [], [], []
        centre_only = self.regress_type != 0
        for k in range(nb):
            cx, cy = cxs[k], cys[k]
            if cx < 0 or cx > H - 1 or cy < 0 or cy > W - 1:
                continue
            x0, x1 = max(cx - half, 0), min(cx - half + span - 1, H - 1)
            y0, y1 = max(cy - half, 0), min(cy - half + span - 1, W - 1)
            win = [px * W + py for px in range(x0, x1 + 1) for py in range(y0, y1 + 1)]      # the reference's order: dx, then dy
            cells += win
            if centre_only:
                rows.append(cx * W + cy); row_box.append(k); row_w.append(1.0 / 14)
            else:
                rows += win
                row_box += [k] * len(win)
                row_w += [1.0 / (len(win) * 14)] * len(win)
        return cells, rows, row_box, row_w

    def assign_arrays(self, boxes, H, W):
        """assign() for the hot path: the same lists as flat integer codes (cell = px * W + py) -- (positive cells, negative cells,
        regression cells, box of each regression cell, weight of each regression cell) -- with the same consumption of numpy's
        legacy generator: RandomState.shuffle draws the same random_interval sequence for a 1-D array of n codes as for a list
        of n pairs (and takes its C fast path there), the negatives are drawn in the same batches.  tests/test_host_logic.py
        pins lists and generator state to assign().  boxes: float32 ndarray [n, >= 2]."""
        c = self.config
        cap = c["pos_sample_threshold"]
        cells, rows, row_box, row_w = self.windows(boxes, H, W)
        pos = np.array(cells, dtype=np.int64)
        np.random.shuffle(pos)
        pos = pos[:cap]
        taken = set(pos.tolist())
        want = c["neg_sample_threshold"] + 1
        neg = []
        while len(neg) < want:
            dr = np.random.randint([H, W], size=(want - len(neg), 2))
            for code in (dr[:, 0] * W + dr[:, 1]).tolist():
                if code not in taken:
                    neg.append(code)
        return pos, np.array(neg, dtype=np.int64), np.array(rows, dtype=np.int64), np.array(row_box, dtype=np.int64), np.array(row_w, dtype=np.float32)

    # ------------------------------------------------------------------ device-side terms
    def _step_seed(self):
        """The seed of this call's hash streams, and the call counted.  Rank 0 / a single process: (seed, calls); other
        data-parallel ranks draw from streams of their own."""
        rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        seed = (self.seed * 0x9E3779B1 + self.calls + rank * 0x85EBCA77C2B2AE63) & 0xFFFFFFFFFFFFFFFF
        self.calls += 1
        return seed

    def _stage(self, ints, floats, dev):
        """The packed lists (numpy) as tensors on dev.  CUDA: through pinned buffers, all index lists / boxes of the step in two
        async copies.  A ring of three buffer pairs: the one being refilled was last used three steps ago, so the wait for its
        copies never blocks -- with a single pair the host stalled here every step until the GPU had reached the previous step's
        loss (the host enqueues a step about as fast as the GPU runs it, so that wait set the pace)."""
        if dev.type != "cuda":
            return torch.from_numpy(ints), torch.from_numpy(floats)
        ni, nf = max(ints.size, 1), max(floats.size, 1)
        ring = getattr(self, "_stage_ring", None)
        if ring is None or ring[0][0].numel() < ni or ring[0][1].numel() < nf:
            ring = []
            for _ in range(3):
                a, b = torch.empty(max(ni, 1 << 16), dtype=torch.long).pin_memory(), torch.empty(max(nf, 1 << 12), dtype=torch.float32).pin_memory()
                ring.append([a, b, None, a.numpy(), b.numpy()])
            self._stage_ring, self._stage_slot = ring, 0
        st = ring[self._stage_slot]
        self._stage_slot = (self._stage_slot + 1) % len(ring)
        if st[2] is not None:
            st[2].synchronize()
        st[3][:ints.size] = ints
        st[4][:floats.size] = floats
        di = st[0][:ni].to(dev, non_blocking=True)
        df = st[1][:nf].to(dev, non_blocking=True)
        st[2] = torch.cuda.Event()
        st[2].record()
        return di, df

    def _forward_lists(self, cls, reg, anc, samples, B, H, W):
        """The terms on per-sample lists (pack_lists): one launch of dcf_loss_fwd_bwd for CUDA tensors, torch ops for CPU tensors."""
        di, df = self._stage(*pack_lists(samples), cls.device)
        if cls.device.type != "cuda":
            return self._terms_host(cls, reg, anc, di, df, B, H, W)
        from . import _hip as Hl
        base, cls, reg = self._head_views(cls, reg, H, W)
        gain, red = float(self.config["regress_loss_gain"]), REDUCTION[self.reduction]

        def launch(loss, gcls, greg):
            args = (cls, cls.stride(0), reg, reg.stride(0), anc, di, df, B, H * W, gain, red, loss, gcls, gcls.stride(0), greg, greg.stride(0))
            if self.deterministic:   # duplicate cells summed in list order, the samples' values added in sample order
                Hl.call("dcf_loss_fwd_bwd_det", *args, torch.empty(B, dtype=torch.float32, device=cls.device), Hl.stream_ptr())
            else:
                Hl.call("dcf_loss_fwd_bwd", *args, Hl.stream_ptr())
        return _FusedLoss.apply(base, cls, reg, launch)

    def _forward_hip(self, cls, reg, anc, ints, floats, plan, B, H, W):
        """Device half as one launch on explicit lists: plan = per sample (off_int, npos, nneg, nrow, off_float, nbox), offsets into
        ints (positive, negative, regression cells, box of each regression cell) and floats (weights, nbox x 7 box parameters)."""
        ints, floats = np.asarray(ints, dtype=np.int64), np.asarray(floats, dtype=np.float32)
        samples = []
        for (o, npos, nneg, nrow, of, nb) in plan:
            cuts = np.cumsum([o, npos, nneg, nrow, nrow])
            samples.append(tuple(ints[i:j] for i, j in zip(cuts[:-1], cuts[1:])) + (floats[of:of + nrow], floats[of + nrow:of + nrow + 7 * nb]))
        return self._forward_lists(cls, reg, anc, samples, B, H, W)

    def _forward_hip_arrays(self, cls, reg, anc, boxes_host, nbox, B, H, W):
        """The CUDA path of the compat mode: numpy target assignment (assign_arrays), no Python lists of cells."""
        bh = boxes_host.numpy() if boxes_host.dtype == torch.float32 else boxes_host.float().numpy()
        samples = []
        for b in range(B):
            nb = int(nbox[b])
            samples.append(self.assign_arrays(bh[b, :nb], H, W) + (bh[b, :nb, :7],))
        return self._forward_lists(cls, reg, anc, samples, B, H, W)

    @staticmethod
    def _head_views(cls, reg, H, W):
        """(base, cls, reg): base = the contiguous [B,>=18,h,w] head tensor cls / reg are views of (the gradient then goes straight
        to it), or None."""
        HW = H * W
        ok = lambda t, c: t.dtype == torch.float32 and t.stride(1) == HW and t.stride(2) == W and t.stride(3) == 1 and t.shape[1] == c
        if not ok(cls, 4):
            cls = cls.float().contiguous()
        if not ok(reg, 14):
            reg = reg.float().contiguous()
        base = cls._base
        if not (base is not None and reg._base is base and base.dim() == 4 and base.is_contiguous() and base.shape[1] >= 18
                and cls.data_ptr() == base.data_ptr() and reg.data_ptr() == base.data_ptr() + 4 * HW * 4 and base.requires_grad):
            base = None
        return base, cls, reg

    def _stage_labels(self, boxes, nbox, dev):
        """The labels on the device: [B,max,9] fp32 and the counts (int32), one small asynchronous copy each when they arrive on the host."""
        if not boxes.is_cuda:
            ring = getattr(self, "_box_ring", None)
            if ring is None or ring[0][0].shape != boxes.shape:
                ring = self._box_ring = [[torch.empty(boxes.shape, dtype=torch.float32).pin_memory(), None] for _ in range(3)]
                self._box_slot = 0
            st = ring[self._box_slot]            # last used three steps ago: the wait below never blocks
            self._box_slot = (self._box_slot + 1) % 3
            if st[1] is not None:
                st[1].synchronize()
            st[0].copy_(boxes)
            boxes = st[0].to(dev, non_blocking=True)
            st[1] = torch.cuda.Event()
            st[1].record()
        else:
            boxes = boxes.float().contiguous()
        nb = nbox.to(device=dev, dtype=torch.int32, non_blocking=True) if torch.is_tensor(nbox) else torch.tensor([int(v) for v in nbox], dtype=torch.int32, device=dev)
        return boxes, nb

    def _forward_device_sampling(self, boxes, nbox, cls, reg, anc, B, H, W):
        c = self.config
        dev = cls.device
        boxes, nb = self._stage_labels(boxes, nbox, dev)
        base, cls, reg = self._head_views(cls, reg, H, W)
        span, pos_cap, neg_count = c["positive_range"], c["pos_sample_threshold"], c["neg_sample_threshold"] + 1
        rs, gain, red = c["anchor_bbox_feature"]["reduced_scale"], c["regress_loss_gain"], REDUCTION[self.reduction]
        hard = self.sampling == "hard"
        outs = (None, None, None)
        if self.keep_samples:
            outs = (torch.empty((B, pos_cap), dtype=torch.int32, device=dev), torch.empty((B, neg_count), dtype=torch.int32, device=dev),
                    torch.empty((B, 3 if hard else 2), dtype=torch.int32, device=dev))
            self.last_samples = outs
        seed = self._step_seed()
        from . import _hip as Hl
        tail = ()
        if hard:
            # the selection's workspace: allocated once per map shape, contents free between calls (all calls go onto one stream)
            ws = getattr(self, "_hard_ws", None)
            if ws is None or ws[0] != (B, H, W, dev):
                nbytes = Hl.lib().dcf_loss_hard_workspace_bytes(B, H, W)
                ws = self._hard_ws = ((B, H, W, dev), torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=dev))
            tail = (ws[1],)
        name = ("dcf_loss_hard_fwd_bwd" if hard else "dcf_loss_sample_fwd_bwd") + ("_det" if self.deterministic else "")

        def launch(loss, gcls, greg):
            rows = (torch.empty(B, dtype=torch.float32, device=dev),) if self.deterministic else ()
            Hl.call(name, cls, cls.stride(0), reg, reg.stride(0), anc, boxes, nb, boxes.shape[1], boxes.shape[2], B, H, W,
                    float(self._xs), float(self._xo), float(self._ys), float(self._yo), float(rs), int(span), int(self.regress_type),
                    int(pos_cap), int(neg_count), int(seed), float(gain), red, loss, gcls, gcls.stride(0), greg, greg.stride(0),
                    *outs, *tail, *rows, Hl.stream_ptr())
        return _FusedLoss.apply(base, cls, reg, launch)

    def _forward_hard_host(self, boxes_host, nbox, cls, reg, anc, B, H, W):
        """loss_sampling: hard on CPU tensors -- the host statement of what the device entry does: windows and positive subset with the
        device sampler's hash (stream 1, the pos_sample_threshold smallest (key, entry) pairs, in entry order), negatives from
        hard_negatives(), the terms through the torch path of the compat mode."""
        c = self.config
        cap, want = c["pos_sample_threshold"], c["neg_sample_threshold"] + 1
        seed = self._step_seed()
        bh = boxes_host.float().numpy()
        scores = cls.detach().float().reshape(B, 4, H * W).numpy()
        samples, kept = [], []
        for b in range(B):
            nb = min(int(nbox[b]), bh.shape[1])
            entries, rows, row_box, row_w = self.windows(bh[b, :nb], H, W)
            if len(entries) > cap:
                keys = sample_rand(seed, b, 1, np.arange(len(entries)))
                chosen = np.sort(np.lexsort((np.arange(len(entries)), keys))[:cap])
                pos = [entries[i] for i in chosen.tolist()]
            else:
                pos = list(entries)
            neg = hard_negatives(scores[b], entries, want).tolist()
            kept.append((pos, neg, len(entries)))
            samples.append((pos, neg, rows, row_box, row_w, bh[b, :nb, :7]))
        if self.keep_samples:
            pos_t, neg_t = torch.full((B, cap), -1, dtype=torch.int32), torch.full((B, want), -1, dtype=torch.int32)
            counts = torch.zeros((B, 3), dtype=torch.int32)
            for b, (pos, neg, n_entries) in enumerate(kept):
                pos_t[b, :len(pos)] = torch.tensor(pos, dtype=torch.int32)
                neg_t[b, :len(neg)] = torch.tensor(neg, dtype=torch.int32)
                counts[b] = torch.tensor([len(pos), n_entries, len(neg)], dtype=torch.int32)
            self.last_samples = (pos_t, neg_t, counts)
        return self._forward_lists(cls, reg, anc, samples, B, H, W)

    def _forward_focal(self, boxes, nbox, cls, reg, anc, B, H, W):
        """loss_sampling: focal.  CUDA tensors: one launch of dcf_loss_focal_fwd_bwd(_det).  CPU tensors: the host statement
        (focal_terms + the torch regression term) behind the same autograd function.  Nothing is drawn: calls is not advanced."""
        c = self.config
        dev = cls.device
        alpha, gamma, eps = self.focal
        gain, red = float(c["regress_loss_gain"]), REDUCTION[self.reduction]
        ws = getattr(self, "_focal_ws", None)           # scratch and terms: allocated once per map shape
        if dev.type != "cuda":
            boxes_host = boxes.detach().float()
            if ws is None or ws[0] != (B, H, W, dev):
                ws = self._focal_ws = ((B, H, W, dev), None, torch.zeros((B, 3), dtype=torch.float32))
            self.last_terms = terms = ws[2]

            def launch(loss, gcls, greg):
                self._focal_host(boxes_host, nbox, cls.detach(), reg.detach(), anc, B, H, W, loss, gcls, greg, terms)
            return _FusedLoss.apply(None, cls, reg, launch)
        from . import ops
        boxes, nb = self._stage_labels(boxes, nbox, dev)
        base, cls, reg = self._head_views(cls, reg, H, W)
        if ws is None or ws[0] != (B, H, W, dev):
            ws = self._focal_ws = ((B, H, W, dev),) + ops.loss_focal_workspace(B, H, W, dev)
        self.last_terms = terms = ws[2]
        grid = (self._xs, self._xo, self._ys, self._yo, c["anchor_bbox_feature"]["reduced_scale"])

        def launch(loss, gcls, greg):
            ops.loss_focal(cls, reg, anc, boxes, nb, grid, c["positive_range"], self.regress_type, alpha, gamma, eps, gain, red,
                           loss, gcls, greg, terms, ws[1], deterministic=self.deterministic)
        return _FusedLoss.apply(base, cls, reg, launch)

    def _focal_host(self, boxes_host, nbox, cls, reg, anc, B, H, W, loss, gcls, greg, terms):
        """The host statement of the focal entry: fills loss [1], the gradient maps and terms [B,3] (float64 arithmetic for the
        classification term, the torch regression term of the other modes and its autograd gradient)."""
        alpha, gamma, eps = self.focal
        gain = float(self.config["regress_loss_gain"])
        bh = boxes_host.numpy()
        terms.zero_()
        total = 0.0
        counted = [B - 1] if self.reduction == "last" else list(range(B))
        w = 1.0 / B if self.reduction == "mean" else 1.0
        for b in counted:
            nb = max(min(int(nbox[b]), bh.shape[1]), 0)
            cells, rows, row_box, row_w = self.windows(bh[b, :nb], H, W)
            value, grad = focal_terms(cls[b].reshape(4, H * W).double().numpy(), cells, alpha, gamma, eps)
            gcls[b] = torch.from_numpy(grad * w).to(gcls.dtype).reshape(4, H, W)
            lr = 0.0
            if rows:
                with torch.enable_grad():
                    rb = reg[b].clone().requires_grad_(True)
                    term = self._reg_term(rb, anc, torch.tensor(rows, dtype=torch.long), torch.tensor(row_box, dtype=torch.long),
                                          torch.tensor(row_w, dtype=torch.float32), torch.from_numpy(bh[b, :nb, :7]), H, W)
                    greg[b] = torch.autograd.grad(term, rb)[0] * (gain * w)
                lr = term.item()
            terms[b] = torch.tensor([value, lr, len(set(cells))], dtype=torch.float32)
            total += w * (value + gain * lr)
        loss[0] = total

    def _forward_anchor(self, boxes, nbox, cls, reg, anc, B, H, W):
        """loss_sampling: anchor.  CUDA tensors: dcf_assign_anchors_iou on the staged labels, then dcf_loss_anchor_fwd_bwd on its
        targets -- five small launches on one stream, no host wait; workspaces, target and counts are allocated once per map shape.
        CPU tensors: the host statements (assign.anchor_targets, anchor_terms) behind the same autograd function.  Nothing is drawn:
        calls is not advanced.  With keep_samples, last_samples = (target [B,2,HW], best [B,2,HW] fp64, counts [B,4]).
        With iou_loss_gain > 0, dcf_loss_anchor_iou_fwd_bwd follows in the same closure (its workspaces are allocated with the others,
        and only then); last_iou = [B,2] (mean IoU of the positives, N_b), and last_samples gains the per-anchor fp64 IoU map."""
        c = self.config
        dev = cls.device
        alpha, gamma, eps = self.focal
        pos_iou, neg_iou = self.assign_iou
        gain, red = float(c["regress_loss_gain"]), REDUCTION[self.reduction]
        ws = getattr(self, "_anchor_ws", None)          # scratch, target, counts and terms: allocated once per map shape
        key = (B, H, W, boxes.shape[1], dev, bool(self.keep_samples))
        if dev.type != "cuda":
            boxes_host = boxes.detach().float()
            if ws is None or ws[0] != key:
                ws = self._anchor_ws = (key, torch.zeros((B, 3), dtype=torch.float32), torch.zeros((B, 2), dtype=torch.float32) if self.iou_gain > 0 else None)
            self.last_terms = terms = ws[1]
            self.last_iou = iou_terms = ws[2]

            def launch(loss, gcls, greg):
                self._anchor_host(boxes_host, nbox, cls.detach(), reg.detach(), anc, B, H, W, loss, gcls, greg, terms, iou_terms)
            return _FusedLoss.apply(None, cls, reg, launch)
        from . import ops
        boxes, nb = self._stage_labels(boxes, nbox, dev)
        base, cls, reg = self._head_views(cls, reg, H, W)
        if ws is None or ws[0] != key:
            ws = self._anchor_ws = ((key,) + ops.assign_anchors_workspace(B, H, W, boxes.shape[1], dev, best=self.keep_samples)
                                    + ops.loss_anchor_workspace(B, H, W, dev)
                                    + (ops.loss_anchor_iou_workspace(B, H, W, dev, iou_map=self.keep_samples) if self.iou_gain > 0 else (None, None, None)))
        _, aws, target, counts, best, lws, terms, iws, iou_terms, iou_map = ws
        self.last_terms, self.last_iou = terms, iou_terms
        if self.keep_samples:
            self.last_samples = (target, best, counts) + ((iou_map,) if self.iou_gain > 0 else ())
        iou_gain, iou_kind = self.iou_gain, IOU_KIND[self.iou_kind]

        def launch(loss, gcls, greg):
            ops.assign_anchors_iou(anc, boxes, nb, H, W, pos_iou, neg_iou, target, counts, aws, best=best)
            ops.loss_anchor(cls, reg, anc, boxes, target, counts, alpha, gamma, eps, gain, red, loss, gcls, greg, terms, lws)
            if iou_gain > 0:
                ops.loss_anchor_iou(reg, anc, boxes, target, counts, iou_kind, iou_gain, red, loss, greg, iou_terms, iws, iou_map=iou_map)
        return _FusedLoss.apply(base, cls, reg, launch)

    def _anchor_host(self, boxes_host, nbox, cls, reg, anc, B, H, W, loss, gcls, greg, terms, iou_terms=None):
        """The host statement of the anchor entries: fills loss [1], the gradient maps and terms [B,3] in float64 arithmetic.  The
        device assigns every sample; here only those the reduction counts, unless keep_samples asks for all.  With iou_loss_gain > 0
        anchor_iou_terms adds the IoU term, fills iou_terms [B,2], and last_samples gains the per-anchor IoU map."""
        from . import assign
        alpha, gamma, eps = self.focal
        pos_iou, neg_iou = self.assign_iou
        gain = float(self.config["regress_loss_gain"])
        bh, an = boxes_host.numpy(), anc.detach().float().numpy()
        HW = H * W
        terms.zero_()
        total = 0.0
        counted = [B - 1] if self.reduction == "last" else list(range(B))
        w = 1.0 / B if self.reduction == "mean" else 1.0
        kept = (np.full((B, 2, HW), -1, np.int32), np.zeros((B, 2, HW)), np.zeros((B, 4), np.int32)) if self.keep_samples else None
        iou_on = self.iou_gain > 0
        if iou_on:
            iou_terms.zero_()
            if kept is not None:
                kept = kept + (np.zeros((B, 2, HW)),)
        for b in (range(B) if kept is not None else counted):
            nb = max(min(int(nbox[b]), bh.shape[1]), 0)
            target, best, counts = assign.anchor_targets(an, bh[b, :nb], pos_iou, neg_iou)
            if kept is not None:
                kept[0][b], kept[1][b], kept[2][b] = target.reshape(2, HW), best.reshape(2, HW), counts
            if b not in counted:
                continue
            lc, lr, n_pos, gc, gr = anchor_terms(cls[b].reshape(4, HW).double().numpy(), reg[b].reshape(14, HW).double().numpy(), an,
                                                 bh[b, :nb], target, alpha, gamma, eps)
            gr = gr * (gain * w)
            total += w * (lc + gain * lr)
            if iou_on:
                li, _, iou_sum, gi, iou_map = anchor_iou_terms(reg[b].reshape(14, HW).double().numpy(), an, bh[b, :nb], target, self.iou_kind)
                gr = gr + gi * (self.iou_gain * w)
                total += w * self.iou_gain * li
                iou_terms[b] = torch.tensor([iou_sum / max(1, n_pos), n_pos], dtype=torch.float32)
                if kept is not None:
                    kept[3][b] = iou_map
            gcls[b] = torch.from_numpy(gc * w).to(gcls.dtype).reshape(4, H, W)
            greg[b] = torch.from_numpy(gr).to(greg.dtype).reshape(14, H, W)
            terms[b] = torch.tensor([lc, lr, n_pos], dtype=torch.float32)
        if kept is not None:
            self.last_samples = tuple(torch.from_numpy(v) for v in kept)
        loss[0] = total

    def forward(self, reference_bboxes_batch, num_ref_bbox_batch, predicted_class_feature_batch, predicted_regress_feature_batch):
        cls, reg = predicted_class_feature_batch, predicted_regress_feature_batch
        dev = cls.device
        B = reference_bboxes_batch.shape[0]
        H, W = cls.shape[-2:]
        if getattr(self, "_anc_dev", None) is None or self._anc_dev.device != dev:
            self._anc_dev = self.anchor_set.to(dev).reshape(2, 7, H * W)
        anc = self._anc_dev
        if self.sampling == "focal":
            return self._forward_focal(reference_bboxes_batch, num_ref_bbox_batch, cls, reg, anc, B, H, W)
        if self.sampling == "anchor":
            return self._forward_anchor(reference_bboxes_batch, num_ref_bbox_batch, cls, reg, anc, B, H, W)
        if self.sampling == "device" or (self.sampling == "hard" and dev.type == "cuda"):
            if dev.type != "cuda":
                raise RuntimeError("loss_sampling: device needs CUDA tensors (the host path is loss_sampling: compat)")
            return self._forward_device_sampling(reference_bboxes_batch, num_ref_bbox_batch, cls, reg, anc, B, H, W)
        # pass CPU boxes (what a DataLoader yields) to avoid a device round trip
        boxes_host = reference_bboxes_batch.detach().cpu() if reference_bboxes_batch.is_cuda else reference_bboxes_batch.detach()
        if self.sampling == "hard":
            return self._forward_hard_host(boxes_host, num_ref_bbox_batch, cls, reg, anc, B, H, W)
        if dev.type == "cuda":
            return self._forward_hip_arrays(cls, reg, anc, boxes_host, num_ref_bbox_batch, B, H, W)
        # ---- host: target assignment for every sample (assign(): the reference's lists and its order of generator draws)
        samples = []
        for b in range(B):
            nb = int(num_ref_bbox_batch[b])
            pos, neg, regress, owner = self.assign(boxes_host[b, :nb], H, W)
            rows, row_box, row_w = [], [], []
            for k in range(nb):
                for m in owner[k]:
                    rows.append(regress[m][0] * W + regress[m][1])
                    row_box.append(k)
                    row_w.append(1.0 / (len(owner[k]) * 14))
            samples.append(([p[0] * W + p[1] for p in pos], [q[0] * W + q[1] for q in neg], rows, row_box, row_w, boxes_host[b, :nb, :7].numpy()))
        return self._forward_lists(cls, reg, anc, samples, B, H, W)

    @staticmethod
    def _reg_term(reg_b, anc, rows, rbox, w_row, boxes, H, W):
        """Smooth-L1 of the encoded box offsets of one sample as torch ops: reg_b [14,h,w], rows / rbox the regression cells and the
        box of each, w_row their weights, boxes [nbox,7]."""
        nrow = rows.shape[0]
        pred = reg_b.reshape(14, H * W)[:, rows].t().reshape(nrow, 2, 7)
        an = anc[:, :, rows].permute(2, 0, 1)            # [nrow,2,7]
        ref = boxes[rbox].unsqueeze(1)                   # [nrow,1,7]
        diag = torch.sqrt(an[:, :, 3:4] ** 2 + an[:, :, 4:5] ** 2)
        d = ref[:, :, 6] - an[:, :, 6]
        target = torch.cat(((ref[:, :, 0:2] - an[:, :, 0:2]) / diag, (ref[:, :, 2:3] - an[:, :, 2:3]) / an[:, :, 5:6],
                            torch.log(ref[:, :, 3:6] / an[:, :, 3:6]), torch.atan2(torch.sin(d), torch.cos(d)).unsqueeze(-1)), -1)
        per_row = F.smooth_l1_loss(pred, target, reduction="none").sum((1, 2))
        return (per_row * w_row).sum()                   # = sum over boxes of the per-box mean (loss.py:163,186)

    def _terms_host(self, cls, reg, anc, di, df, B, H, W):
        """The terms on the packed lists as torch ops (CPU tensors): gathers + CE + Smooth-L1, vectorised per sample."""
        dev = cls.device
        plan = di[:6 * B].reshape(B, 6).tolist()
        total = torch.zeros(1, device=dev)
        acc = torch.zeros(1, device=dev)
        for b in range(B):
            o, npos, nneg, nrow, of, nb = plan[b]
            pos_i, neg_i = di[o:o + npos], di[o + npos:o + npos + nneg]
            lc = torch.zeros(1, device=dev)
            for a in range(2):                                   # per anchor: loss.py:64-65
                sc = cls[b, 2 * a:2 * a + 2].reshape(2, H * W)
                term = None                                      # (an empty list has no term: hard mining with no candidate cell)
                if nneg > 0:
                    term = F.cross_entropy(sc[:, neg_i].t(), torch.zeros(nneg, dtype=torch.long, device=dev))
                if npos > 0:
                    tp = F.cross_entropy(sc[:, pos_i].t(), torch.ones(npos, dtype=torch.long, device=dev))
                    term = tp if term is None else tp + term
                if term is not None:
                    lc = lc + term
            lr = torch.zeros(1, device=dev)
            if nrow > 0:
                rows = di[o + npos + nneg:o + npos + nneg + nrow]
                rbox = di[o + npos + nneg + nrow:o + npos + nneg + 2 * nrow]
                w_row = df[of:of + nrow]
                boxes = df[of + nrow:of + nrow + nb * 7].reshape(nb, 7)
                lr = lr + self._reg_term(reg[b], anc, rows, rbox, w_row, boxes, H, W)
            total = lc + self.config["regress_loss_gain"] * lr
            acc = acc + total
        if self.reduction == "last":
            return total
        return acc if self.reduction == "sum" else acc / B

"""Shared by tests/test_loss_iou_host.py and tests/test_gpu_loss_iou.py: the regression inputs of the rotated-IoU regression term
(`iou_loss_gain`) on the maps of tests/_anchor_util.py, the input conditions (which kinds of pair occur, how far
every pair is from a change of topology) and the float64 statement of the whole loss with the term on (tests/_anchor_util.terms_statement
plus loss.anchor_iou_terms)."""
import numpy as np
import torch

from _anchor_util import B, MAPS, assigned, case, terms_statement
from _focal_util import regression_input
from _util import pkg

KINDS = ("3d", "bev")
GAIN = 2.0
ROLES = ("p contains q", "q contains p", "disjoint", "no z overlap", "loose", "tight")
# noise per offset channel (x, y, z, log l, log w, log h, yaw), in the offsets' own units
TIGHT = np.array([0.02, 0.02, 0.05, 0.02, 0.02, 0.05, 0.02])
LOOSE = np.array([0.15, 0.15, 0.20, 0.15, 0.15, 0.15, 0.20])


def case_iou(name, kind="3d", gain=GAIN, **over):
    return case(name, iou_loss_gain=gain, iou_loss_kind=kind, **over)


def encoded(anc_a, rows):
    """The regression targets of loss.anchor_terms: anc_a [7, m] anchors, rows [m, >= 7] labels -> [7, m] float64."""
    A, ref = np.asarray(anc_a, dtype=np.float64), np.asarray(rows, dtype=np.float64)[:, :7].T
    diag = np.sqrt(A[3] ** 2 + A[4] ** 2)
    dyaw = ref[6] - A[6]
    return np.stack(((ref[0] - A[0]) / diag, (ref[1] - A[1]) / diag, (ref[2] - A[2]) / A[5], np.log(ref[3] / A[3]), np.log(ref[4] / A[4]),
                     np.log(ref[5] / A[5]), np.arctan2(np.sin(dyaw), np.cos(dyaw))))


_REG = {}


def regression(name):
    """reg [B,14,H,W] fp32 of a map, built once: random offsets everywhere, and at every positive anchor of the statement's assignment the
    encoded target of its label plus seeded noise.  The positives of the map, counted through the samples in index order, take the
    ROLES in turn: the label scaled up or down inside tiny noise (one box contains the other), a shift in x or in z that separates the
    boxes, loose noise (IoU mostly below 0.5) and tight noise (IoU above 0.7)."""
    if name not in _REG:
        H, W, _, _, seed = MAPS[name]
        HW = H * W
        _, boxes, nb, _, _ = case(name)
        targets, anc = assigned(name)
        g = np.random.default_rng(7000 + seed)
        reg = regression_input(H, W).double().numpy().reshape(B, 14, HW)
        turn = 0
        for b in range(B):
            t = np.asarray(targets[b][0]).reshape(2, HW)
            for a in range(2):
                for cell in np.flatnonzero(t[a] >= 0):
                    enc = encoded(anc[a][:, cell:cell + 1], boxes[b, t[a, cell]].numpy()[None])[:, 0]
                    role, n = ROLES[turn % len(ROLES)], g.standard_normal(7)
                    turn += 1
                    if role == "p contains q":
                        off = 0.1 * TIGHT * n + np.array([0, 0, 0, 0.1, 0.1, 0.1, 0])
                    elif role == "q contains p":
                        off = 0.1 * TIGHT * n - np.array([0, 0, 0, 0.4, 0.4, 0.4, 0])
                    elif role == "disjoint":
                        off = TIGHT * n + np.array([3.0, 0, 0, 0, 0, 0, 0])
                    elif role == "no z overlap":
                        off = TIGHT * n + np.array([0, 0, 2.5, 0, 0, 0, 0])
                    else:
                        off = (LOOSE if role == "loose" else TIGHT) * n
                    reg[b, 7 * a:7 * a + 7, cell] = enc + off
        _REG[name] = torch.from_numpy(reg).float().reshape(B, 14, H, W).contiguous()
    return _REG[name]


def pairs(name, reg=None):
    """Per sample (j [m] anchor indices, p [m,7], q [m,7]) of the positive anchors, in float64 from the fp32 inputs (loss.decode_offsets)."""
    H, W = MAPS[name][:2]
    HW = H * W
    _, boxes, nb, _, _ = case(name)
    targets, anc = assigned(name)
    reg = regression(name) if reg is None else reg
    out = []
    for b in range(B):
        t = np.asarray(targets[b][0])
        j = np.flatnonzero(t >= 0)
        a, cell = j // HW, j % HW
        r = reg[b].reshape(14, HW).double().numpy()
        rr = np.stack([r[7 * a + c, cell] for c in range(7)])
        p, _ = pkg("loss").decode_offsets(rr, anc[a, :, cell].T)
        out.append((j, p.T, boxes[b, t[j], :7].double().numpy()))
    return out


def _side(P, Q):
    """Signed distance of every corner of the rectangles P [m,4,2] to every edge line of Q [m,4,2]: [m,4,4], positive inside."""
    a, b = Q[:, None, :, :], np.roll(Q, -1, axis=1)[:, None, :, :]
    e = b - a
    d = P[:, :, None, :] - a
    return (e[..., 0] * d[..., 1] - e[..., 1] * d[..., 0]) / np.hypot(e[..., 0], e[..., 1])


def geometry(p, q):
    """(corner-to-line distances p in q [m,4,4], q in p [m,4,4], z-face distances [m,4]) of pairs p, q [m,7]."""
    Lm = pkg("loss")
    P, Q = Lm._rects(p[:, 0], p[:, 1], p[:, 3], p[:, 4], p[:, 6]), Lm._rects(q[:, 0], q[:, 1], q[:, 3], q[:, 4], q[:, 6])
    tp, bp, tq, bq = p[:, 2] + p[:, 5] / 2, p[:, 2] - p[:, 5] / 2, q[:, 2] + q[:, 5] / 2, q[:, 2] - q[:, 5] / 2
    return _side(P, Q), _side(Q, P), np.stack((tp - tq, bp - bq, tp - bq, bp - tq), 1)


def margin(p, q, kind="3d"):
    """How far each pair is from a change of topology, in metres [m]: the least distance of a corner of one rectangle to an edge line of
    the other and ('3d') of two z faces to each other."""
    s_pq, s_qp, dz = geometry(p, q)
    m = np.minimum(np.abs(s_pq).reshape(len(p), -1).min(1), np.abs(s_qp).reshape(len(p), -1).min(1))
    return np.minimum(m, np.abs(dz).min(1)) if kind == "3d" else m


def kinds_present(name):
    """How many positives of the map are of each kind the tests need, by the statement: disjoint in the bird's-eye view; IoU in (0, 0.5);
    IoU > 0.7 (both for either kind of IoU); bird's-eye overlap without z overlap; p containing q; q containing p (as 3-D boxes)."""
    EK = pkg("evalkitti")
    n = dict.fromkeys(("disjoint", "low", "high", "no z overlap", "p contains q", "q contains p"), 0)
    for j, p, q in pairs(name):
        if not len(j):
            continue
        iou = np.array([EK.iou_pair(p[i], q[i]) for i in range(len(j))])          # (bev, 3d)
        s_pq, s_qp, dz = geometry(p, q)
        z_in = lambda d: (d[:, 0] < 0) & (d[:, 1] > 0)                              # p's z range strictly inside q's
        n["disjoint"] += int((iou[:, 0] == 0).sum())
        n["low"] += int(((iou > 0) & (iou < 0.5)).all(1).sum())
        n["high"] += int((iou > 0.7).all(1).sum())
        n["no z overlap"] += int(((iou[:, 0] > 0) & (iou[:, 1] == 0)).sum())
        n["p contains q"] += int(((s_qp > 0).reshape(len(j), -1).all(1) & z_in(-dz)).sum())
        n["q contains p"] += int(((s_pq > 0).reshape(len(j), -1).all(1) & z_in(dz)).sum())
    return n


def iou_statement(cfg, anc, boxes, nb, targets, reg, H, W):
    """The float64 statement of the IoU term alone on given targets, for cfg's reduction, gain and kind: (weighted loss term, its
    d / d reg [B,14,H,W], iou_terms [B,2] = (mean IoU of the positives, N_b), per-anchor IoU [B,2,HW])."""
    Lm = pkg("loss")
    gain, kind = Lm.parse_iou_loss_config(cfg)
    red = cfg.get("loss_reduction", "last")
    nB, HW = reg.shape[0], H * W
    gr, terms, maps = np.zeros((nB, 14, HW)), np.zeros((nB, 2)), np.zeros((nB, 2, HW))
    total = 0.0
    w = 1.0 / nB if red == "mean" else 1.0
    for b in ([nB - 1] if red == "last" else range(nB)):
        n = max(min(int(nb[b]), boxes.shape[1]), 0)
        li, n_pos, iou_sum, g, iou_map = Lm.anchor_iou_terms(reg[b].reshape(14, HW).numpy(), anc, boxes[b, :n].numpy(), targets[b], kind)
        gr[b], terms[b], maps[b] = g * (gain * w), (iou_sum / max(1, n_pos), n_pos), iou_map
        total += w * gain * li
    return total, gr.reshape(nB, 14, H, W), terms, maps


_WANT = {}


def statement(name, kind, pattern="uniform", **over):
    """(cfg, boxes, nb, H, W, cls, reg, want) of a committed case, computed once: want = (loss, dL/dcls, dL/dreg, terms [B,3], iou_terms
    [B,2], iou map [B,2,HW]) in float64 -- the anchor terms plus the IoU term."""
    from _focal_util import scores
    key = (name, kind, pattern, tuple(sorted(over.items())))
    if key not in _WANT:
        cfg, boxes, nb, H, W = case_iou(name, kind, **over)
        cls, reg = scores(pattern, H, W), regression(name)
        targets, anc = assigned(name)
        tg = [t for t, _, _ in targets]
        loss, gc, gr, terms = terms_statement(cfg, anc, boxes, nb, tg, cls, reg, H, W)
        li, gi, iou_terms, iou_map = iou_statement(cfg, anc, boxes, nb, tg, reg, H, W)
        _WANT[key] = (cfg, boxes, nb, H, W, cls, reg, (loss + li, gc, gr + gi, terms, iou_terms, iou_map))
    return _WANT[key]


def close_iou(iou_terms, want_terms):
    """iou_terms [B,2] against the statement: N_b exactly, the mean IoU at the loss bound 2e-6 * max(1, |.|)."""
    t = iou_terms.detach().cpu().double().numpy()
    assert t.shape == want_terms.shape and np.array_equal(t[:, 1], want_terms[:, 1]), (t, want_terms)
    assert (np.abs(t[:, 0] - want_terms[:, 0]) <= 2e-6 * np.maximum(1.0, np.abs(want_terms[:, 0]))).all(), (t, want_terms)

"""Lists for the list-driven loss kernel (dcf_loss_fwd_bwd), shared by the GPU loss tests (test infrastructure)."""
import numpy as np


def flat_lists(lists, bxs):
    """(ints, floats, plan) as LossTotal._forward_hip takes them, from per-sample (pos, neg, rows, row_box, row_w) and boxes [n, 7]."""
    ints, floats, plan = [], [], []
    for (pos, neg, rows, row_box, row_w), bx in zip(lists, bxs):
        o, of = len(ints), len(floats)
        ints += list(pos) + list(neg) + list(rows) + list(row_box)
        floats += [float(v) for v in row_w] + bx.reshape(-1).tolist()
        plan.append((o, len(pos), len(neg), len(rows), of, len(bx)))
    return ints, floats, plan


def assign_lists(Lc, boxes, nb, H, W, pos_neg=None):
    """Per sample the five lists of oracle/loss_ref.py::loss_from_lists -- (pos, neg, rows, row_box, row_w), cells as px * W + py,
    weights as fp32, the way the kernels hold them -- from LossTotal.assign of the compat-mode Lc (host side, numpy's generator as it
    stands).  pos_neg: take the positive and negative cells of sample b from pos_neg[b] instead (a device sampler's); assign's own
    draws are then thrown away, and numpy's generator is seeded with 0 before each of them.
    Returns (lists, boxes [n, 7] per sample, (ints, floats, plan) for Lc._forward_hip)."""
    lists, bxs = [], []
    for b in range(boxes.shape[0]):
        n = int(nb[b])
        if pos_neg is not None:
            np.random.seed(0)
        pos, neg, regress, owner = Lc.assign(boxes[b, :n], H, W)
        rows, row_box, row_w = [], [], []
        for k in range(n):
            for m in owner[k]:
                rows.append(regress[m][0] * W + regress[m][1]); row_box.append(k); row_w.append(1.0 / (len(owner[k]) * 14))
        pos, neg = ([p[0] * W + p[1] for p in pos], [v[0] * W + v[1] for v in neg]) if pos_neg is None else pos_neg[b][:2]
        lists.append((pos, neg, rows, row_box, np.asarray(row_w, dtype=np.float32)))
        bxs.append(boxes[b, :n, :7].numpy())
    return lists, bxs, flat_lists(lists, bxs)

"""GPU suite: the ranked evaluation on the device (`eval_metric: ranked`; csrc/evalpost.hip k_rank_* / k_ap_*)
against its host statement (evalrank.py): rank filter, suppression on the bird's-eye IoU (dcf_eval_nms mode 2), one-to-one matching,
accumulation and KITTI R40 average precision, through ops and RankedTest.  Integers compare exactly, average precision to 1e-12."""
import math

import numpy as np
import pytest
import torch

from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

THR = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]


def ER():
    return pkg("evalrank")


def harness(cls="RankedTest", **cfg):
    Tm = pkg("test")
    T = getattr(Tm, cls).__new__(getattr(Tm, cls))
    torch.nn.Module.__init__(T)
    T.config = dict({"score_threshold": 0.5}, **cfg)
    T.initialize_ap()
    return T


# ------------------------------------------------------------------ rank filter
def filter_pred():
    """[2,32,24,50]: 2400 candidates per sample (more than one 1024-thread pass), scores quantised to 1/64; sample 1 has none."""
    det = pkg("detfill")
    pred = det.uniform((2, 32, 24, 50), 7100, -1.0, 1.0)
    for a in range(2):
        pred[0, 2 * a + 1] = (np.round(det.uniform((24, 50), 7101 + a, 0.0, 1.0) * 64.0) / 64.0).astype(np.float32)
        pred[1, 2 * a + 1] = -1.0
    pred[0, 1, 3, 7] = np.nan                                           # a NaN score is never kept
    return pred


@pytest.mark.parametrize("cap", [4096, 64, 100])
def test_rank_filter_equals_host_statement(cap):
    ops = pkg("ops")
    pred = filter_pred()
    full = ER().rank_filter(pred, 0.5, 4096)
    want = ER().rank_filter(pred, 0.5, cap)
    assert 1024 < full[3][0] < 2400 and full[3][1] == 0
    if cap < 4096:
        assert full[1][0, cap - 1] == full[1][0, cap], "a block of tied scores must straddle the cut"
    boxes, scores, count, total = ops.eval_rank_filter(torch.from_numpy(pred).cuda(), 0.5, cap)
    assert count.cpu().tolist() == want[2].tolist() == [min(cap, int(full[3][0])), 0]
    assert total.cpu().tolist() == want[3].tolist() == full[3].tolist()
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


# ------------------------------------------------------------------ suppression (mode 2) + matching
def mapped(u, span):
    return np.stack([u[:, 0] * span, u[:, 1] * span, -1.0 + 0.2 * u[:, 2], 3.5 + 1.3 * u[:, 3], 1.6 + 0.5 * u[:, 4], 1.4 + 0.4 * u[:, 5],
                     3.14159 * u[:, 6]], 1).astype(np.float32)


_CASES = {}


def case(n, G, seed, nms_iou):
    """Detections in rank order, label rows, and the host statement's decisions with their distance from every threshold."""
    key = (n, G, seed, nms_iou)
    if key in _CASES:
        return _CASES[key]
    det = pkg("detfill")
    u = det.uniform((n, 8), seed, 0.0, 1.0)
    span = 3.0 * np.sqrt(n)
    boxes = mapped(u, span)
    labels = mapped(det.uniform((G, 7), seed + 1, 0.0, 1.0), span)
    for i in range(min(n, 4 * G)):
        s = 0.02 * (1 + i // G) ** 2
        boxes[i] = (labels[i % G].astype(np.float64) + (u[i, :7].astype(np.float64) - 0.5) * np.array([4 * s, 4 * s, 0.1, s, s, 0.1, 0.5 * s])).astype(np.float32)
    scores = (np.round(u[:, 7] * 64.0) / 64.0).astype(np.float32)
    order = np.argsort(ER().rank_keys(scores, np.arange(n)))[::-1]
    boxes, scores = np.ascontiguousarray(boxes[order]), scores[order]
    refs = np.zeros((G + 3, 9), dtype=np.float32)                       # three unlabelled rows: first, in the middle, last
    rows = [r for r in range(G + 3) if r not in (0, G // 2 + 1, G + 2)]
    refs[rows, :7], refs[rows, 8] = labels, 1.0
    refs[0, :7], refs[G + 2, :7] = labels[0], labels[-1]                # copies of labelled boxes that must never be taken
    # the host statement, keeping the distance of every decision from its threshold
    b64 = boxes.astype(np.float64)
    keep, kept, m_nms = np.zeros(n, np.int32), [], math.inf
    for i in range(n):
        v = [ER().bev_iou(b64[i], b64[j]) for j in kept]
        m_nms = min([m_nms] + [abs(x - nms_iou) for x in v])
        if not any(x > nms_iou for x in v):
            keep[i] = 1
            kept.append(i)
    iou = ER().iou_matrix(boxes, keep, refs)
    pos = [np.sort(row[row > 0]) for row in iou[keep != 0]]
    m_thr = min(abs(x - t) for row in pos for x in row for t in THR)
    m_gap = min([math.inf] + [float(np.diff(row).min()) for row in pos if len(row) > 1])
    tp = ER().match(boxes, keep, refs, THR, iou=iou)
    _CASES[key] = dict(boxes=boxes, scores=scores, refs=refs, keep=keep, tp=tp, margins=(m_nms, m_thr, m_gap))
    return _CASES[key]


def device_decisions(c, nms_iou, pad=0):
    """keep flags and tpmask of the device for case c; pad: rows past the count (they must not be read as candidates)."""
    ops = pkg("ops")
    n = len(c["boxes"])
    boxes = torch.from_numpy(np.concatenate([c["boxes"], c["boxes"][:pad]])).cuda()
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    keep, nkeep = ops.eval_nms(boxes, "bev", nms_iou, count=count)
    tp = ops.eval_match_ranked(boxes, keep, count, torch.from_numpy(c["refs"]).cuda(), torch.tensor(THR, dtype=torch.float64, device="cuda"))
    return boxes, keep, nkeep, tp


@pytest.mark.parametrize("n,G,seed,survivors,tps", [
    (65, 5, 7001, 29, [4, 4, 4, 3, 2, 2, 2, 2, 2, 2]),
    (300, 20, 7002, 140, [10, 10, 10, 10, 10, 10, 9, 5, 4, 3]),
    (300, 70, 7003, 67, [56, 55, 54, 48, 46, 40, 35, 24, 20, 13])])
def test_nms_bev_and_one_to_one_matching_equal_host_statement(n, G, seed, survivors, tps):
    c = case(n, G, seed, 0.1)
    print("margins (nms, threshold, gap):", c["margins"], "survivors", int(c["keep"].sum()),
          "tp", [int(((c["tp"] >> t) & 1).sum()) for t in range(10)])
    # a condition on the inputs, not a tolerance: no decision of the host statement hangs on the last bits of cos / sin
    assert min(c["margins"]) >= 1e-9
    assert int(c["keep"].sum()) == survivors
    assert [int(((c["tp"] >> t) & 1).sum()) for t in range(10)] == tps
    _, keep, nkeep, tp = device_decisions(c, 0.1, pad=7)
    assert keep.cpu().numpy()[:n].tolist() == c["keep"].tolist() and not keep.cpu().numpy()[n:].any()
    assert int(nkeep.cpu()) == survivors
    assert tp.cpu().numpy()[:n].view(np.uint32).tolist() == c["tp"].tolist()


def test_duplicates_count_once_where_the_compat_counter_counts_each():
    """Suppression threshold 0.7: duplicates survive; one-to-one matching counts a label once, Test.precision_recall_singleshot
    counts every survivor that overlaps a label."""
    n, G = 65, 5
    c = case(n, G, 7001, 0.7)
    assert min(c["margins"]) >= 1e-9
    boxes, keep, _, tp = device_decisions(c, 0.7)
    assert keep.cpu().numpy().tolist() == c["keep"].tolist() and tp.cpu().numpy().view(np.uint32).tolist() == c["tp"].tolist()
    ranked_tp = int((c["tp"] & 1).sum())
    assert 0 < ranked_tp <= G
    T = harness("Test")
    surv = [boxes[i] for i in np.nonzero(c["keep"])[0]]
    T.precision_recall_singleshot([surv], torch.from_numpy(c["refs"])[None])
    assert T.get_num_P() == len(surv) and T.get_num_T() == G
    assert ranked_tp < T.get_num_TP_set()[0.5]


@pytest.mark.parametrize("rows", [(3, 10), (3, 67), (70, 6)])
def test_iou_ties_go_to_the_lower_row_on_the_device(rows):
    """A detection midway between two labelled rows (axis-aligned, so the two IoUs are the same fp64 number on host and device)
    takes the lower ROW, whichever lane holds it: rows in two lanes, in one lane (3 and 67), and the lower row in the higher lane."""
    ops = pkg("ops")

    def box(x):
        return [x, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0]
    refs = np.zeros((80, 9), dtype=np.float32)
    refs[:, :7] = box(1.0)                                              # unlabelled copies under the detection: never taken
    refs[rows[0], :7], refs[rows[1], :7] = box(0.0), box(2.0)
    refs[list(rows), 8] = 1.0
    dets = np.array([box(1.0), box(-0.2 if rows[0] < rows[1] else 2.2)], dtype=np.float32)
    keep = np.ones(2, np.int32)
    iou = ER().iou_matrix(dets, keep, refs)
    assert iou[0, rows[0]] == iou[0, rows[1]] and np.isnan(iou[0]).sum() == 78
    want = ER().match(dets, keep, refs, THR, iou=iou)
    assert want.tolist() == [0b0000000011, 0b0111111100]              # the second detection finds its row taken at 0.5 and 0.55
    tp = ops.eval_match_ranked(torch.from_numpy(dets).cuda(), torch.from_numpy(keep).cuda(), torch.tensor([2], dtype=torch.int32, device="cuda"),
                               torch.from_numpy(refs).cuda(), torch.tensor(THR, dtype=torch.float64, device="cuda"))
    assert tp.cpu().numpy().view(np.uint32).tolist() == want.tolist()


# ------------------------------------------------------------------ accumulate + average precision
def feed(T, scores, tpmask, n_gt, parts, truncated_part=None):
    """Appends the detections in len(parts) calls of ops.eval_accumulate: kept rows between rows that are not kept, rows past the
    count that are flagged but must be ignored, and the labels spread over the calls."""
    ops = pkg("ops")
    acc = T._accumulators(torch.device("cuda", torch.cuda.current_device()))
    lo = 0
    for k, m in enumerate(parts):
        rows = m + m // 3 + 4
        keep = np.ones(rows, np.int32)
        keep[3::4] = 0
        idx = np.nonzero(keep)[0][:m]
        count = int(idx[-1]) + 1 if m else 0
        keep[count:] = 1                                                # junk past the count
        sc = np.full(rows, 7.0, np.float32)
        tp = np.full(rows, 0x3FF, np.uint32)
        sc[idx], tp[idx] = scores[lo:lo + m], tpmask[lo:lo + m]
        lo += m
        g = n_gt // 3 + (n_gt % 3 if k == 0 else 0)
        refs = np.zeros((g + 5, 9), np.float32)
        refs[2:2 + g, 8] = 1.0
        refs[0, 8] = 2.0                                                # only == 1 is a label
        total = rows + 1 if k == truncated_part else count
        ops.eval_accumulate(torch.from_numpy(sc).cuda(), torch.from_numpy(tp.view(np.int32)).cuda(), torch.from_numpy(keep).cuda(),
                            torch.tensor([count], dtype=torch.int32, device="cuda"), torch.tensor([total], dtype=torch.int32, device="cuda"),
                            torch.from_numpy(refs).cuda(), acc["scores"], acc["tpmask"], acc["state"])
    assert lo == len(scores)


def detections(N, seed):
    det = pkg("detfill")
    scores = (np.round(det.uniform((N,), seed, 0.5, 1.0) * 32.0) / 32.0).astype(np.float32)         # heavily tied
    u = det.uniform((N, 10), seed + 1, 0.0, 1.0)
    tpmask = np.zeros(N, dtype=np.uint32)
    for t in range(10):
        tpmask |= ((u[:, t] < 0.8 - 0.06 * t).astype(np.uint32) << np.uint32(t))
    return scores, tpmask


@pytest.mark.parametrize("n_gt", [0, 7, 1000])
@pytest.mark.parametrize("N", [0, 1, 65, 5000])
def test_accumulate_and_average_precision_equal_host_statement(N, n_gt):
    scores, tpmask = detections(N, 7200 + N)
    T = harness(eval_max_detections=8192)
    feed(T, scores, tpmask, n_gt, [N // 7, N // 2, N - N // 7 - N // 2], truncated_part=1)
    got = T.summary()
    want = ER().summarize(scores, tpmask, n_gt, THR, truncated=1)
    assert (got["num_P"], got["num_T"], got["truncated_candidates"]) == (N, n_gt, 1)
    assert got["tp"] == want["tp"]
    assert (T.get_num_P(), T.get_num_T(), T.get_num_TP_set()) == (N, n_gt, want["tp"])
    for t in THR:
        if n_gt == 0:
            assert math.isnan(got["ap"][t]) and math.isnan(want["ap"][t]) and math.isnan(got["recall"][t])
        else:
            assert abs(got["ap"][t] - want["ap"][t]) <= 1e-12, (t, got["ap"][t], want["ap"][t])
            assert got["recall"][t] == want["recall"][t]
        assert got["precision"][t] == want["precision"][t]
    assert math.isnan(got["map"]) if n_gt == 0 else abs(got["map"] - want["map"]) <= 1e-12
    # the accumulated order is the order fed
    acc = T._acc
    assert np.array_equal(acc["scores"][:N].cpu().numpy(), scores) and np.array_equal(acc["tpmask"][:N].cpu().numpy().view(np.uint32), tpmask)
    # initialize_ap starts over on the same buffers
    T.initialize_ap()
    assert T.summary()["num_P"] == 0 and T.summary()["num_T"] == 0


def test_accumulator_overflow_raises_and_writes_nothing_past_the_capacity():
    scores, tpmask = detections(300, 7300)
    T = harness(eval_max_detections=256)
    feed(T, scores, tpmask, 7, [100, 150, 50])
    with pytest.raises(RuntimeError, match="eval_max_detections"):
        T.summary()
    acc = T._acc
    assert acc["scores"].shape[0] == 256 and acc["state"].cpu().tolist()[:2] == [300, 7]
    assert np.array_equal(acc["scores"].cpu().numpy(), scores[:256])


# ------------------------------------------------------------------ end to end
def test_ranked_eval_step_on_device_equals_host_statement():
    from test_gpu_model import build, tiny_input
    z = load_golden("model_tiny.npz")
    lz = load_golden("loss.npz")
    net, cfg = build(golden_cfg(z), "f32")
    cfg["score_threshold"] = 0.5
    Tm = pkg("test")
    x = tiny_input().cuda()
    img = torch.zeros(x.shape[0], 3, 8, 8, dtype=torch.uint8, device="cuda")
    boxes, nb = torch.from_numpy(lz["bboxes"]), torch.from_numpy(lz["nbox"])
    with torch.no_grad():
        pred = net(x, img)
    T = Tm.RankedTest(net, dict(cfg, eval_metric="ranked"))
    H = Tm.RankedTest(net, dict(cfg, eval_metric="ranked"))
    C = Tm.Test(net, cfg)
    for step in range(2):
        np.random.seed(3)
        loss_d, cand = T.get_eval_value_onestep(x, img, boxes, nb)
        np.random.seed(3)
        loss_c, _ = C.get_eval_value_onestep(x, img, boxes, nb)
        assert abs(loss_d - loss_c) < 1e-6
        H.accumulate(pred.cpu(), boxes)
        hb, hc = H._last[0], H._last[2]
        assert [int(c.shape[0]) for c in cand] == hc.tolist() and sum(hc.tolist()) > 0
        assert all(np.array_equal(cand[b].cpu().numpy(), hb[b, :hc[b]]) for b in range(len(cand)))
        dd, dh = T.detections(), H.detections()
        assert all(torch.equal(p[0].cpu(), q[0]) and torch.equal(p[1].cpu(), q[1]) for p, q in zip(dd, dh))
    got, want = T.summary(), H.summary()
    assert got["num_P"] == want["num_P"] > 0 and got["num_T"] == want["num_T"] > 0 and got["tp"] == want["tp"]
    assert got["truncated_candidates"] == want["truncated_candidates"] == 0
    for t in THR:
        assert abs(got["ap"][t] - want["ap"][t]) <= 1e-12 and got["precision"][t] == want["precision"][t] and got["recall"][t] == want["recall"][t]
    assert abs(got["map"] - want["map"]) <= 1e-12


# ------------------------------------------------------------------ the compat path shares k_eval_pairs: still the golden survivors
def test_compat_suppression_is_untouched_after_the_ranked_kernels_ran():
    z = load_golden("eval.npz")
    T = harness("Test")
    pred = [torch.from_numpy(z["pred"][b]).cuda() for b in range(2)]
    pkg("ops").eval_nms(pred[0], "bev", 0.1)                            # mode 2 first, in this process
    ki, ks = T.NMS_IOU(pred, 0.01), T.NMS_SAT(pred)

    def idx(kept, boxes):
        b = boxes.cpu().numpy()
        return np.array([int(np.where((b == k.cpu().numpy()).all(1))[0][0]) for k in kept], dtype=np.int64)
    for b in range(2):
        assert np.array_equal(idx(ki[b], pred[b]), z["keep_iou_%d" % b]), "IoU survivors of sample %d" % b
        assert np.array_equal(idx(ks[b], pred[b]), z["keep_sat_%d" % b]), "SAT survivors of sample %d" % b

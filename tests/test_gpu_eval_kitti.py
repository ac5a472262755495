"""GPU suite: the KITTI-style protocol on the device (`eval_protocol: kitti`; csrc/evalpost.hip k_kitti_*)
against its host statement (evalkitti.py): projected flags, the two IoU matrices, the three-outcome matching per (metric, difficulty,
threshold), accumulation and average precision without the ignored detections, through ops and RankedTest.  Integers, masks, flags
and counts compare exactly, IoU and average precision to 1e-12.  Every case first asserts from the host statement that no decision
is closer than 1e-9 to its boundary (the device's cos / sin may differ from libm in the last bit): a condition on the inputs."""
import math

import numpy as np
import pytest
import torch

from _util import golden_cfg, load_golden, pkg

pytestmark = pytest.mark.gpu

THR = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
IH, IW = 375, 1242


def EK():
    return pkg("evalkitti")


def ER():
    return pkg("evalrank")


def camera(x0, y0, z0, f=400.0, cx=621.0, cy=187.0):
    """[4,3] pinhole at (x0, y0, z0) looking along +x: d = x - x0, u = cx - f (y - y0) / d, v = cy - f (z - z0) / d."""
    return np.array([[cx, cy, 1.0], [-f, 0.0, 0.0], [0.0, -f, 0.0], [-cx * x0 + f * y0, -cy * x0 + f * z0, -x0]], dtype=np.float32)


def harness(**cfg):
    Tm = pkg("test")
    T = Tm.RankedTest.__new__(Tm.RankedTest)
    torch.nn.Module.__init__(T)
    T.config = dict({"score_threshold": 0.5, "eval_metric": "ranked", "eval_protocol": "kitti", "image_height": IH, "image_width": IW}, **cfg)
    T.initialize_ap()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ the distance of every decision from its boundary
def margins(boxes, keep, refs, C, dontcare, s, nms_iou):
    """min over: |IoU - nms threshold| among the suppression tests, |IoU - t| and the gaps between a survivor's positive IoUs (both
    metrics), |corner depth|, |height - minimum|, |DontCare share - overlap|."""
    E, R = EK(), ER()
    b64 = boxes.astype(np.float64)
    kept, m = [], math.inf
    for i in range(len(boxes)):
        v = [R.bev_iou(b64[i], b64[j]) for j in kept]
        m = min([m] + [abs(x - nms_iou) for x in v])
        if not any(x > nms_iou for x in v):
            kept.append(i)
    assert kept == np.nonzero(keep)[0].tolist()
    for mat in E.iou_matrices(boxes, keep, refs):
        for row in mat[keep != 0]:
            pos = np.sort(row[row > 0])
            m = min([m] + [abs(x - t) for x in pos for t in THR] + ([float(np.diff(pos).min())] if len(pos) > 1 else []))
    C64 = np.asarray(C, np.float32).astype(np.float64)
    for b in boxes:
        rect = pkg("evalgeom").bev_rect(b[:2].astype(np.float64), b[3:5].astype(np.float64), float(b[6]))
        for z in (float(b[2]) - float(b[5]) / 2, float(b[2]) + float(b[5]) / 2):
            m = min([m] + [abs(x * C64[0, 2] + y * C64[1, 2] + z * C64[2, 2] + C64[3, 2]) for x, y in rect])
        p = E.project_box(b, C, IH, IW)
        m = min([m] + [abs(p[4] - h) for h in s["min_height"]])
        if p[5] > 0 and dontcare is not None:
            m = min([m] + [abs(E.dontcare_ratio(p, rc) - s["dontcare_overlap"]) for rc in dontcare])
    return m


# ------------------------------------------------------------------ one sample: flags, IoU matrices, matching
def mapped(u, span):
    return np.stack([u[:, 0] * span, u[:, 1] * span, -1.0 + 0.2 * u[:, 2], 3.5 + 1.3 * u[:, 3], 1.6 + 0.5 * u[:, 4], 1.4 + 0.4 * u[:, 5],
                     3.14159 * u[:, 6]], 1).astype(np.float32)


def rectangles(D, seed):
    u = pkg("detfill").uniform((max(D, 1), 4), seed, 0.0, 1.0)[:D]
    l, t = u[:, 0] * IW * 0.8, u[:, 1] * IH * 0.6
    return np.stack([l, t, l + 40.0 + u[:, 2] * 500.0, t + 30.0 + u[:, 3] * 200.0], 1).astype(np.float32).reshape(D, 4)


N, G, R_ROWS, NMS_IOU = 300, 64, 70, 0.1
_CASE = {}


def case():
    """300 detections in rank order (about 150 survive), R = 70 label rows (a lane of the matching holds two) of which 6 are not
    valid, levels mixed 0 / 1 / 2 / 3, a zero-area detection and a zero-area valid row (a NaN pair), a camera inside the scene so
    that boxes lie in front of it, behind it and across its plane; the host statement's decisions for D = 33 rectangles."""
    if _CASE:
        return _CASE
    det, E = pkg("detfill"), EK()
    u = det.uniform((N, 8), 8001, 0.0, 1.0)
    span = 3.0 * np.sqrt(N)
    boxes = mapped(u, span)
    labels = mapped(det.uniform((G, 7), 8002, 0.0, 1.0), span)
    for i in range(2 * G):
        s = 0.02 * (1 + i // G) ** 2
        boxes[i] = (labels[i % G].astype(np.float64) + (u[i, :7].astype(np.float64) - 0.5) * np.array([4 * s, 4 * s, 1.2, s, s, 0.4, 0.5 * s])).astype(np.float32)
    boxes[N - 1, 3:5] = 0.0                                             # a zero-area detection at ...
    labels[G - 1, 3:5] = 0.0                                            # ... the zero-area row: NaN in both matrices
    boxes[N - 1, :2] = labels[G - 1, :2]
    scores = (np.round(u[:, 7] * 64.0) / 64.0).astype(np.float32)
    order = np.argsort(ER().rank_keys(scores, np.arange(N)))[::-1]
    boxes, scores = np.ascontiguousarray(boxes[order]), scores[order]
    refs = np.zeros((R_ROWS, 9), dtype=np.float32)
    invalid = (0, 9, 33, 64, 65, 69)
    rows = [r for r in range(R_ROWS) if r not in invalid]
    refs[rows, :7], refs[rows, 8] = labels, 1.0
    refs[0, :7], refs[69, :7], refs[33, :7], refs[33, 8] = labels[0], labels[-2], labels[5], 2.0       # copies that do not exist
    levels = (det.uniform((R_ROWS,), 8003, 0.0, 1.0) * 4.0).astype(np.int32).clip(0, 3)
    C = camera(15.0, 0.5 * span, -1.0)
    dc = rectangles(33, 8004)
    s = E.settings({})
    keep = ER().nms(boxes, NMS_IOU)
    bev, i3d = E.iou_matrices(boxes, keep, refs)
    flags = E.det_flags(boxes, C, IH, IW, dc, s)
    tp, ig = E.match_levels(keep, refs, levels, bev, i3d, flags, THR)
    _CASE.update(boxes=boxes, scores=scores, refs=refs, levels=levels, C=C, dc=dc, s=s, keep=keep, bev=bev, i3d=i3d, flags=flags, tp=tp, ig=ig,
                 margin=margins(boxes, keep, refs, C, dc, s, NMS_IOU))
    return _CASE


def test_case_is_away_from_every_boundary_and_covers_the_paths():
    c = case()
    print("margin", c["margin"], "survivors", int(c["keep"].sum()), "levels", np.bincount(c["levels"][c["refs"][:, 8] == 1], minlength=4).tolist())
    assert c["margin"] >= 1e-9
    assert 130 <= int(c["keep"].sum()) <= 200
    assert (np.bincount(c["levels"][c["refs"][:, 8] == 1], minlength=4) >= 5).all()
    last = np.nonzero((c["boxes"][:, 3] == 0))[0]
    assert len(last) == 1 and c["keep"][last[0]] == 1 and np.isnan(c["bev"][last[0]]).sum() == 7 and np.isnan(c["i3d"][last[0]]).sum() == 7
    front = [sum(1 for z in (-1, 1) for x, y in pkg("evalgeom").bev_rect(b[:2], b[3:5], b[6]) if x > 15.0) for b in c["boxes"].astype(np.float64)]
    assert min(front) == 0 and max(front) == 8 and any(0 < f < 8 for f in front), "behind, in front of and across the camera plane"
    surv = c["keep"] != 0
    for m in range(2):
        tp, ig = c["tp"][m][surv], c["ig"][m][surv]
        assert not (tp & ig).any()
        for d in range(3):
            f = np.uint32(0x3FF << (10 * d))
            assert (tp & f).any() and (ig & f).any() and ((~(tp | ig)) & f).any(), "all three outcomes at (%d, %d)" % (m, d)
    assert (c["tp"][0] != c["tp"][1]).any() and (c["ig"][0][surv] != c["ig"][0][surv][0]).any()
    assert ((c["flags"] & 8) != 0).any() and ((c["flags"] & 8) == 0).any() and len(set(c["flags"].tolist())) >= 4


@pytest.mark.parametrize("D", [0, 1, 33])
def test_det_flags_equal_host_statement(D):
    ops, c = pkg("ops"), case()
    dc = c["dc"][:D] if D != 1 else c["dc"][2:3]
    want = c["flags"] if D == 33 else EK().det_flags(c["boxes"], c["C"], IH, IW, dc, c["s"])
    if D == 0:
        assert not (want & 8).any() and (want == (c["flags"] & 7)).all()
    else:
        assert (want & 8).any()
    pad = 9                                                             # rows past the count are not candidates
    boxes = dev(np.concatenate([c["boxes"], c["boxes"][:pad]]))
    got = ops.eval_det_flags(boxes, torch.tensor([N], dtype=torch.int32, device="cuda"), c["C"], dev(dc) if D else None, IH, IW,
                             c["s"]["min_height"], c["s"]["dontcare_overlap"])
    assert u32(got)[:N].tolist() == want.tolist() and not u32(got)[N:].any()


def device_match(c, levels="case", count=None, flags=None, refs=None):
    ops = pkg("ops")
    pad = 7
    n = N if count is None else count
    boxes = dev(np.concatenate([c["boxes"], c["boxes"][:pad]]))
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    keep, nkeep = ops.eval_nms(boxes, "bev", NMS_IOU, count=cnt)
    refs = dev(c["refs"] if refs is None else refs)
    bev, i3d = ops.eval_iou_levels(boxes, keep, cnt, refs)
    fl = dev((c["flags"] if flags is None else flags).view(np.int32))
    fl = torch.cat([fl, torch.full((pad,), 15, dtype=torch.int32, device="cuda")])
    lv = dev(c["levels"]) if isinstance(levels, str) else levels
    tp, ig = ops.eval_match_levels(bev, i3d, keep, cnt, refs, lv, fl, torch.tensor(THR, dtype=torch.float64, device="cuda"))
    return keep, bev, i3d, tp, ig


def test_iou_matrices_and_matching_equal_host_statement():
    c = case()
    assert c["margin"] >= 1e-9
    keep, bev, i3d, tp, ig = device_match(c)
    assert keep.cpu().numpy()[:N].tolist() == c["keep"].tolist() and not keep.cpu().numpy()[N:].any()
    for got, want in ((bev, c["bev"]), (i3d, c["i3d"])):
        got = got.cpu().numpy()[:N]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.nanmax(np.abs(got - want)) <= 1e-12
    assert np.array_equal(u32(tp)[:, :N], c["tp"]) and np.array_equal(u32(ig)[:, :N], c["ig"])
    assert not u32(tp)[:, N:].any() and not u32(ig)[:, N:].any()
    # without levels every valid row is level 0: nothing is ignored by a row, and the bird's-eye bits are evalrank.match's
    keep, _, _, tp, ig = device_match(c, levels=None)
    want_tp, want_ig = EK().match_levels(c["keep"], c["refs"], None, c["bev"], c["i3d"], c["flags"], THR)
    assert np.array_equal(u32(tp)[:, :N], want_tp) and np.array_equal(u32(ig)[:, :N], want_ig)
    plain = ER().match(c["boxes"], c["keep"], c["refs"], THR, iou=c["bev"])
    assert want_tp[0].tolist() == (plain | (plain << np.uint32(10)) | (plain << np.uint32(20))).tolist()


def test_empty_sample_and_sample_without_a_valid_row():
    c = case()
    keep, _, _, tp, ig = device_match(c, count=0)
    assert not keep.cpu().numpy().any() and not u32(tp).any() and not u32(ig).any()
    refs = c["refs"].copy()
    refs[:, 8] = 0.0
    keep, bev, i3d, tp, ig = device_match(c, refs=refs)
    assert np.isnan(bev.cpu().numpy()[:N]).all() and np.isnan(i3d.cpu().numpy()[:N]).all() and not u32(tp).any()
    none = np.full((N, R_ROWS), np.nan)
    want_tp, want_ig = EK().match_levels(c["keep"], refs, c["levels"], none, none, c["flags"], THR)
    assert not want_tp.any() and want_ig.any() and np.array_equal(u32(ig)[:, :N], want_ig)
    # and through the accumulator: the empty sample adds its counted rows only
    ops = pkg("ops")
    T = harness(eval_max_detections=512)
    acc = T._accumulators(torch.device("cuda", torch.cuda.current_device()))
    z = torch.zeros(N, dtype=torch.int32, device="cuda")
    ops.eval_accumulate_levels(dev(c["scores"]), torch.zeros((2, N), dtype=torch.int32, device="cuda"), torch.zeros((2, N), dtype=torch.int32, device="cuda"),
                               z + 1, z[:1], z[:1], dev(c["refs"]), dev(c["levels"]), acc["scores"], acc["tpmask"], acc["igmask"], acc["state"])
    assert acc["state"].cpu().tolist() == [0] + EK().count_rows(c["refs"], c["levels"]).tolist() + [0, 0, 0, 0]


# ------------------------------------------------------------------ accumulate + average precision
def random_marks(n, seed):
    det = pkg("detfill")
    scores = (np.round(det.uniform((n,), seed, 0.5, 1.0) * 32.0) / 32.0).astype(np.float32)        # heavily tied
    u = det.uniform((4, max(n, 1), 30), seed + 1, 0.0, 1.0)[:, :n]
    tp = np.zeros((2, n), np.uint32)
    ig = np.zeros((2, n), np.uint32)
    for m in range(2):
        for k in range(30):
            tp[m] |= (u[m, :, k] < 0.7 - 0.015 * k).astype(np.uint32) << np.uint32(k)
            ig[m] |= (u[2 + m, :, k] < 0.1 + 0.01 * k).astype(np.uint32) << np.uint32(k)
    return scores, tp, ig


def feed(T, scores, tp, ig, row_levels, parts, truncated_part=None):
    """Appends the detections in len(parts) calls of ops.eval_accumulate_levels: kept rows between rows that are not kept, flagged junk
    past the count, and the label rows (with their levels, between rows that are not valid) spread over the calls."""
    ops = pkg("ops")
    acc = T._accumulators(torch.device("cuda", torch.cuda.current_device()))
    lo, glo = 0, 0
    for k, m in enumerate(parts):
        rows = m + m // 3 + 4
        keep = np.ones(rows, np.int32)
        keep[3::4] = 0
        idx = np.nonzero(keep)[0][:m]
        count = int(idx[-1]) + 1 if m else 0
        keep[count:] = 1                                                # junk past the count
        sc = np.full(rows, 7.0, np.float32)
        tpm = np.full((2, rows), 0x3FFFFFFF, np.uint32)
        igm = np.full((2, rows), 0x3FFFFFFF, np.uint32)
        sc[idx], tpm[:, idx], igm[:, idx] = scores[lo:lo + m], tp[:, lo:lo + m], ig[:, lo:lo + m]
        lo += m
        g = len(row_levels) // len(parts) + (len(row_levels) % len(parts) if k == 0 else 0)
        refs = np.zeros((g + 5, 9), np.float32)
        lv = np.zeros(g + 5, np.int32)                                  # level 0 on rows that are not valid: must not count
        refs[2:2 + g, 8], lv[2:2 + g] = 1.0, row_levels[glo:glo + g]
        refs[0, 8] = 2.0                                                # only == 1 is a label
        glo += g
        total = rows + 1 if k == truncated_part else count
        ops.eval_accumulate_levels(dev(sc), dev(tpm.view(np.int32)), dev(igm.view(np.int32)), dev(keep), torch.tensor([count], dtype=torch.int32, device="cuda"),
                                   torch.tensor([total], dtype=torch.int32, device="cuda"), dev(refs), dev(lv), acc["scores"], acc["tpmask"], acc["igmask"],
                                   acc["state"])
    assert lo == len(scores) and glo == len(row_levels)


def same(got, want, ap_tol=1e-12):
    assert set(got) == set(want) and (got["protocol"], got["num_P"], got["truncated_candidates"]) == (want["protocol"], want["num_P"], want["truncated_candidates"])
    for metric in ("bev", "3d"):
        for name in ("easy", "moderate", "hard"):
            g, w = got[metric][name], want[metric][name]
            assert g["tp"] == w["tp"] and g["num_ignored"] == w["num_ignored"] and g["num_T"] == w["num_T"] and g["precision"] == w["precision"]
            for t in THR:
                if w["num_T"] == 0:
                    assert math.isnan(g["ap"][t]) and math.isnan(w["ap"][t]) and math.isnan(g["recall"][t]) and math.isnan(w["recall"][t])
                else:
                    assert abs(g["ap"][t] - w["ap"][t]) <= ap_tol, (metric, name, t, g["ap"][t], w["ap"][t])
                    assert g["recall"][t] == w["recall"][t]
            assert math.isnan(g["map"]) and math.isnan(w["map"]) if w["num_T"] == 0 else abs(g["map"] - w["map"]) <= ap_tol


@pytest.mark.parametrize("n", [0, 1, 1100])
def test_accumulate_and_average_precision_equal_host_statement(n):
    """1100 detections: more than one 1024 chunk, so the scans over the true positives and over the detections that stay both carry.
    No row of level 0: n_gt = (0, 40, 90), NaN at easy."""
    scores, tp, ig = random_marks(n, 8100 + n)
    row_levels = np.array([1] * 40 + [2] * 50 + [3] * 30, np.int32)
    T = harness(eval_max_detections=2048)
    feed(T, scores, tp, ig, row_levels, [n // 7, n // 2, n - n // 7 - n // 2], truncated_part=1)
    got = T.summary()
    want = EK().summarize(scores, tp, ig, [0, 40, 90], THR, truncated=1)
    same(got, want)
    assert got["bev"]["hard"]["num_T"] == 90 and (n < 1100 or min(got["3d"]["hard"]["num_ignored"].values()) > 0)
    assert (T.get_num_P(), T.get_num_T(), T.get_num_TP_set()) == (n, 40, want["bev"]["moderate"]["tp"])
    acc = T._acc
    assert acc["state"].cpu().tolist() == [n, 0, 40, 90, 1, 0, 0, 0]
    assert np.array_equal(acc["scores"][:n].cpu().numpy(), scores)      # the accumulated order is the order fed
    assert np.array_equal(u32(acc["tpmask"])[:, :n], tp) and np.array_equal(u32(acc["igmask"])[:, :n], ig)
    T.initialize_ap()                                                   # starts over on the same buffers
    assert T.summary()["num_P"] == 0 and T.summary()["bev"]["hard"]["num_T"] == 0


def test_accumulator_overflow_raises_and_writes_nothing_past_the_capacity():
    scores, tp, ig = random_marks(300, 8300)
    T = harness(eval_max_detections=256)
    acc = T._accumulators(torch.device("cuda", torch.cuda.current_device()))
    feed(T, scores, tp, ig, np.array([0] * 7, np.int32), [100, 150, 50])
    with pytest.raises(RuntimeError, match="eval_max_detections"):
        T.summary()
    assert acc["scores"].shape[0] == 256 and acc["state"].cpu().tolist()[:4] == [300, 7, 7, 7]
    assert np.array_equal(acc["scores"].cpu().numpy(), scores[:256])
    # the two mask arrays are [2][256]: metric 0's tail is followed by metric 1's head, which must be metric 1's, not a spill
    assert np.array_equal(u32(acc["tpmask"]), tp[:, :256]) and np.array_equal(u32(acc["igmask"]), ig[:, :256])


# ------------------------------------------------------------------ end to end
def test_protocol_eval_step_on_device_equals_host_statement_and_leaves_the_plain_entries_alone():
    from test_gpu_model import build, tiny_input
    z = load_golden("model_tiny.npz")
    lz = load_golden("loss.npz")
    net, cfg = build(golden_cfg(z), "f32")
    cfg.update(score_threshold=0.5, eval_metric="ranked", eval_protocol="kitti", image_height=IH, image_width=IW)
    Tm = pkg("test")
    x = tiny_input().cuda()
    img = torch.zeros(x.shape[0], 3, 8, 8, dtype=torch.uint8, device="cuda")
    boxes, nb = torch.from_numpy(lz["bboxes"]), torch.from_numpy(lz["nbox"])
    B, R = boxes.shape[0], boxes.shape[1]
    with torch.no_grad():
        pred = net(x, img).clone()
    hw = pred.shape[2] * pred.shape[3]
    best = int(torch.argmax(pred[0, 1].flatten()))
    pred[0, 1].view(-1)[best] = float("nan")                            # a NaN score is never a candidate
    valid = boxes[:, :, 8] == 1
    centre = boxes[valid][:, :3].double().mean(0)
    crt = [torch.from_numpy(camera(float(centre[0]) - 12.0, float(centre[1]), float(centre[2]))), None][:B] + [None] * (B - 2)
    levels = (torch.arange(B * R).reshape(B, R) % 4).to(torch.int32)
    dontcare = torch.from_numpy(np.stack([rectangles(5, 8400 + b) for b in range(B)]))
    T, H = Tm.RankedTest(net, cfg), Tm.RankedTest(net, cfg)
    loss, cand = T.get_eval_value_onestep(x, img, boxes, nb, levels=levels, dontcare=dontcare, crt=crt)
    assert math.isfinite(loss)
    T.initialize_ap()
    for step in range(2):
        T.accumulate(pred, boxes, levels=levels, dontcare=dontcare, crt=crt)
        H.accumulate(pred.cpu(), boxes, levels=levels, dontcare=dontcare, crt=crt)
    hb, hs, hc, hk = H._last
    assert sum(hc.tolist()) > 0 and T._last[2].cpu().tolist() == hc.tolist()
    s = EK().settings(cfg)
    calib = pkg("calib")
    for b in range(B):
        nb_ = int(hc[b])
        C = calib.carla_crt() if crt[b] is None else crt[b].numpy()
        assert margins(hb[b, :nb_], hk[b], boxes[b].numpy(), C, dontcare[b].numpy(), s, 0.1) >= 1e-9
        assert T._last[3][b].cpu().numpy()[:nb_].tolist() == hk[b].tolist()
        for got, want in zip(T._last_marks[b], H._last_marks[b]):
            assert np.array_equal(u32(got)[..., :nb_], want)
    got, want = T.summary(), H.summary()
    assert got["num_P"] > 0 and want["bev"]["hard"]["num_T"] > want["bev"]["easy"]["num_T"] > 0
    same(got, want)
    # one plain-protocol batch in the same process still equals evalrank: the new kernels leave the old entries alone
    plain = dict(cfg, eval_protocol="plain")
    P, Q = Tm.RankedTest(net, plain), Tm.RankedTest(net, plain)
    P.accumulate(pred, boxes)
    Q.accumulate(pred.cpu(), boxes)
    gp, wp = P.summary(), Q.summary()
    assert "protocol" not in gp and gp["num_P"] == wp["num_P"] == got["num_P"] // 2 and gp["num_T"] == wp["num_T"] and gp["tp"] == wp["tp"]
    for t in THR:
        assert abs(gp["ap"][t] - wp["ap"][t]) <= 1e-12 and gp["precision"][t] == wp["precision"][t] and gp["recall"][t] == wp["recall"][t]
    assert P._acc["state"].numel() == 4 and "igmask" not in P._acc

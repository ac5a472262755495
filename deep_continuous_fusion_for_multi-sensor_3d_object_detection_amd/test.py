"""Drop-in counterpart of the reference's test.py `Test` class (the part train.py uses).

Test(net, config) puts the module in eval mode exactly like test.py:37 (which is why the
reference trains with eval-mode BatchNorm) and evaluates loss + score-threshold
counts for a batch.  The rotated-NMS / precision-recall post-processing (test.py:88-206; SURVEY.md
section 8(f) N2) keeps the reference's behaviour -- greedy suppression in INPUT order (no score sort), IoU
candidates shifted by 1e-4, touching rectangles suppress each other in the SAT flavour, and the aliased
per-box TP history (test.py:204 appends the same dict object every time) -- pinned by tests/golden/eval.npz.
Boxes that live on the GPU take the HIP kernels of csrc/evalpost.hip (score filter + compaction, pairwise overlap
matrix + one-wave greedy scan, bird's-eye-IoU matching); boxes handed over as host tensors take the numpy statement
of the same definitions (evalgeom.py), which is also what the device kernels are checked against.

RankedTest (`eval_metric: ranked`) is the evaluator the reference never built, next to the compat one:
suppression in score order on the (x, y) bird's-eye IoU, one-to-one matching against the labels and KITTI R40 average precision,
accumulated on the device and read once in summary().  evalrank.py is its host statement.  With `eval_protocol: kitti` (DESIGN.md
section 22; host statement evalkitti.py) it additionally reports bird's-eye and 3-D AP at easy / moderate / hard, with KITTI's
ignore rules; without the key it is what it was.
"""
import numpy as np
import torch
import torch.nn as nn

from . import evalgeom as EG
from . import evalkitti as EK
from . import evalrank as ER
from .loss import LossTotal


class Test(nn.Module):
    def __init__(self, pre_trained_net, config):
        super(Test, self).__init__()
        self.net = pre_trained_net
        self.net.eval()
        self.config = config
        self.loss_total = LossTotal(config)
        self.initialize_ap()

    IOU_threshold = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]

    def initialize_ap(self):
        self.num_T = 0
        self.num_P = 0
        self.num_TP_set = {t: 0 for t in self.IOU_threshold}
        self.num_TP_set_per_predbox = []
        self.loss_value = None

    def get_num_TP_set(self):
        return self.num_TP_set

    # ------------------------------------------------------------------ post-processing (host)
    @staticmethod
    def _np(box):
        return box.detach().cpu().numpy().astype(np.float64) if isinstance(box, torch.Tensor) else np.asarray(box, dtype=np.float64)

    def _nms(self, pred_bboxes, overlaps):
        """Greedy suppression in input order (test.py:110-175): a box survives iff it overlaps none of the survivors."""
        out = []
        for boxes in pred_bboxes:
            kept, kept_np = [], []
            for i in range(len(boxes)):
                cand = self._np(boxes[i])
                if all(not overlaps(cand, k) for k in kept_np):
                    kept.append(boxes[i])
                    kept_np.append(cand)
            out.append(kept)
        return out

    @staticmethod
    def _on_device(pred_bboxes):
        from .ops import EVAL_NMS_CAP
        ok = [isinstance(b, torch.Tensor) and b.is_cuda and b.dim() == 2 and b.shape[0] <= EVAL_NMS_CAP for b in pred_bboxes]
        return bool(ok) and all(ok)

    @staticmethod
    def _nms_device(pred_bboxes, mode, thr=0.01):
        from . import ops
        flags = [ops.eval_nms(b, mode, thr)[0] if b.shape[0] else None for b in pred_bboxes]
        out = []
        for b, f in zip(pred_bboxes, flags):
            idx = [] if f is None else torch.nonzero(f.cpu()).flatten().tolist()      # the one device -> host transfer
            out.append([b[i] for i in idx])
        return out

    def NMS_IOU(self, pred_bboxes, nms_iou_score_theshold=0.01):
        """test.py:110-140: 3-D IoU above the threshold suppresses; the survivor's centre is nudged by 1e-4 as there."""
        if self._on_device(pred_bboxes):
            return self._nms_device(pred_bboxes, "iou", nms_iou_score_theshold)

        def over(c, k):
            cc = EG.box_corners(c[:3], c[3:6], c[6])
            kc = EG.box_corners(k[:3] + 0.0001, k[3:6], k[6])
            return EG.rotated_iou(cc, kc)[0] > nms_iou_score_theshold
        return self._nms(pred_bboxes, over)

    def NMS_SAT(self, pred_bboxes):
        """test.py:142-175: any overlap (or contact) of the bird's-eye rectangles suppresses."""
        if self._on_device(pred_bboxes):
            return self._nms_device(pred_bboxes, "sat")

        def over(c, k):
            return EG.rects_overlap(EG.bev_rect(c[:2], c[3:5], c[6]), EG.bev_rect(k[:2], k[3:5], k[6]))
        return self._nms(pred_bboxes, over)

    def precision_recall_singleshot(self, pred_bboxes, ref_bboxes):
        """test.py:177-206: a predicted box is a true positive at threshold t if its bird's-eye IoU with any labelled
        box (last column == 1) exceeds t."""
        dev = [p for p in pred_bboxes if p is not None and len(p) and isinstance(p[0], torch.Tensor) and p[0].is_cuda]
        if dev:
            return self._precision_recall_device(pred_bboxes, ref_bboxes)
        for b in range(ref_bboxes.shape[0]):
            refs = [self._np(r) for r in ref_bboxes[b] if float(r[-1]) == 1]
            ref_c = [EG.box_corners(r[:3], r[3:6], r[6]) for r in refs]
            if pred_bboxes[b] is not None:
                for pb in pred_bboxes[b]:
                    self.num_P += 1
                    p = self._np(pb)
                    pc = EG.box_corners(p[:3], p[3:6], p[6])
                    hit = set()
                    for rc in ref_c:
                        iou2d = EG.rotated_iou(pc, rc)[1]
                        hit.update(t for t in self.IOU_threshold if iou2d > t)
                    for t in hit:
                        self.num_TP_set[t] += 1
                    self.num_TP_set_per_predbox.append(self.num_TP_set)      # same object every time, as in the reference
            self.num_T += len(refs)

    def _precision_recall_device(self, pred_bboxes, ref_bboxes):
        """The same counters from dcf_eval_match: one launch per sample, ten integers back at the end."""
        from . import ops
        device = next(p[0].device for p in pred_bboxes if p is not None and len(p))
        thr = torch.tensor(self.IOU_threshold, dtype=torch.float64, device=device)
        tp = torch.zeros(len(self.IOU_threshold), dtype=torch.int32, device=device)
        refs_dev = ref_bboxes.to(device=device, dtype=torch.float32)
        for b in range(ref_bboxes.shape[0]):
            kept = pred_bboxes[b]
            if kept is not None and len(kept):
                ops.eval_match(torch.stack([k.float() for k in kept], 0), refs_dev[b], thr, tp)
                self.num_P += len(kept)
                self.num_TP_set_per_predbox.extend([self.num_TP_set] * len(kept))   # same object every time, as in the reference
            self.num_T += int((ref_bboxes[b][:, -1] == 1).sum())
        for t, v in zip(self.IOU_threshold, tp.cpu().tolist()):
            self.num_TP_set[t] += v

    def display_average_precision(self, plot_AP_graph=False):
        """test.py:208-242 without the matplotlib file output: (precision, recall) curves per IoU threshold."""
        precisions = {t: [1] for t in self.IOU_threshold}
        recalls = {t: [0] for t in self.IOU_threshold}
        for n, tp in enumerate(self.num_TP_set_per_predbox, 1):
            for t in self.IOU_threshold:
                precisions[t].append(tp[t] / n)
                recalls[t].append(tp[t] / self.num_T)
        self.total_precision = {t: self.num_TP_set[t] / (self.num_P + 0.01) for t in self.IOU_threshold}
        self.total_recall = {t: self.num_TP_set[t] / (self.num_T + 0.01) for t in self.IOU_threshold}
        return precisions, recalls

    def get_num_T(self):
        return self.num_T

    def get_num_P(self):
        return self.num_P

    def get_bboxes_device(self, pred, score_threshold=None):
        """test.py:88-108 as one launch (dcf_eval_score_filter) on the model output pred [B,32,h,w]: [n,7] boxes per sample,
        anchor 0's in raster order, then anchor 1's.  Falls back to get_bboxes when a sample has more than 4096 candidates."""
        from . import ops
        thr = self.config["score_threshold"] if score_threshold is None else score_threshold
        boxes, count = ops.eval_score_filter(pred, thr)
        n = count.cpu().tolist()
        if max(n) > boxes.shape[1]:
            _, _, pb = torch.split(pred, [4, 14, 14], dim=1)
            return self.get_bboxes(pred[:, 0:4], pb, thr)
        return [boxes[b, :n[b]] for b in range(pred.shape[0])]

    def get_bboxes(self, pred_cls, pred_bbox, score_threshold=None):
        """test.py:88-108: anchors whose positive-class score exceeds the threshold -> [n,7] boxes per sample."""
        thr = self.config["score_threshold"] if score_threshold is None else score_threshold
        out = []
        for b in range(pred_cls.shape[0]):
            boxes = []
            for a in range(2):
                mask = pred_cls[b, 2 * a + 1] > thr
                boxes.append(pred_bbox[b, 7 * a:7 * a + 7][:, mask].t())
            out.append(torch.cat(boxes, 0))
        return out

    def get_eval_value_onestep(self, lidar_voxel, camera_image, object_data, num_ref_box, **extra):
        with torch.no_grad():
            pred = self.net(lidar_voxel, camera_image, **extra)
            pred_cls, pred_reg, pred_bbox = torch.split(pred, [4, 14, 14], dim=1)
            self.loss_value = self.loss_total(object_data.to(pred.device), num_ref_box, pred_cls, pred_reg)
            boxes = self.get_bboxes_device(pred) if pred.is_cuda else self.get_bboxes(pred_cls, pred_bbox)
        # test.py:84-86: SAT suppression, then the precision / recall counters (on the device when the boxes are there and a
        # sample has at most 4096 candidates; the numpy statement otherwise)
        if not self._on_device(boxes):
            boxes_nms = [b.float().cpu() for b in boxes]
        else:
            boxes_nms = boxes
        self.refined_bbox = self.NMS_SAT(boxes_nms)
        self.precision_recall_singleshot(self.refined_bbox, object_data.detach().float().cpu())
        return self.loss_value.item(), boxes


class RankedTest(Test):
    """`eval_metric: ranked`: candidates ranked by score, greedy suppression on the (x, y) bird's-eye IoU, one-to-one matching per
    IoU threshold, KITTI R40 average precision (definitions: evalrank.py).  accumulate() enqueues one batch on the device without
    waiting for it; summary() is the one synchronisation.  CPU tensors take the numpy statement."""

    def __init__(self, pre_trained_net, config):
        if EK.protocol(config) == "kitti":                      # bad values raise here, not in the first batch
            EK.settings(config, self.IOU_threshold)
        super(RankedTest, self).__init__(pre_trained_net, config)

    def _settings(self):
        c = self.config
        thr = c.get("eval_score_threshold")
        return (float(c["score_threshold"] if thr is None else thr), float(c.get("eval_nms_iou", 0.1)),
                int(c.get("eval_max_candidates", 4096)), int(c.get("eval_max_detections", 131072)))

    def _kitti(self):
        """The validated settings of `eval_protocol: kitti`, or None under the plain protocol."""
        if (self.config.get("eval_protocol") or "plain") == "plain":
            return None
        EK.protocol(self.config)
        return EK.settings(self.config, self.IOU_threshold)

    def initialize_ap(self):
        super(RankedTest, self).initialize_ap()
        self._last = None
        self._summary = None
        acc = getattr(self, "_acc", None)
        if acc is not None:                                     # allocated lazily by the first accumulate()
            if acc["device"].type == "cuda":
                acc["state"].zero_()
            else:
                acc["state"][:] = 0

    def _accumulators(self, device):
        cap = self._settings()[3]
        acc = getattr(self, "_acc", None)
        kitti = self._kitti() is not None
        if acc is None or acc["device"] != device or acc["scores"].shape[0] != cap or ("igmask" in acc) != kitti:
            if kitti and device.type == "cuda":
                acc = {"device": device, "scores": torch.zeros(cap, dtype=torch.float32, device=device),
                       "tpmask": torch.zeros((2, cap), dtype=torch.int32, device=device), "igmask": torch.zeros((2, cap), dtype=torch.int32, device=device),
                       "state": torch.zeros(8, dtype=torch.int64, device=device),
                       "thr": torch.tensor(self.IOU_threshold, dtype=torch.float64, device=device)}
            elif kitti:
                acc = {"device": device, "scores": np.zeros(cap, dtype=np.float32), "tpmask": np.zeros((2, cap), dtype=np.uint32),
                       "igmask": np.zeros((2, cap), dtype=np.uint32), "state": np.zeros(8, dtype=np.int64)}
            elif device.type == "cuda":
                acc = {"device": device, "scores": torch.zeros(cap, dtype=torch.float32, device=device),
                       "tpmask": torch.zeros(cap, dtype=torch.int32, device=device), "state": torch.zeros(4, dtype=torch.int64, device=device),
                       "thr": torch.tensor(self.IOU_threshold, dtype=torch.float64, device=device)}
            else:
                acc = {"device": device, "scores": np.zeros(cap, dtype=np.float32), "tpmask": np.zeros(cap, dtype=np.uint32),
                       "state": np.zeros(4, dtype=np.int64)}
            self._acc = acc
        return acc

    def accumulate(self, pred, object_data, levels=None, dontcare=None, crt=None):
        """One batch: rank filter, then per sample suppression, matching and the append to the accumulators.  pred [B,32,h,w] fp32
        (the model output), object_data [B,R,9] label rows.  Nothing here waits for the device.
        Under `eval_protocol: kitti` also levels [B,R] (absent: every row level 0), dontcare [B,D,4] image rectangles (absent: none) and
        crt, per sample the [4,3] host matrix the frame is projected with (absent or None: calib.carla_crt(), FrameGeometry's default)."""
        if self._kitti() is not None:
            return self._accumulate_kitti(pred, object_data, levels, dontcare, crt)
        thr, nms_iou, cap, _ = self._settings()
        acc = self._accumulators(pred.device)
        self._summary = None
        if pred.is_cuda:
            from . import ops
            refs = object_data.to(device=pred.device, dtype=torch.float32).contiguous()
            boxes, scores, count, total = ops.eval_rank_filter(pred.float(), thr, cap)
            keeps = []
            for b in range(pred.shape[0]):
                keep, _ = ops.eval_nms(boxes[b], "bev", nms_iou, count=count[b:b + 1])
                tpmask = ops.eval_match_ranked(boxes[b], keep, count[b:b + 1], refs[b], acc["thr"])
                ops.eval_accumulate(scores[b], tpmask, keep, count[b:b + 1], total[b:b + 1], refs[b], acc["scores"], acc["tpmask"], acc["state"])
                keeps.append(keep)
            self._last = (boxes, scores, count, keeps)
            return boxes, count
        refs = object_data.detach().float().numpy()
        boxes, scores, count, total = ER.rank_filter(pred.detach().float().numpy(), thr, cap)
        keeps = []
        st, capd = acc["state"], acc["scores"].shape[0]
        for b in range(pred.shape[0]):
            n = int(count[b])
            keep = ER.nms(boxes[b, :n], nms_iou)
            tpmask = ER.match(boxes[b, :n], keep, refs[b], self.IOU_threshold)
            for i in np.nonzero(keep)[0]:
                if st[0] < capd:
                    acc["scores"][st[0]], acc["tpmask"][st[0]] = scores[b, i], tpmask[i]
                st[0] += 1                                      # keeps counting past the capacity: summary() raises
            st[1] += int((refs[b][:, 8] == 1).sum())
            st[2] += int(total[b] > cap)
            keeps.append(keep)
        self._last = (boxes, scores, count, keeps)
        return boxes, count

    def _accumulate_kitti(self, pred, object_data, levels, dontcare, crt):
        """accumulate() under `eval_protocol: kitti`: per sample the flags, both IoU matrices, the 2 x 3 x 10 matchings, the append."""
        from . import calib
        s = self._kitti()
        thr, nms_iou, cap, _ = self._settings()
        acc = self._accumulators(pred.device)
        self._summary = None
        B = pred.shape[0]
        H, W = int(self.config["image_height"]), int(self.config["image_width"])
        mats = [None if (crt is None or crt[b] is None) else crt[b] for b in range(B)]
        mats = [calib.carla_crt() if m is None else (m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m) for m in mats]
        mats = [np.ascontiguousarray(m, dtype=np.float32).reshape(4, 3) for m in mats]
        keeps, marks = [], []
        if pred.is_cuda:
            from . import ops
            dev = pred.device
            refs = object_data.to(device=dev, dtype=torch.float32).contiguous()
            lv = None if levels is None else levels.to(device=dev, dtype=torch.int32).contiguous()
            dc = None if dontcare is None else dontcare.to(device=dev, dtype=torch.float32).contiguous()
            boxes, scores, count, total = ops.eval_rank_filter(pred.float(), thr, cap)
            for b in range(B):
                cnt, lvb = count[b:b + 1], None if lv is None else lv[b]
                keep, _ = ops.eval_nms(boxes[b], "bev", nms_iou, count=cnt)
                flags = ops.eval_det_flags(boxes[b], cnt, mats[b], None if dc is None else dc[b], H, W, s["min_height"], s["dontcare_overlap"])
                bev, i3d = ops.eval_iou_levels(boxes[b], keep, cnt, refs[b])
                tpm, igm = ops.eval_match_levels(bev, i3d, keep, cnt, refs[b], lvb, flags, acc["thr"])
                ops.eval_accumulate_levels(scores[b], tpm, igm, keep, cnt, total[b:b + 1], refs[b], lvb, acc["scores"], acc["tpmask"], acc["igmask"], acc["state"])
                keeps.append(keep)
                marks.append((flags, tpm, igm))
            self._last, self._last_marks = (boxes, scores, count, keeps), marks
            return boxes, count
        refs = object_data.detach().float().numpy()
        lv = None if levels is None else levels.detach().numpy() if isinstance(levels, torch.Tensor) else np.asarray(levels)
        dc = None if dontcare is None else dontcare.detach().float().numpy() if isinstance(dontcare, torch.Tensor) else np.asarray(dontcare, np.float32)
        boxes, scores, count, total = ER.rank_filter(pred.detach().float().numpy(), thr, cap)
        st, capd = acc["state"], acc["scores"].shape[0]
        for b in range(B):
            n = int(count[b])
            lvb = None if lv is None else lv[b]
            keep = ER.nms(boxes[b, :n], nms_iou)
            flags = EK.det_flags(boxes[b, :n], mats[b], H, W, None if dc is None else dc[b], s)
            bev, i3d = EK.iou_matrices(boxes[b, :n], keep, refs[b])
            tpm, igm = EK.match_levels(keep, refs[b], lvb, bev, i3d, flags, self.IOU_threshold)
            for i in np.nonzero(keep)[0]:
                if st[0] < capd:
                    acc["scores"][st[0]], acc["tpmask"][:, st[0]], acc["igmask"][:, st[0]] = scores[b, i], tpm[:, i], igm[:, i]
                st[0] += 1                                      # keeps counting past the capacity: summary() raises
            st[1:4] += EK.count_rows(refs[b], lvb)
            st[4] += int(total[b] > cap)
            keeps.append(keep)
            marks.append((flags, tpm, igm))
        self._last, self._last_marks = (boxes, scores, count, keeps), marks
        return boxes, count

    def _summary_kitti(self):
        acc = getattr(self, "_acc", None)
        thr = self.IOU_threshold
        if acc is None or "igmask" not in acc:
            return EK.summarize(np.zeros(0, np.float32), np.zeros((2, 0), np.uint32), np.zeros((2, 0), np.uint32), [0, 0, 0], thr)
        if acc["device"].type == "cuda":
            from . import ops
            ap, tp, ig = ops.eval_ap_levels(acc["scores"], acc["tpmask"], acc["igmask"], acc["state"], len(thr))
            state = acc["state"].cpu().tolist()
            self._check_capacity(state[0], acc["scores"].shape[0])
            return EK.assemble(ap.cpu().numpy(), tp.cpu().numpy(), ig.cpu().numpy(), state[0], state[1:4], thr, state[4])
        state = acc["state"].tolist()
        self._check_capacity(state[0], acc["scores"].shape[0])
        return EK.summarize(acc["scores"][:state[0]], acc["tpmask"][:, :state[0]], acc["igmask"][:, :state[0]], state[1:4], thr, state[4])

    def summary(self):
        """The one synchronisation: average precision per IoU threshold (KITTI R40), their mean, and the totals.  Under
        `eval_protocol: kitti` the dictionary of evalkitti.assemble: the same per metric ("bev", "3d") and level ("easy", "moderate",
        "hard"); num_T / num_P / num_TP_set then report the bird's-eye moderate values."""
        if self._summary is not None:
            return self._summary
        if self._kitti() is not None:
            out = self._summary_kitti()
            mod = out["bev"]["moderate"]
            self.num_P, self.num_T = out["num_P"], mod["num_T"]
            self.num_TP_set = dict(mod["tp"])
            self._summary = out
            return out
        acc = getattr(self, "_acc", None)
        thr = self.IOU_threshold
        if acc is None:
            out = ER.summarize(np.zeros(0, np.float32), np.zeros(0, np.uint32), 0, thr)
        elif acc["device"].type == "cuda":
            from . import ops
            ap, tp = ops.eval_ap(acc["scores"], acc["tpmask"], acc["state"], len(thr))
            state = acc["state"].cpu().tolist()
            self._check_capacity(state[0], acc["scores"].shape[0])
            out = ER.assemble(ap.cpu().numpy(), tp.cpu().numpy(), state[0], state[1], thr, state[2])
        else:
            state = acc["state"].tolist()
            self._check_capacity(state[0], acc["scores"].shape[0])
            out = ER.summarize(acc["scores"][:state[0]], acc["tpmask"][:state[0]], state[1], thr, state[2])
        self.num_P, self.num_T = out["num_P"], out["num_T"]
        self.num_TP_set = dict(out["tp"])
        self._summary = out
        return out

    @staticmethod
    def _check_capacity(cursor, capacity):
        if cursor > capacity:
            raise RuntimeError("RankedTest: %d detections accumulated, eval_max_detections holds %d: raise it (nothing is dropped silently)"
                               % (cursor, capacity))

    def get_num_TP_set(self):
        self.summary()
        return self.num_TP_set

    def get_num_T(self):
        self.summary()
        return self.num_T

    def get_num_P(self):
        self.summary()
        return self.num_P

    def detections(self):
        """Per sample (boxes [k,7], scores [k]) of the last batch's survivors, in rank order.  Synchronises: for inspection."""
        if self._last is None:
            return []
        boxes, scores, count, keeps = self._last
        out = []
        for b in range(len(keeps)):
            if isinstance(boxes, torch.Tensor):
                sel = keeps[b].bool()
                sel[int(count[b]):] = False
                out.append((boxes[b][sel], scores[b][sel]))
            else:
                sel = np.zeros(boxes.shape[1], dtype=bool)
                sel[:len(keeps[b])] = keeps[b] != 0
                out.append((torch.from_numpy(boxes[b][sel]), torch.from_numpy(scores[b][sel])))
        return out

    def get_eval_value_onestep(self, lidar_voxel, camera_image, object_data, num_ref_box, levels=None, dontcare=None, crt=None, **extra):
        """levels / dontcare / crt: the protocol's optional inputs (accumulate()); they do not reach the network."""
        with torch.no_grad():
            pred = self.net(lidar_voxel, camera_image, **extra)
            pred_cls, pred_reg, pred_bbox = torch.split(pred, [4, 14, 14], dim=1)
            self.loss_value = self.loss_total(object_data.to(pred.device), num_ref_box, pred_cls, pred_reg)
            boxes, count = self.accumulate(pred, object_data, levels=levels, dontcare=dontcare, crt=crt)
        value = self.loss_value.item()                          # the caller's loss value: the step's one wait, after everything is enqueued
        n = count.cpu().tolist() if isinstance(count, torch.Tensor) else count.tolist()
        cand = [boxes[b, :n[b]] if isinstance(boxes, torch.Tensor) else torch.from_numpy(boxes[b, :n[b]]) for b in range(pred.shape[0])]
        return value, cand

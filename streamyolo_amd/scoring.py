"""COCO-style scoring of detections on the device: the sAP / AP numbers without pycocotools.

Mirrors, for boxes, what the reference gets from `COCOeval(...).evaluate(); accumulate(); summarize()`:
  DetectionScorer   the evaluator's state on the device: ticks append their detections and ground truth with no host read
                    (sy_score_match, csrc/score.hip), one summarize() runs sy_score_accumulate and reads the result
  score_coco()      sAP/det/__init__.py::eval_ccf (:180-195) for COCO-format rows (streaming.pair_with_ground_truth,
                    streaming.convert_to_coco_format) and annotation dicts — through the same scorer

The evaluation parameters are COCOeval's own, computed here on the host exactly as pycocotools' Params does and handed to the
kernels as data.  PyTorch is used for memory and streams only.
"""
import numpy as np
import torch

from . import _lib, ops

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]      # all, small, medium, large
MAX_DETS = [1, 10, 100]
EPS = np.spacing(1)
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def summarize_arrays(precision, recall):
    """COCOeval.summarize's twelve numbers from precision [T, R, K, A, M] and recall [T, K, A, M] (numpy, host)."""
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    last = len(MAX_DETS) - 1
    out = {"AP": mean(precision[:, :, :, 0, last]), "AP50": mean(precision[0, :, :, 0, last]),
           "AP75": mean(precision[5, :, :, 0, last]), "APs": mean(precision[:, :, :, 1, last]),
           "APm": mean(precision[:, :, :, 2, last]), "APl": mean(precision[:, :, :, 3, last]),
           "AR1": mean(recall[:, :, 0, 0]), "AR10": mean(recall[:, :, 0, 1]), "AR100": mean(recall[:, :, 0, 2]),
           "ARs": mean(recall[:, :, 1, last]), "ARm": mean(recall[:, :, 2, last]), "ARl": mean(recall[:, :, 3, last])}
    return out


class DetectionScorer:
    """COCOeval for boxes with its state on the device.

    add() appends the rows of one tick (or of any batch) as the next images; it launches one kernel on the current stream
    and reads nothing back.  summarize() sorts and accumulates on the device, performs the evaluation's only host read and
    returns the twelve COCOeval statistics plus the `precision` [10, 101, K, 4, 3] and `recall` [10, K, 4, 3] arrays.

    capacity: detection records kept per class (an image contributes at most 100 per class); when a class runs out of room
    the records are dropped and counted, and summarize() raises.  max_gt: ground truths per image, at most 256.  Scores must
    be >= 0 (products of sigmoids here)."""

    def __init__(self, num_classes=8, capacity=1 << 16, max_gt=64, device="cuda"):
        if not 1 <= int(max_gt) <= _lib.SCORE_MAX_GT:
            raise ValueError("DetectionScorer: max_gt must be in 1..%d, got %r" % (_lib.SCORE_MAX_GT, max_gt))
        self.num_classes, self.capacity, self.max_gt = int(num_classes), int(capacity), int(max_gt)
        self.device = torch.device(device)
        self.params = ops.score_params(IOU_THRS, REC_THRS, AREA_RNG, MAX_DETS, EPS)
        self.state = torch.zeros(ops.score_state_bytes(self.num_classes, self.capacity), dtype=torch.uint8, device=self.device)
        self._workspace = None
        self.images = 0
        self.reset()

    def reset(self):
        """Forget every image added so far."""
        ops.score_reset(self.state, self.num_classes, self.capacity)
        self.images = 0

    def add(self, det, cnt, gt, gt_cnt, divisor=None, rows=None, layout="nms"):
        """Rows 0..rows-1 (default: all) become the next images, in order.  det / cnt: device tensors as detect_device returns
        them (layout "nms": det [B, D, 7]) or as the tracker writes them (layout "track": out [B, T, 6] / out_cnt; "xywh": the
        same with x, y, w, h in the first four columns, as COCO result rows carry them); divisor:
        None or the float32 [B] tensor whose entry divides the row's coordinates (camera coordinates = network / divisor); gt
        float64 [B, <= max_gt, 7] = x, y, w, h, class, iscrowd, area in the detections' final coordinates, gt_cnt int32 [B].
        No host read, no synchronisation; not part of any launch tape."""
        if layout not in _lib.SCORE_LAYOUT:
            raise ValueError("DetectionScorer: layout must be one of %s, got %r" % (sorted(_lib.SCORE_LAYOUT), layout))
        n = det.shape[0] if rows is None else int(rows)
        if gt.dim() != 3 or gt.shape[1] > self.max_gt:
            raise ValueError("DetectionScorer: gt must be [B, <= %d, 7], got %r" % (self.max_gt, tuple(gt.shape)))
        ops.score_match(det, cnt, gt, gt_cnt, self.images, self.params, self.state, self.num_classes, self.capacity,
                        divisor=divisor, rows=n, layout=layout)
        self.images += n

    def counters(self):
        """(used [K], npig [K, 4], overflow) as host numbers: one host read."""
        K = self.num_classes
        hdr = self.state[:(5 * K + 1) * 4].cpu().numpy().view(np.int32)
        return hdr[:K].copy(), hdr[K:5 * K].reshape(K, 4).copy(), int(hdr[5 * K])

    def summarize(self):
        K = self.num_classes
        if self._workspace is None:
            self._workspace = torch.empty(ops.score_workspace_bytes(K, self.capacity), dtype=torch.uint8, device=self.device)
        T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
        # one buffer, one copy: precision, recall, then the overflow counter, which the accumulate launch writes as a double
        n_p, n_r = T * R * K * A * M, T * K * A * M
        buf = torch.empty(n_p + n_r + 1, dtype=torch.float64, device=self.device)
        ops.score_accumulate(self.state, K, self.capacity, self.params, self._workspace, buf[:n_p].view(T, R, K, A, M),
                             buf[n_p:n_p + n_r].view(T, K, A, M), overflow=buf[n_p + n_r:])
        host = buf.cpu().numpy()
        overflow = int(host[-1])
        if overflow:
            raise RuntimeError("DetectionScorer: %d detection records did not fit (capacity %d per class): the statistics "
                               "would be wrong" % (overflow, self.capacity))
        precision, recall = host[:n_p].reshape(T, R, K, A, M).copy(), host[n_p:n_p + n_r].reshape(T, K, A, M).copy()
        out = summarize_arrays(precision, recall)
        out["precision"], out["recall"] = precision, recall
        return out


def score_coco(results, annotations, class_ids, image_ids=None, device=None, batch=64):
    """eval_ccf(db, results) without pycocotools, for boxes.  results: rows with image_id, bbox (xywh), score, category_id, as
    streaming.pair_with_ground_truth and streaming.convert_to_coco_format return them; annotations: COCO annotation dicts
    (image_id, bbox, category_id, optional iscrowd, optional area: default w * h); class_ids: the dataset's category ids, the
    position in this list is the class.  Images are scored in ascending image_id: `image_ids` when given, else those of the
    annotations.  A result on an unknown image is a ValueError; rows of a category outside class_ids are left out, as
    COCOeval leaves them.  Returns DetectionScorer.summarize()'s dict."""
    if device is None:
        device = "cpu" if _lib.is_emulator() else "cuda"
    ids = sorted(set(int(i) for i in image_ids) if image_ids is not None else set(int(a["image_id"]) for a in annotations))
    pos = {i: n for n, i in enumerate(ids)}
    cls = {c: n for n, c in enumerate(class_ids)}
    dets, gts = [[] for _ in ids], [[] for _ in ids]
    for r in results:
        n = pos.get(int(r["image_id"]))
        if n is None:
            raise ValueError("score_coco: result on unknown image_id %r" % (r["image_id"],))
        k = cls.get(int(r["category_id"]))
        if k is None:
            continue
        x, y, w, h = (np.float32(v) for v in np.asarray(r["bbox"], dtype=np.float64)[:4])
        score = np.float32(r["score"]) + np.float32(0.0)         # (-0.0 becomes 0.0)
        if not score >= 0:                                      # (NaN too: the device orders scores by their bits)
            raise ValueError("score_coco: score %r on image_id %r; scores must be >= 0" % (r["score"], r["image_id"]))
        dets[n].append((x, y, w, h, score, k))
    for a in annotations:
        n = pos.get(int(a["image_id"]))
        k = cls.get(int(a["category_id"]))
        if n is None or k is None:
            continue
        x, y, w, h = (float(v) for v in a["bbox"][:4])
        gts[n].append((x, y, w, h, k, float(bool(a.get("iscrowd", 0))), float(a["area"]) if "area" in a else w * h))
    D, G = max([len(d) for d in dets] + [1]), max([len(g) for g in gts] + [1])
    per_class = np.zeros(len(class_ids), dtype=np.int64)
    for d in dets:
        c = np.bincount([r[5] for r in d], minlength=len(class_ids)) if d else np.zeros(len(class_ids), dtype=np.int64)
        per_class += np.minimum(c, _lib.SCORE_MAX_DET)
    scorer = DetectionScorer(len(class_ids), capacity=max(int(per_class.max()), 1), max_gt=G, device=device)
    for n0 in range(0, len(ids), batch):
        n1 = min(n0 + batch, len(ids))
        det = np.zeros((n1 - n0, D, 6), dtype=np.float32)        # the "xywh" layout: the rows' own x, y, w, h as float32
        gt = np.zeros((n1 - n0, G, 7), dtype=np.float64)
        cnt, gcnt = np.zeros(n1 - n0, dtype=np.int32), np.zeros(n1 - n0, dtype=np.int32)
        for b, n in enumerate(range(n0, n1)):
            cnt[b], gcnt[b] = len(dets[n]), len(gts[n])
            if dets[n]:
                det[b, :len(dets[n])] = dets[n]
            if gts[n]:
                gt[b, :len(gts[n])] = gts[n]
        scorer.add(torch.from_numpy(det).to(scorer.device), torch.from_numpy(cnt).to(scorer.device),
                   torch.from_numpy(gt).to(scorer.device), torch.from_numpy(gcnt).to(scorer.device), layout="xywh")
    return scorer.summarize()

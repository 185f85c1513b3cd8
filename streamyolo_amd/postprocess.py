"""postprocess — drop-in for yolox.utils.postprocess as the reference calls it
(exps/evaluators/onex_stream_evaluator.py:148-150) and for the inline `inference()` of
sAP/streamyolo/streamyolo_det.py:62-83: confidence filter + NMS on the device (class-aware: sy_postprocess;
class-agnostic: sy_postprocess_rows with a uniform policy table), one host read of the per-image counts at
the end (the reference's `.cpu()`).  DetectionPolicy is what one batch row of sy_postprocess_rows may ask for."""
import math
import operator

import torch

from . import ops
from ._lib import DET_MAX_CLASSES

_ws_cache = {}


class DetectionPolicy:
    """What counts as a detection for one camera stream (one sy_det_policy row of sy_postprocess_rows):

        conf_thre, nms_thresh   the thresholds; None = the detector's own
        classes                 iterable of the class ids that are reported; None = all; empty = nothing is reported.  A box of
                                another class is removed before the NMS: it suppresses nothing
        class_agnostic          NMS over the raw boxes whatever their classes (torchvision.ops.nms), as
                                yolox.utils.postprocess(class_agnostic=True)
        max_candidates          only the best-scoring max_candidates candidates enter the NMS; None = all
        max_det                 at most this many detections (the best ones) are returned; None = all

    ValueError for a threshold that is not finite, nms_thresh < 0 or a cap below 1; class ids are checked against the detector's
    num_classes where the policy is given to one (record())."""

    def __init__(self, conf_thre=None, nms_thresh=None, classes=None, class_agnostic=False, max_candidates=None, max_det=None):
        def number(name, v):
            try:
                f = float(v)
            except (TypeError, ValueError):
                f = math.nan
            if isinstance(v, bool) or not math.isfinite(f):
                raise ValueError("DetectionPolicy: %s must be a finite number or None, got %r" % (name, v))
            return f

        def integer(name, v, lo):
            try:
                i = None if isinstance(v, bool) else operator.index(v)
            except TypeError:
                i = None
            if i is None or not lo <= i < 2 ** 31:
                raise ValueError("DetectionPolicy: %s must be an integer >= %d, got %r" % (name, lo, v))
            return i
        self.conf_thre = None if conf_thre is None else number("conf_thre", conf_thre)
        self.nms_thresh = None if nms_thresh is None else number("nms_thresh", nms_thresh)
        if self.nms_thresh is not None and self.nms_thresh < 0:
            raise ValueError("DetectionPolicy: nms_thresh must be >= 0, got %r" % (nms_thresh,))
        self.max_candidates = None if max_candidates is None else integer("max_candidates", max_candidates, 1)
        self.max_det = None if max_det is None else integer("max_det", max_det, 1)
        if classes is not None:
            classes = tuple(sorted(set(integer("a class id", c, 0) for c in classes)))
        self.classes, self.class_agnostic = classes, bool(class_agnostic)

    def __repr__(self):
        return "DetectionPolicy(conf_thre=%r, nms_thresh=%r, classes=%r, class_agnostic=%r, max_candidates=%r, max_det=%r)" % (
            self.conf_thre, self.nms_thresh, self.classes, self.class_agnostic, self.max_candidates, self.max_det)

    def record(self, num_classes, conf_thre, nms_thresh):
        """The sy_det_policy tuple (ops.det_policy_record) of this policy on a detector with the given class count and default
        thresholds.  ValueError for a class id outside [0, num_classes) or defaults that are no valid thresholds."""
        if not 1 <= int(num_classes) <= DET_MAX_CLASSES:
            raise ValueError("DetectionPolicy: num_classes must be in 1..%d, got %r" % (DET_MAX_CLASSES, num_classes))
        conf = self.conf_thre if self.conf_thre is not None else float(conf_thre)
        nms = self.nms_thresh if self.nms_thresh is not None else float(nms_thresh)
        if not (math.isfinite(conf) and math.isfinite(nms) and nms >= 0):
            raise ValueError("DetectionPolicy: thresholds must be finite and nms_thresh >= 0, got %r / %r" % (conf, nms))
        if self.classes is not None and any(c >= num_classes for c in self.classes):
            raise ValueError("DetectionPolicy: class ids must lie in [0, %d), got %r" % (num_classes, self.classes))
        classes = range(int(num_classes)) if self.classes is None else self.classes
        return ops.det_policy_record(conf, nms, classes, self.class_agnostic, self.max_candidates or 0, self.max_det or 0)


def _as_policy(policy):
    """policy argument of the detectors -> DetectionPolicy (True / None: the defaults); ValueError for anything else."""
    if policy is None or policy is True:
        return DetectionPolicy()
    if not isinstance(policy, DetectionPolicy):
        raise ValueError("policy must be a DetectionPolicy, got %r" % (policy,))
    return policy


def postprocess_device(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
    """No host synchronisation in the class-aware mode: returns (det [B,A,7], anchor_index [B,A], count [B]) device tensors.
    class_agnostic=True goes through sy_postprocess_rows with the same policy row for every image (its small table is
    copied to the device first)."""
    pred = prediction.float().contiguous()
    key = (pred.shape[0], pred.shape[1], str(pred.device))
    ws = _ws_cache.get(key)
    if ws is None:
        ws = ops.PostprocessWorkspace(pred.shape[0], pred.shape[1], pred.device)
        _ws_cache[key] = ws
    if class_agnostic:
        row = DetectionPolicy(class_agnostic=True).record(num_classes, conf_thre, nms_thre)
        return ops.postprocess_rows(pred, num_classes, ops.det_policy_table([row] * pred.shape[0], pred.device), ws)
    return ops.postprocess(pred, num_classes, conf_thre, nms_thre, ws)


def postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
    """List (one entry per image) of [n,7] tensors (x1,y1,x2,y2,obj,class_conf,class_pred) in
    descending score order, or None when nothing survives — as yolox.utils.postprocess returns.
    Like the reference it also rewrites prediction[..., :4] to corner form in place."""
    det, idx, cnt = postprocess_device(prediction, num_classes, conf_thre, nms_thre, class_agnostic)
    counts = cnt.cpu().tolist()
    if prediction.dtype == torch.float32 and prediction.is_contiguous() and prediction.dim() == 3:
        ops.head_decode(prediction, boxes=False, corners=True)          # one launch (sy_head_decode, flag 4)
    else:                                                               # a caller's half / strided tensor: its own dtype's arithmetic
        cx, cy, w, h = prediction[..., 0].clone(), prediction[..., 1].clone(), prediction[..., 2].clone(), prediction[..., 3].clone()
        prediction[..., 0], prediction[..., 1] = cx - w / 2, cy - h / 2
        prediction[..., 2], prediction[..., 3] = cx + w / 2, cy + h / 2
    return [det[i, :n].clone().to(prediction.dtype) if n else None for i, n in enumerate(counts)]

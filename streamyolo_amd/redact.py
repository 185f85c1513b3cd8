"""Redact detected objects in camera surfaces on the device (csrc/redact.hip, sy_redact): hand a frame on — to a recorder, a
monitor wall, a dataset export — WITHOUT the people and vehicles in it, and without pulling the boxes to the host, pixelating a
host copy of the frame and uploading it again.

  RedactSpec                        what a redaction looks like: pixelate or fill, cell size, rectangle or ellipse, padding,
                                    class filter, minimum score; validated on the host
  MultiStreamDetector.redact()      the latest tick's results of some streams in the targets given, ONE launch on the current
  StreamingDetector.redact()        stream behind the tick, no host read, not on the tick's tape (streaming.py)
  redact_detections()               the stand-alone form for any boxes in the target's own pixel coordinates

The rule (rectangle, padding, shape, union, fill, pixelation, chroma, untouched bytes) is stated once, in
include/streamyolo_hip.h.  EVERY list entry is looked at — there is no cap of 256 as in drawing and cropping: coverage is a
union, and an entry dropped is an object exposed.  With tracking the tracker's forecast lists are redacted, which survive a missed
detection: a single flickered frame would otherwise expose the object.

WARNING — redaction is IN PLACE.  A hardware decoder keeps the surfaces it still needs as reference frames for the pictures that
follow; redacting one corrupts every frame predicted from it.  Never redact a decoder surface that the decoder may still hold:
redact a copy,

    det.redact([s.clone() for s in surfaces], sids)

(`Surface.clone()`: same format, sizes and pitches, its own memory), or surfaces the decoder has released.

ORDER — redact() before draw().  Drawn outlines and label tabs inside a box would be pixelated with it; redacted first, the
drawing lies on top and stays legible:

    out = [s.clone() for s in surfaces]
    det.redact(out, sids)
    det.draw(out, sids)
"""
import math
import operator

import numpy as np
import torch

from . import ops
from ._lib import DET_MAX_CLASSES, REDACT_CELLS, REDACT_ELLIPSE, REDACT_FILL, REDACT_PIXELATE, REDACT_RECT
from .overlay import OverlayRows, as_target, palette_rows

_MODES = {"pixelate": REDACT_PIXELATE, "fill": REDACT_FILL}
_SHAPES = {"rect": REDACT_RECT, "ellipse": REDACT_ELLIPSE}


class RedactSpec:
    """What a redaction looks like.
        mode        "pixelate": every covered pixel takes the mean of its cell; "fill": the fill colour
        cell        pixelation cell in luma pixels: 4, 8, 16 or 32.  Cells are aligned to the surface's origin, not to the box
        shape       "rect": the whole padded box; "ellipse": the ellipse inscribed in it
        pad         growth around the box, per side, as a fraction of the box's side: 0..1 (stored as pad_q8 = round(256 pad))
        classes     iterable of the class ids that are redacted (ids in 0..127); None = all
        min_score   entries below it are left visible
        fill        (B, G, R) in 0..255 of mode "fill"; its (Y, U, V) for NV12 / P010 targets come from overlay.palette_rows
    ValueError for anything else, before anything reaches the device.  Specs compare and hash BY VALUE (`key`)."""

    def __init__(self, mode="pixelate", cell=16, shape="rect", pad=0.1, classes=None, min_score=0.0, fill=(0, 0, 0)):
        def integer(v):
            try:
                return None if isinstance(v, bool) else operator.index(v)
            except TypeError:
                return None
        if not isinstance(mode, str) or mode not in _MODES:
            raise ValueError('RedactSpec: mode must be "pixelate" or "fill", got %r' % (mode,))
        if integer(cell) not in REDACT_CELLS:
            raise ValueError("RedactSpec: cell must be 4, 8, 16 or 32, got %r" % (cell,))
        if not isinstance(shape, str) or shape not in _SHAPES:
            raise ValueError('RedactSpec: shape must be "rect" or "ellipse", got %r' % (shape,))
        try:
            pad_f = float(pad)
        except (TypeError, ValueError):
            pad_f = math.nan
        if isinstance(pad, bool) or not 0.0 <= pad_f <= 1.0:
            raise ValueError("RedactSpec: pad must be a number in 0..1, got %r" % (pad,))
        if classes is not None:
            try:
                ids = [integer(c) for c in classes]
            except TypeError:
                ids = [None]
            if any(c is None or not 0 <= c < DET_MAX_CLASSES for c in ids):
                raise ValueError("RedactSpec: classes is an iterable of class ids in 0..%d or None, got %r" % (DET_MAX_CLASSES - 1, classes))
            classes = tuple(sorted(set(ids)))
        try:
            min_score = float(min_score)
        except (TypeError, ValueError):
            raise ValueError("RedactSpec: min_score must be a number, got %r" % (min_score,)) from None
        if not math.isfinite(min_score):
            raise ValueError("RedactSpec: min_score must be finite, got %r" % (min_score,))
        try:
            fill3 = tuple(integer(v) for v in fill)
        except TypeError:
            fill3 = ()
        if len(fill3) != 3 or any(v is None or not 0 <= v <= 255 for v in fill3):
            raise ValueError("RedactSpec: fill is a (B, G, R) triple in 0..255, got %r" % (fill,))
        self.mode, self.cell, self.shape, self.pad, self.classes = mode, integer(cell), shape, pad_f, classes
        self.min_score, self.fill = min_score, fill3
        self.mode_code, self.shape_code = _MODES[mode], _SHAPES[shape]
        self.pad_q8 = int(round(pad_f * 256))
        mask = [0, 0, 0, 0]
        for c in range(DET_MAX_CLASSES) if classes is None else classes:
            mask[c >> 5] |= 1 << (c & 31)
        self.class_mask = tuple(mask)
        p = palette_rows([fill3])[0]                                 # B, G, R, text, Y, U, V, text luma
        self.fill_bytes = (int(p[0]), int(p[1]), int(p[2]), 0, int(p[4]), int(p[5]), int(p[6]), 0)
        self.key = (self.mode_code, self.cell, self.shape_code, self.pad_q8, self.class_mask, min_score, fill3)

    def __eq__(self, other):
        return isinstance(other, RedactSpec) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return "RedactSpec(mode=%r, cell=%d, shape=%r, pad=%r, classes=%r, min_score=%r, fill=%r)" % (
            self.mode, self.cell, self.shape, self.pad, self.classes, self.min_score, self.fill)


# sy_redact_row (include/streamyolo_hip.h), one per batch row
_REDACT_DTYPE = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("Hs", "<i4"), ("Ws", "<i4"), ("row_stride", "<i4"),
                          ("chroma_stride", "<i4"), ("format", "<i4"), ("divisor", "<f4"), ("min_score", "<f4"), ("pad_q8", "<i4"),
                          ("mode", "<i4"), ("cell", "<i4"), ("shape", "<i4"), ("reserved", "<i4"), ("fill", "u1", (8,)),
                          ("class_mask", "<u4", (4,))])
assert _REDACT_DTYPE.itemsize == 88


class RedactRows(OverlayRows):
    """The table of sy_redact_row descriptors of `batch` rows (overlay.OverlayRows with another record): one device buffer with a
    ring of pinned host mirrors, upload() is a single non-blocking copy on the current stream; it holds the plane tensors its rows
    point into.  A row nobody set redacts nothing."""
    _DTYPE = _REDACT_DTYPE

    def set_row(self, b, surface, divisor, spec):
        yuv = len(surface.planes) == 2
        self._rows[b] = (surface.planes[0].data_ptr(), surface.planes[1].data_ptr() if yuv else 0, surface.hw[0], surface.hw[1],
                         surface.pitch, surface.chroma_pitch, surface.format, divisor, spec.min_score, spec.pad_q8, spec.mode_code,
                         spec.cell, spec.shape_code, 0, spec.fill_bytes, spec.class_mask)
        self._held[b] = surface.planes


def redact_rows(rows, max_hw, boxes, layout, cnt):
    """The one launch: the uploaded table `rows` (RedactRows) over the list tensors."""
    ops.redact(rows.table, rows.batch, max_hw, boxes, layout, cnt)


def check_spec(spec, who):
    if not isinstance(spec, RedactSpec):
        raise ValueError("%s: spec must be a RedactSpec, got %r" % (who, spec))
    return spec


_default_spec = None                                                 # redact_detections(spec=None)
_single = {}                                                         # device -> the one-row table of redact_detections


def redact_detections(target, boxes, scores, labels, spec=None):
    """Redact boxes in `target` (a Surface, or a uint8 device tensor [H, W, 3] taken as BGR), in place, and return it.  boxes
    [n, 4] (x1, y1, x2, y2 in the target's own pixel coordinates), scores [n], labels [n]: host arrays or tensors; device tensors
    are used where they lie (no host read).  EVERY entry is looked at, in any order: coverage is a union.  The same kernel, rule
    and spec as MultiStreamDetector.redact.  IN PLACE: redact a `clone()` while a decoder may still hold the surface as a
    reference frame; redact before draw_detections, so that the drawing stays legible on top."""
    global _default_spec
    if spec is None:
        spec = _default_spec = _default_spec or RedactSpec()
    check_spec(spec, "redact_detections")
    surf = as_target(target, who="redact_detections")
    dev = surf.device
    b = torch.as_tensor(boxes).to(device=dev, dtype=torch.float32).reshape(-1, 4)
    n = int(b.shape[0])
    s = torch.as_tensor(scores).to(device=dev, dtype=torch.float32).reshape(-1)
    l = torch.as_tensor(labels).to(device=dev, dtype=torch.float32).reshape(-1)
    if s.numel() != n or l.numel() != n:
        raise ValueError("redact_detections: %d boxes with %d scores, %d labels" % (n, s.numel(), l.numel()))
    if n == 0:
        return target
    lists = torch.cat([b, s[:, None], l[:, None]], dim=1).reshape(1, n, 6).contiguous()
    cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
    rows = _single.get(dev)
    if rows is None:
        rows = _single[dev] = RedactRows(1, dev)
    rows.set_row(0, surf, 1.0, spec)
    rows.upload()
    redact_rows(rows, surf.hw, lists, 1, cnt)
    return target

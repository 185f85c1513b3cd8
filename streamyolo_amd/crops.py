"""Crop detected objects out of camera surfaces on the device (csrc/crop.hip, sy_crop_gather): the hand-off to a second stage —
traffic-light state, sign and plate readers, attribute classifiers, re-ID embeddings — which needs the objects as images at the
camera's own resolution, not the decimated network input, and without reading the boxes back to the host.

  CropSpec                          what a crop batch looks like: size, context padding, aspect, dtype, channel order, mean / std,
                                    filters and caps; validated on the host
  Crops                             the result: images [capacity, 3, Ch, Cw], index, rect, count — device tensors, no host read
  MultiStreamDetector.crops()       the latest tick's results of some streams out of the surfaces given, ONE C call on the current
  StreamingDetector.crops()         stream behind the tick, not on the tick's tape (streaming.py)
  crop_detections()                 the stand-alone form for any boxes in the source's own pixel coordinates

The rule (rectangle, padding, aspect, sampling, taps, output, slots) is stated once, in include/streamyolo_hip.h.  It is a
bilinear resampling with half-pixel centres: a box much larger than the crop is decimated without a low-pass filter.
"""
import math
import operator

import numpy as np
import torch

from . import ops
from ._lib import CROP_KEEP_ASPECT, CROP_MAX_BOXES, CROP_RGB_OUT, DET_MAX_CLASSES
from .data import Surface
from .overlay import OverlayRows

_DTYPES = (torch.uint8, torch.float32, torch.float16, torch.bfloat16)
DEFAULT_PER_STREAM = 32                                              # capacity=None without max_per_stream: slots per batch row


class CropSpec:
    """What a crop batch looks like.
        size            (Ch, Cw) of every crop: 8..512 each, Cw a multiple of 8
        pad             context around the box, per side, as a fraction of the box's side: 0..1 (stored as pad_q8 = round(256 pad))
        keep_aspect     True: the shorter side of the padded box grows until the rectangle has the crop's aspect; False: each axis
                        is stretched on its own
        dtype           torch.uint8 (the interpolated bytes), float32, float16 or bfloat16
        channel_order   "bgr" or "rgb": the order of the three output planes
        mean, std       per OUTPUT plane (in channel_order): a float crop is (v - mean) * (1 / std), the reciprocal taken in
                        float32; None = 0 / 1.  Not with uint8
        min_score       entries below it are skipped
        max_per_stream  at most this many crops per stream, the first ones in list order (descending score); 0 = no cap
        classes         iterable of the class ids that are cropped (ids in 0..127); None = all
        fill            (B, G, R) of what lies outside the surface
        capacity        slots of the batch; None = batch rows x (max_per_stream or 32).  Kept entries beyond it are counted in
                        count[1] and not written
    ValueError for anything else, before anything reaches the device.  Specs compare and hash BY VALUE (`key`): a spec built
    again with the same arguments — inline, once per tick — is the same spec to a detector's output cache."""

    def __init__(self, size=(64, 64), pad=0.0, keep_aspect=True, dtype=torch.float16, channel_order="bgr", mean=None, std=None,
                 min_score=0.0, max_per_stream=0, classes=None, fill=(114, 114, 114), capacity=None):
        def integer(v):
            try:
                return None if isinstance(v, bool) else operator.index(v)
            except TypeError:
                return None

        def triple(name, v):
            try:
                t = tuple(float(x) for x in v)
            except (TypeError, ValueError):
                t = ()
            if len(t) != 3 or not all(math.isfinite(x) for x in t):
                raise ValueError("CropSpec: %s is three finite numbers, one per output plane, or None, got %r" % (name, v))
            return t
        try:
            ch, cw = (integer(v) for v in size)
        except (TypeError, ValueError):
            ch = cw = None
        if ch is None or cw is None or not 8 <= ch <= 512 or not 8 <= cw <= 512 or cw % 8:
            raise ValueError("CropSpec: size is (height, width) in 8..512 with the width a multiple of 8, got %r" % (size,))
        try:
            pad_f = float(pad)
        except (TypeError, ValueError):
            pad_f = math.nan
        if isinstance(pad, bool) or not 0.0 <= pad_f <= 1.0:
            raise ValueError("CropSpec: pad must be a number in 0..1, got %r" % (pad,))
        if dtype not in _DTYPES:
            raise ValueError("CropSpec: dtype must be torch.uint8, float32, float16 or bfloat16, got %r" % (dtype,))
        if channel_order not in ("bgr", "rgb"):
            raise ValueError('CropSpec: channel_order must be "bgr" or "rgb", got %r' % (channel_order,))
        if dtype == torch.uint8 and (mean is not None or std is not None):
            raise ValueError("CropSpec: mean / std need a float dtype, got torch.uint8")
        mean3 = None if mean is None else triple("mean", mean)
        std3 = None if std is None else triple("std", std)
        if std3 is not None and any(s == 0.0 for s in std3):
            raise ValueError("CropSpec: std must not be 0, got %r" % (std,))
        try:
            min_score = float(min_score)
        except (TypeError, ValueError):
            raise ValueError("CropSpec: min_score must be a number, got %r" % (min_score,)) from None
        if not math.isfinite(min_score):
            raise ValueError("CropSpec: min_score must be finite, got %r" % (min_score,))
        cap_row = integer(max_per_stream)
        if cap_row is None or not 0 <= cap_row <= CROP_MAX_BOXES:
            raise ValueError("CropSpec: max_per_stream must be an integer in 0..%d (0: no cap), got %r" % (CROP_MAX_BOXES, max_per_stream))
        if classes is not None:
            try:
                ids = [integer(c) for c in classes]
            except TypeError:
                ids = [None]
            if any(c is None or not 0 <= c < DET_MAX_CLASSES for c in ids):
                raise ValueError("CropSpec: classes is an iterable of class ids in 0..%d or None, got %r" % (DET_MAX_CLASSES - 1, classes))
            classes = tuple(sorted(set(ids)))
        try:
            fill3 = tuple(integer(v) for v in fill)
        except TypeError:
            fill3 = ()
        if len(fill3) != 3 or any(v is None or not 0 <= v <= 255 for v in fill3):
            raise ValueError("CropSpec: fill is a (B, G, R) triple in 0..255, got %r" % (fill,))
        if capacity is not None:
            cap = integer(capacity)
            if cap is None or not 1 <= cap < 2 ** 31:
                raise ValueError("CropSpec: capacity must be an integer >= 1 or None, got %r" % (capacity,))
            capacity = cap
        self.size, self.pad, self.keep_aspect, self.dtype, self.channel_order = (ch, cw), pad_f, bool(keep_aspect), dtype, channel_order
        self.min_score, self.max_per_stream, self.classes, self.fill, self.capacity = min_score, cap_row, classes, fill3, capacity
        self.pad_q8 = int(round(pad_f * 256))
        self.flags = (CROP_KEEP_ASPECT if self.keep_aspect else 0) | (CROP_RGB_OUT if channel_order == "rgb" else 0)
        mask = [0, 0, 0, 0]
        for c in range(DET_MAX_CLASSES) if classes is None else classes:
            mask[c >> 5] |= 1 << (c & 31)
        self.class_mask = tuple(mask)
        # host tables, in output plane order: what the kernel subtracts and multiplies by (None: 0 / 1, no table)
        self.mean = None if mean3 is None and std3 is None else np.asarray(mean3 or (0.0, 0.0, 0.0), dtype=np.float32)
        self.scale = None if self.mean is None else \
            (np.float32(1.0) / np.asarray(std3 or (1.0, 1.0, 1.0), dtype=np.float32)).astype(np.float32)
        self._dev = {}                                               # device -> (mean, scale)
        # everything the kernel and the output tensors depend on: the spec's value
        self.key = (self.size, self.pad_q8, self.flags, dtype, mean3, std3, min_score, cap_row, self.class_mask, fill3, capacity)

    def __eq__(self, other):
        return isinstance(other, CropSpec) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def tables(self, device):
        """(mean [3], scale [3]) fp32 tensors on `device`, built once; (None, None) without mean / std."""
        if self.mean is None:
            return None, None
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(torch.from_numpy(a).to(device) for a in (self.mean, self.scale))
        return t

    def slots(self, batch):
        """The capacity of a crop batch over `batch` rows."""
        return self.capacity if self.capacity is not None else int(batch) * (self.max_per_stream or DEFAULT_PER_STREAM)


class Crops:
    """A crop batch, all DEVICE tensors (nothing is read to produce them):
        images [capacity, 3, Ch, Cw]   the spec's dtype, planes in its channel_order
        index  [capacity, 4] int32     batch row, list index, track id (-1 without tracking), class of every slot
        rect   [capacity, 4] int32     X1, Y1, X2, Y2 (inclusive) of the sampled rectangle in the source's pixels, after padding and
                                       aspect; it may leave the surface (the fill colour is sampled there)
        count  [2] int32               slots written (= min(kept, capacity)), entries kept in total
    Only the first count[0] slots mean anything; the others are never written.  index[:, 0] is the BATCH ROW of the tick:
    `row_sids[b]` is the stream id that row b served (None: the row was not asked for), a host tuple known without a device
    read.  The tensors are owned by whoever made them (a detector reuses them for its next crops() with the same spec)."""

    def __init__(self, images, index, rect, count, row_sids=(None,)):
        self.images, self.index, self.rect, self.count, self.row_sids = images, index, rect, count, tuple(row_sids)
        self.spec = None                                             # the CropSpec a detector allocated it for

    @classmethod
    def empty(cls, spec, capacity, device):
        dev, i32 = torch.device(device), torch.int32
        return cls(torch.zeros((capacity, 3) + spec.size, dtype=spec.dtype, device=dev), torch.zeros((capacity, 4), dtype=i32, device=dev),
                   torch.zeros((capacity, 4), dtype=i32, device=dev), torch.zeros(2, dtype=i32, device=dev))


class CropCache:
    """A detector's output tensors per spec VALUE, the few most recently used ones (a deployment crops with one or two specs; a
    spec that varies from tick to tick must not pile up batches of device memory).  An evicted batch lives on for whoever holds it."""
    SIZE = 4

    def __init__(self):
        self._held = {}                                              # spec -> Crops, least recently used first

    def get(self, spec, batch, device):
        """The Crops of `spec` (allocated, zeroed, on first use) — the same tensors for every spec equal to it."""
        out = self._held.pop(spec, None)
        if out is None:
            out = Crops.empty(spec, spec.slots(batch), device)
            out.spec = spec                                          # (whose device tables every equal spec then uses)
            while len(self._held) >= self.SIZE:
                del self._held[next(iter(self._held))]
        self._held[spec] = out
        return out

    def peek(self, spec):
        return self._held.get(spec)

    def __len__(self):
        return len(self._held)


# sy_crop_row (include/streamyolo_hip.h), one per batch row
_CROP_DTYPE = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("Hs", "<i4"), ("Ws", "<i4"), ("row_stride", "<i4"),
                        ("chroma_stride", "<i4"), ("format", "<i4"), ("divisor", "<f4"), ("min_score", "<f4"), ("max_crops", "<i4"),
                        ("pad_q8", "<i4"), ("fill", "u1", (4,)), ("class_mask", "<u4", (4,))])
assert _CROP_DTYPE.itemsize == 72


def as_source(source, device=None, hw=None, who="crops"):
    """A crop source as a Surface: a Surface as it is, a uint8 device tensor [H, W, 3] taken as BGR.  ValueError for anything else,
    for a source on another device than `device`, for a size other than `hw`."""
    if not isinstance(source, Surface):
        if not isinstance(source, torch.Tensor):
            raise ValueError("%s: a source is a Surface or a uint8 tensor [H, W, 3] (BGR), got %r" % (who, type(source).__name__))
        source = Surface(source, "bgr")
    if device is not None and source.device != torch.device(device):
        raise ValueError("%s: a source on %s cannot be cropped from %s" % (who, source.device, device))
    if hw is not None and tuple(source.hw) != tuple(hw):
        raise ValueError("%s: a %dx%d source for a %dx%d frame" % ((who,) + tuple(source.hw) + tuple(hw)))
    return source


class CropRows(OverlayRows):
    """The table of sy_crop_row descriptors of `batch` rows (overlay.OverlayRows with another record): one device buffer with a ring
    of pinned host mirrors, upload() is a single non-blocking copy on the current stream.  A row nobody set keeps nothing."""
    _DTYPE = _CROP_DTYPE

    def set_row(self, b, surface, divisor, spec):
        yuv = len(surface.planes) == 2
        self._rows[b] = (surface.planes[0].data_ptr(), surface.planes[1].data_ptr() if yuv else 0, surface.hw[0], surface.hw[1],
                         surface.pitch, surface.chroma_pitch, surface.format, divisor, spec.min_score, spec.max_per_stream,
                         spec.pad_q8, spec.fill + (0,), spec.class_mask)
        self._held[b] = surface.planes


def gather_rows(rows, boxes, layout, ids, cnt, spec, crops):
    """The one C call: the uploaded table `rows` (CropRows) over the list tensors into `crops`."""
    mean, scale = spec.tables(rows.table.device)
    ops.crop_gather(rows.table, rows.batch, boxes, layout, ids, cnt, crops.images, crops.index, crops.rect, crops.count,
                    flags=spec.flags, mean=mean, scale=scale)
    return crops


def check_spec(spec, who):
    if not isinstance(spec, CropSpec):
        raise ValueError("%s: spec must be a CropSpec, got %r" % (who, spec))
    return spec


_default_spec = None                                                 # crop_detections(spec=None)
_single = {}                                                         # device -> the one-row table of crop_detections (any spec: every
                                                                     # call writes the whole row)


def crop_detections(source, boxes, scores, labels, ids=None, spec=None):
    """Crop boxes out of `source` (a Surface, or a uint8 device tensor [H, W, 3] taken as BGR) -> Crops.  boxes [n, 4] (x1, y1, x2,
    y2 in the source's own pixel coordinates), scores [n], labels [n], ids [n] or None: host arrays or tensors; device tensors are
    used where they lie (no host read).  At most 256 entries are looked at; capacity=None makes room for all of them.  The same
    kernel, rule and spec as MultiStreamDetector.crops; the result's tensors are fresh."""
    global _default_spec
    if spec is None:
        spec = _default_spec = _default_spec or CropSpec()
    check_spec(spec, "crop_detections")
    surf = as_source(source, who="crop_detections")
    dev = surf.device
    b = torch.as_tensor(boxes).to(device=dev, dtype=torch.float32).reshape(-1, 4)
    n = int(b.shape[0])
    s = torch.as_tensor(scores).to(device=dev, dtype=torch.float32).reshape(-1)
    l = torch.as_tensor(labels).to(device=dev, dtype=torch.float32).reshape(-1)
    i = None if ids is None else torch.as_tensor(ids).to(device=dev, dtype=torch.int32).reshape(1, -1)
    if s.numel() != n or l.numel() != n or (i is not None and i.numel() != n):
        raise ValueError("crop_detections: %d boxes with %d scores, %d labels%s"
                         % (n, s.numel(), l.numel(), "" if i is None else ", %d ids" % i.numel()))
    m = max(n, 1)                                                    # (an empty list is one unused entry: the call still counts 0)
    lists = torch.zeros((1, m, 6), dtype=torch.float32, device=dev)
    lists[0, :n] = torch.cat([b, s[:, None], l[:, None]], dim=1)
    if i is not None:
        i = i.contiguous() if n else torch.zeros((1, 1), dtype=torch.int32, device=dev)
    cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
    rows = _single.get(dev)
    if rows is None:
        rows = _single[dev] = CropRows(1, dev)
    rows.set_row(0, surf, 1.0, spec)
    rows.upload()
    cap = spec.capacity if spec.capacity is not None else min(m, spec.max_per_stream or CROP_MAX_BOXES, CROP_MAX_BOXES)
    return gather_rows(rows, lists, 1, i, cnt, spec, Crops.empty(spec, cap, dev))

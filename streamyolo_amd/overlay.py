"""Draw detections and track ids into camera surfaces on the device (csrc/overlay.hip, sy_overlay_draw): the last step of a
camera pipeline — what a monitor wall, a recorder or an encoder is fed — without pulling the boxes to the host, drawing into a
host copy of the frame and uploading it again.

  OverlayStyle                      what a drawing looks like: class names, colours, outline width, label size; validated on the
                                    host, its palette / class text / font tables built once per device
  MultiStreamDetector.draw()        the latest tick's results of some streams into the targets given, ONE launch on the current
  StreamingDetector.draw()          stream behind the tick, no host read, not on the tick's tape (streaming.py)
  draw_detections()                 the stand-alone form for any boxes in the target's own pixel coordinates

The rendering rule (rectangle, outline, label tab, precedence, clipping, chroma, untouched bytes) is stated once, in
include/streamyolo_hip.h.  Everything is opaque and the lowest list index wins a pixel, so the best box ends on top.

WARNING — drawing is IN PLACE.  A hardware decoder keeps the surfaces it still needs as reference frames for the pictures that
follow; drawing on one corrupts every frame predicted from it.  Never draw on a decoder surface that the decoder may still
hold: draw on a copy,

    det.draw([s.clone() for s in surfaces], sids)

(`Surface.clone()`: same format, sizes and pitches, its own memory), or on surfaces the decoder has released.

The 8 x 8 font below was drawn for this project (upper case, digits and `# % . - _ :`; 5 x 7 shapes in an 8 x 8 cell).  Names
are upper-cased, cut to 8 glyphs, and characters outside ASCII 32..95 become spaces.
"""
import numpy as np
import torch

from . import ops
from ._lib import OVERLAY_ID, OVERLAY_MAX_BOXES, OVERLAY_SCORE
from .data import Surface

# the eight Argoverse-HD classes, in label order
DEFAULT_CLASS_NAMES = ["person", "bicycle", "car", "motorcycle", "bus", "truck", "traffic_light", "stop_sign"]
# eight distinct colours, (B, G, R)
DEFAULT_PALETTE = [(60, 60, 230), (40, 160, 250), (80, 200, 60), (220, 120, 30), (200, 60, 180), (230, 220, 40), (30, 230, 230),
                   (140, 40, 90)]

# 5 x 7 shapes, one string per glyph row (top to bottom), 'X' = set; placed in columns 1..5, rows 0..6 of the 8 x 8 cell
_SHAPES = {
    "A": ".XXX. X...X X...X XXXXX X...X X...X X...X", "B": "XXXX. X...X X...X XXXX. X...X X...X XXXX.",
    "C": ".XXX. X...X X.... X.... X.... X...X .XXX.", "D": "XXXX. X...X X...X X...X X...X X...X XXXX.",
    "E": "XXXXX X.... X.... XXXX. X.... X.... XXXXX", "F": "XXXXX X.... X.... XXXX. X.... X.... X....",
    "G": ".XXX. X...X X.... X.XXX X...X X...X .XXXX", "H": "X...X X...X X...X XXXXX X...X X...X X...X",
    "I": ".XXX. ..X.. ..X.. ..X.. ..X.. ..X.. .XXX.", "J": "..XXX ...X. ...X. ...X. ...X. X..X. .XX..",
    "K": "X...X X..X. X.X.. XX... X.X.. X..X. X...X", "L": "X.... X.... X.... X.... X.... X.... XXXXX",
    "M": "X...X XX.XX X.X.X X.X.X X...X X...X X...X", "N": "X...X XX..X X.X.X X..XX X...X X...X X...X",
    "O": ".XXX. X...X X...X X...X X...X X...X .XXX.", "P": "XXXX. X...X X...X XXXX. X.... X.... X....",
    "Q": ".XXX. X...X X...X X...X X.X.X X..X. .XX.X", "R": "XXXX. X...X X...X XXXX. X.X.. X..X. X...X",
    "S": ".XXXX X.... X.... .XXX. ....X ....X XXXX.", "T": "XXXXX ..X.. ..X.. ..X.. ..X.. ..X.. ..X..",
    "U": "X...X X...X X...X X...X X...X X...X .XXX.", "V": "X...X X...X X...X X...X X...X .X.X. ..X..",
    "W": "X...X X...X X...X X.X.X X.X.X XX.XX X...X", "X": "X...X X...X .X.X. ..X.. .X.X. X...X X...X",
    "Y": "X...X X...X .X.X. ..X.. ..X.. ..X.. ..X..", "Z": "XXXXX ....X ...X. ..X.. .X... X.... XXXXX",
    "0": ".XXX. X...X X..XX X.X.X XX..X X...X .XXX.", "1": "..X.. .XX.. ..X.. ..X.. ..X.. ..X.. .XXX.",
    "2": ".XXX. X...X ....X ...X. ..X.. .X... XXXXX", "3": "XXXXX ...X. ..X.. ...X. ....X X...X .XXX.",
    "4": "...X. ..XX. .X.X. X..X. XXXXX ...X. ...X.", "5": "XXXXX X.... XXXX. ....X ....X X...X .XXX.",
    "6": "..XX. .X... X.... XXXX. X...X X...X .XXX.", "7": "XXXXX ....X ...X. ..X.. .X... .X... .X...",
    "8": ".XXX. X...X X...X .XXX. X...X X...X .XXX.", "9": ".XXX. X...X X...X .XXXX ....X ...X. .XX..",
    "#": ".X.X. .X.X. XXXXX .X.X. XXXXX .X.X. .X.X.", "%": "XX... XX..X ...X. ..X.. .X... X..XX ...XX",
    ".": "..... ..... ..... ..... ..... .XX.. .XX..", "-": "..... ..... ..... XXXXX ..... ..... .....",
    "_": "..... ..... ..... ..... ..... ..... XXXXX", ":": "..... .XX.. .XX.. ..... .XX.. .XX.. .....",
}


def font_glyphs():
    """The font as sy_overlay_draw reads it: uint8 [64, 8], glyph code c = ASCII 32 + c, one byte per glyph row, the MSB is the left
    pixel.  Codes without a shape (most punctuation) are blank."""
    g = np.zeros((64, 8), dtype=np.uint8)
    for ch, shape in _SHAPES.items():
        for r, row in enumerate(shape.split()):
            g[ord(ch) - 32, r] = sum(1 << (6 - c) for c in range(5) if row[c] == "X")
    return g


def encode_name(name):
    """A class name as glyph codes: upper-cased, cut to 8 glyphs, characters outside ASCII 32..95 become spaces."""
    codes = []
    for ch in str(name).upper()[:8]:
        o = ord(ch)
        codes.append(o - 32 if 32 <= o <= 95 else 0)
    return codes


def palette_rows(colours):
    """(B, G, R) colours [K, 3] -> the kernel's palette uint8 [K, 8]: B, G, R, text value (0 or 255), Y, U, V, text luma (16 or 235).
    BT.601 limited range in its integer form, Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 with the matching U and V rows; the
    text is white on a colour with Y < 128 and black otherwise."""
    c = np.asarray(colours, dtype=np.int64).reshape(-1, 3)
    b, g, r = c[:, 0], c[:, 1], c[:, 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    white = y < 128
    out = np.stack([b, g, r, np.where(white, 255, 0), y, u, v, np.where(white, 235, 16)], axis=1)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


class OverlayStyle:
    """What a drawing looks like.  class_names: one per class id (default: the eight Argoverse-HD classes), at most 128; palette:
    one (B, G, R) per class (default: eight distinct colours, repeated for longer name lists); thickness: outline width in
    pixels, 1..16; text_scale: 0 = no label tab, 1..4 = glyph cells of 8 x scale pixels; show: what follows the class name on the
    tab — "id" (the track id; plain detections have none and show the name alone), "score" (in percent) or None; min_score: boxes
    below it are not drawn; max_boxes: at most this many list entries per frame are looked at, 1..256.  ValueError for anything
    else, before anything reaches the device."""

    def __init__(self, class_names=None, palette=None, thickness=2, text_scale=2, show="id", min_score=0.3, max_boxes=128):
        names = list(DEFAULT_CLASS_NAMES if class_names is None else class_names)
        if not 1 <= len(names) <= 128 or not all(isinstance(n, str) for n in names):
            raise ValueError("OverlayStyle: class_names is a list of 1..128 strings, got %r" % (class_names,))
        if palette is None:
            colours = [DEFAULT_PALETTE[k % len(DEFAULT_PALETTE)] for k in range(len(names))]
        else:
            try:
                colours = [tuple(int(v) for v in c) for c in palette]
            except (TypeError, ValueError):
                raise ValueError("OverlayStyle: palette is a list of (B, G, R) triples, got %r" % (palette,)) from None
            if len(colours) != len(names) or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in colours):
                raise ValueError("OverlayStyle: palette needs one (B, G, R) in 0..255 per class name (%d), got %r" % (len(names), palette))
        if isinstance(thickness, bool) or not isinstance(thickness, (int, np.integer)) or not 1 <= thickness <= 16:
            raise ValueError("OverlayStyle: thickness must be an integer in 1..16, got %r" % (thickness,))
        if isinstance(text_scale, bool) or not isinstance(text_scale, (int, np.integer)) or not 0 <= text_scale <= 4:
            raise ValueError("OverlayStyle: text_scale must be an integer in 0..4, got %r" % (text_scale,))
        if show not in ("id", "score", None):
            raise ValueError('OverlayStyle: show must be "id", "score" or None, got %r' % (show,))
        try:
            min_score = float(min_score)
        except (TypeError, ValueError):
            raise ValueError("OverlayStyle: min_score must be a number, got %r" % (min_score,)) from None
        if not np.isfinite(min_score):
            raise ValueError("OverlayStyle: min_score must be finite, got %r" % (min_score,))
        if isinstance(max_boxes, bool) or not isinstance(max_boxes, (int, np.integer)) or not 1 <= max_boxes <= OVERLAY_MAX_BOXES:
            raise ValueError("OverlayStyle: max_boxes must be an integer in 1..%d, got %r" % (OVERLAY_MAX_BOXES, max_boxes))
        self.class_names, self.colours = names, colours
        self.thickness, self.text_scale, self.show = int(thickness), int(text_scale), show
        self.min_score, self.max_boxes = min_score, int(max_boxes)
        self.flags = OVERLAY_ID if show == "id" else OVERLAY_SCORE if show == "score" else 0
        self.palette = palette_rows(colours)                         # host tables: uint8 [K, 8]
        self.class_text = np.full((len(names), 8), 0xFF, dtype=np.uint8)
        for k, n in enumerate(names):
            codes = encode_name(n)
            self.class_text[k, :len(codes)] = codes
        self._dev = {}                                               # device -> (palette, class_text, glyphs)
        self._single = {}                                            # device -> the one-row table of draw_detections

    def tables(self, device):
        """(palette [K, 8], class_text [K, 8], glyphs [64, 8]) uint8 tensors on `device`, built once."""
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            t = tuple(torch.from_numpy(a).to(device) for a in (self.palette, self.class_text, font_glyphs()))
            self._dev[device] = t
        return t


# sy_overlay_row (include/streamyolo_hip.h), one per batch row
_OVERLAY_DTYPE = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("Hs", "<i4"), ("Ws", "<i4"), ("row_stride", "<i4"),
                           ("chroma_stride", "<i4"), ("format", "<i4"), ("divisor", "<f4"), ("min_score", "<f4"),
                           ("max_boxes", "<i4"), ("thickness", "<i4"), ("text_scale", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
assert _OVERLAY_DTYPE.itemsize == 64


def as_target(target, device=None, hw=None, who="draw"):
    """A drawing target as a Surface: a Surface as it is, a uint8 device tensor [H, W, 3] taken as BGR.  ValueError for anything
    else, for a target on another device than `device`, for a size other than `hw`."""
    if not isinstance(target, Surface):
        if not isinstance(target, torch.Tensor):
            raise ValueError("%s: a target is a Surface or a uint8 tensor [H, W, 3] (BGR), got %r" % (who, type(target).__name__))
        target = Surface(target, "bgr")
    if device is not None and target.device != torch.device(device):
        raise ValueError("%s: a target on %s cannot be drawn on from %s" % (who, target.device, device))
    if hw is not None and tuple(target.hw) != tuple(hw):
        raise ValueError("%s: a %dx%d target for a %dx%d frame" % ((who,) + tuple(target.hw) + tuple(hw)))
    return target


class OverlayRows:
    """The table of sy_overlay_row descriptors of `batch` rows: one device buffer with a ring of pinned host mirrors, upload() is a
    single non-blocking copy on the current stream (as data.FrameRowsU8).  A row nobody set draws nothing."""
    _DTYPE = _OVERLAY_DTYPE                                          # the record (crops.CropRows: sy_crop_row)

    def __init__(self, batch, device):
        self.batch, dev = int(batch), torch.device(device)
        nbytes = self._DTYPE.itemsize * self.batch
        self.table = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._rows = np.zeros(self.batch, dtype=self._DTYPE)
        self._ring = [torch.zeros(nbytes, dtype=torch.uint8) for _ in range(4 if dev.type == "cuda" else 1)]
        if dev.type == "cuda":
            self._ring = [h.pin_memory() for h in self._ring]
        self._done = [None] * len(self._ring)
        self._at = 0
        self._held = [None] * self.batch                             # row -> the plane tensors its descriptor points into

    def clear(self):
        self._rows[:] = 0
        self._held = [None] * self.batch

    def set_row(self, b, surface, divisor, style):
        yuv = len(surface.planes) == 2
        self._rows[b] = (surface.planes[0].data_ptr(), surface.planes[1].data_ptr() if yuv else 0, surface.hw[0], surface.hw[1],
                         surface.pitch, surface.chroma_pitch, surface.format, divisor, style.min_score, style.max_boxes,
                         style.thickness, style.text_scale, style.flags, 0)
        self._held[b] = surface.planes

    def upload(self):
        self._at = (self._at + 1) % len(self._ring)
        if self._done[self._at] is not None:
            self._done[self._at].synchronize()                       # (only when the device is a whole ring of draws behind)
        self._ring[self._at].numpy()[:] = self._rows.view(np.uint8)
        self.table.copy_(self._ring[self._at], non_blocking=True)
        if self.table.is_cuda:
            ev = self._done[self._at] or torch.cuda.Event()
            ev.record()
            self._done[self._at] = ev


def draw_rows(rows, max_hw, boxes, layout, ids, cnt, style):
    """The one launch: the uploaded table `rows` (OverlayRows) over the list tensors."""
    palette, text, glyphs = style.tables(rows.table.device)
    ops.overlay_draw(rows.table, rows.batch, max_hw, boxes, layout, ids, cnt, palette, text, glyphs)


def draw_detections(target, boxes, scores, labels, ids=None, style=None):
    """Draw boxes into `target` (a Surface, or a uint8 device tensor [H, W, 3] taken as BGR), in place, and return it.  boxes
    [n, 4] (x1, y1, x2, y2 in the target's own pixel coordinates), scores [n], labels [n], ids [n] or None: host arrays or
    tensors; device tensors are used where they lie (no host read).  The order given is the precedence: entry 0 ends on top, so
    pass the boxes in descending score.  At most style.max_boxes (<= 256) entries are drawn.  The same kernel, rule and style
    as MultiStreamDetector.draw."""
    style = OverlayStyle() if style is None else style
    if not isinstance(style, OverlayStyle):
        raise ValueError("draw_detections: style must be an OverlayStyle, got %r" % (style,))
    surf = as_target(target, who="draw_detections")
    dev = surf.device
    b = torch.as_tensor(boxes).to(device=dev, dtype=torch.float32).reshape(-1, 4)
    n = int(b.shape[0])
    s = torch.as_tensor(scores).to(device=dev, dtype=torch.float32).reshape(-1)
    l = torch.as_tensor(labels).to(device=dev, dtype=torch.float32).reshape(-1)
    i = None if ids is None else torch.as_tensor(ids).to(device=dev, dtype=torch.int32).reshape(1, -1).contiguous()
    if s.numel() != n or l.numel() != n or (i is not None and i.numel() != n):
        raise ValueError("draw_detections: %d boxes with %d scores, %d labels%s"
                         % (n, s.numel(), l.numel(), "" if i is None else ", %d ids" % i.numel()))
    if n == 0:
        return target
    lists = torch.cat([b, s[:, None], l[:, None]], dim=1).reshape(1, n, 6).contiguous()
    cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
    rows = style._single.get(dev)
    if rows is None:
        rows = style._single[dev] = OverlayRows(1, dev)
    rows.set_row(0, surf, 1.0, style)
    rows.upload()
    draw_rows(rows, surf.hw, lists, 1, i, cnt, style)
    return target

"""Device-side input pipeline: the host mirror of what the reference does between
`cv2.imread` and `model(inps, targets)`, with the per-pixel work in ONE HIP launch (csrc/input_pipeline.hip).

Reference path (per sample, CPU workers, then the GPU):
    `_mirror` + `preproc` (exps/data/data_augment_flip.py:140-167)  ->  fp32 CHW on a 114 canvas
    `np.concatenate((img, support_img))` (exps/data/tal_flip_mosaicdetection.py:257)  ->  fp32 [6,H,W]
    `DataPrefetcher` H2D on a side stream (exps/train_utils/double_data_prefetcher.py)  ->  13.8 MB per 600x960 pair
    `Exp.preprocess(inps, targets, tsize)` (cfgs/l_s50_onex_dfp_tal_filp.py:161-172)  ->  bilinear multi-scale resize
Here the uint8 HWC frames are uploaded as they are (3.5 MB per pair) and `FramePairsU8` carries them, with the mirror
flags and the target size, to the plan's stem, where `sy_frames_u8_pack` writes the Focus-packed operand directly.
Box targets are scaled by the same torch arithmetic as the reference (tiny tensors — glue).

There is no CPU implementation here: every entry point needs the HIP library.
"""
import copy

import numpy as np
import torch

from . import ops
from ._lib import PIX_NV12, PIX_P010, pixel_format_code


class FramePairsU8:
    """A batch of (current, support) uint8 HWC frames on the device, standing in for the reference's fp32
    [B, 6, H, W] input tensor (`mode='off_pipe'`) or, with `sup=None`, its [B, 3, H, W] on_pipe frame.

    cur, sup : uint8 [B, Hs, Ws, 3] (BGR, as cv2.imread delivers them), same strides
    pixel_format : "bgr", or "rgb" (the same shape; PIL, torchvision, GStreamer), or "nv12" (hardware video decoders): cur / sup
               are uint8 [B, Hs*3/2, Ws] — Hs luma rows, then Hs/2 rows of interleaved (U, V), Hs and Ws even; stride(1) may
               exceed Ws (a decoder's pitch), the innermost stride is 1.  The pack kernel converts per source pixel (BT.601
               limited range, csrc/input_pipeline.hip): the result is what the BGR path gives for the converted frame
    canvas   : (H, W) letterbox size = exp.input_size / exp.test_size; the frames sit top-left on a 114 canvas
    decimate : 1, or 2 for the exact 2x load-time resize (Argoverse 1200x1920 -> 600x960), or 0 for any other camera
               size: `preproc`'s r = min(H / h, W / w) bilinear letterbox resize (OpenCV fixed-point arithmetic), or -1
               for the streaming detector's per-axis stretch to exactly the canvas (streamyolo_det.py:176-178)
    mirror   : None or uint8 [B]; flag b flips BOTH frames of pair b horizontally (DoubleTrainTransform)
    out_size : (Ho, Wo) the plan runs at (Exp.preprocess's tsize); defaults to the canvas

    Quacks like the tensor it replaces where the model facades look at their input (`shape`, `size()`, `dtype`,
    `device`, `is_cuda`, `float()`, `contiguous()`)."""

    def __init__(self, cur, sup, canvas, decimate=1, mirror=None, out_size=None, pixel_format="bgr"):
        self.pixel_format = pixel_format
        if pixel_format_code(pixel_format) == PIX_NV12:
            assert cur.dtype == torch.uint8 and cur.dim() == 3 and cur.stride(2) == 1
            if cur.shape[1] % 3 or cur.shape[2] % 2:               # (rows = Hs * 3 / 2 with Hs even <=> rows % 3 == 0)
                raise ValueError("FramePairsU8: NV12 images are uint8 [B, Hs*3/2, Ws] with Hs and Ws even, got %s"
                                 % (tuple(cur.shape),))
            assert sup is None or (sup.shape == cur.shape and sup.stride() == cur.stride())
            self.cur, self.sup = cur, sup                        # (a pitch above Ws is part of the format: no repacking)
        else:
            assert cur.dtype == torch.uint8 and cur.dim() == 4 and cur.shape[-1] == 3
            self.cur, self.sup = cur.contiguous(), (None if sup is None else sup.contiguous())
        self.canvas = (int(canvas[0]), int(canvas[1]))
        self.decimate = int(decimate)
        self.mirror = None if mirror is None else mirror.to(device=cur.device, dtype=torch.uint8).contiguous()
        self.out_size = self.canvas if out_size is None else (int(out_size[0]), int(out_size[1]))

    # ---- tensor look-alike -------------------------------------------------------------------------------
    @property
    def shape(self):
        return torch.Size((self.cur.shape[0], 3 if self.sup is None else 6, self.out_size[0], self.out_size[1]))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    dtype = torch.float32

    @property
    def device(self):
        return self.cur.device

    @property
    def is_cuda(self):
        return self.cur.is_cuda

    def float(self):
        return self

    def contiguous(self):
        return self

    def resized(self, tsize):
        """Same frames, run at `tsize` (the bilinear resize happens inside the pack kernel)."""
        return FramePairsU8(self.cur, self.sup, self.canvas, self.decimate, self.mirror, tsize, self.pixel_format)

    def paired_with_self(self):
        """3-channel input on the off_pipe path: the reference duplicates it (dfp_pafpn.py:236-238)."""
        return self if self.sup is not None else FramePairsU8(self.cur, self.cur, self.canvas, self.decimate,
                                                             self.mirror, self.out_size, self.pixel_format)

    # ---- materialisation ---------------------------------------------------------------------------------
    def to_nchw(self):
        """The reference's own input tensor: fp32 [B, 3|6, Ho, Wo] (drop-in for any consumer of `inps`)."""
        out = torch.empty(tuple(self.shape), dtype=torch.float32, device=self.device)
        ops.frames_u8_pack(self.cur, self.sup, self.canvas, self.out_size, out, None, self.decimate, self.mirror,
                           self.pixel_format)
        return out

    def pack_focus(self, cur_view, sup_view=None):
        """Write the stem operand(s) (Focus-packed NHWC16 Views of the plan) straight from the uint8 frames."""
        assert (sup_view is None) == (self.sup is None)
        ops.frames_u8_pack(self.cur, self.sup, self.canvas, self.out_size, cur_view, sup_view, self.decimate, self.mirror,
                           self.pixel_format)


def row_geometry(frame_hw, canvas, decimate=None):
    """The load-time resize of ONE camera of size frame_hw = (hs, ws) onto the `canvas`, as sy_frames_u8_pack resolves it:
    -> (decimate, r).  decimate None picks the mode from the size: 1 when the frame is the canvas, 2 when it is exactly twice
    the canvas, else 0 = `preproc`'s letterbox.  r = min(H / hs, W / ws) is the ratio boxes on the network input are divided by
    to land on the camera frame (the evaluators' `bboxes /= scale`, exps/evaluators/onex_stream_evaluator.py); None for
    decimate -1, whose two axes are stretched separately.  ValueError for a geometry the kernel would refuse."""
    hs, ws = int(frame_hw[0]), int(frame_hw[1])
    H, W = int(canvas[0]), int(canvas[1])
    if hs < 1 or ws < 1:
        raise ValueError("frame size %dx%d" % (hs, ws))
    if decimate is None:
        decimate = 1 if (hs, ws) == (H, W) else 2 if (hs, ws) == (2 * H, 2 * W) else 0
    decimate = int(decimate)
    if decimate == -1:
        return -1, None
    r = min(H / hs, W / ws)
    if decimate == 0:
        if int(hs * r) < 1 or int(ws * r) < 1 or int(hs * r) > H or int(ws * r) > W:
            raise ValueError("a %dx%d frame letterboxed onto %dx%d leaves no pixels (int(h r) x int(w r) = %dx%d)"
                             % (hs, ws, H, W, int(hs * r), int(ws * r)))
        return 0, r
    if decimate not in (1, 2) or hs % decimate or ws % decimate:
        raise ValueError("decimate %r of a %dx%d frame" % (decimate, hs, ws))
    h, w = hs // decimate, ws // decimate
    if h > H or w > W or (h != H and w != W):
        raise ValueError("decimate %d of a %dx%d frame does not letterbox onto %dx%d with ratio 1" % (decimate, hs, ws, H, W))
    return decimate, r


# sy_frame_src (include/streamyolo_hip.h), one per batch row
_ROW_DTYPE = np.dtype([("cur", "<u8"), ("Hs", "<i4"), ("Ws", "<i4"), ("row_stride", "<i4"), ("decimate", "<i4"),
                       ("mirror", "<i4"), ("format", "<i4")])
assert _ROW_DTYPE.itemsize == 32


class FrameRowsU8(FramePairsU8):
    """The per-row counterpart of FramePairsU8 for on_pipe batches (`sup` is always None): every batch row has its OWN camera
    size, decimate mode and mirror flag, kept as a table of sy_frame_src descriptors the pack kernel reads on the device
    (sy_frames_u8_pack_rows) — which camera sits in which row is data, so one recorded launch serves every mix.

    Owns a byte staging arena [batch, Hmax * Wmax * 3] on the device (set_row copies a frame contiguously into its row's
    bytes, row_stride = 3 Ws; an NV12 frame takes half of that, row_stride = Ws — the pixel format is per-row data too) and
    the table with a per-row box divisor behind it: ONE device buffer with pinned host mirrors of the same layout, upload()
    is a single non-blocking copy.  A row without a frame is the plain 114 canvas.

        rows = FrameRowsU8(batch, (Hmax, Wmax), canvas, device)
        rows.set_row(0, frame_a); rows.set_row(1, None); rows.upload()
        model(rows, mode="on_pipe")             # or rows.to_nchw(), rows.pack_focus(view)"""

    _DESC = _ROW_DTYPE                                               # one table row (FrameSurfacesU8: sy_frame_surf)
    _KEY = "rows"

    def __init__(self, batch, max_frame_hw, canvas, device, out_size=None):
        self.batch = int(batch)
        self.max_frame_hw = (int(max_frame_hw[0]), int(max_frame_hw[1]))
        assert self.batch >= 1 and min(self.max_frame_hw) >= 1
        self.canvas = (int(canvas[0]), int(canvas[1]))
        self.out_size = self.canvas if out_size is None else (int(out_size[0]), int(out_size[1]))
        dev = torch.device(device)
        B = self.batch
        self.arena = torch.zeros((B, self.max_frame_hw[0] * self.max_frame_hw[1] * 3), dtype=torch.uint8, device=dev)
        D = self._DESC.itemsize                                      # 32: sy_frame_src
        self._buf = torch.zeros((D + 4) * B, dtype=torch.uint8, device=dev)
        self.table = self._buf[:D * B]                               # B sy_frame_src
        self.divisor = self._buf[D * B:].view(torch.float32)         # [B]: boxes of row b / divisor[b] = camera coordinates
        self._rows = np.zeros(B, dtype=self._DESC)                   # host master copy, edited by set_row
        self._div = np.ones(B, dtype=np.float32)
        # a ring of host mirrors: an upload still in flight keeps reading its mirror while the next tick's rows are written
        self._ring = [torch.zeros((D + 4) * B, dtype=torch.uint8) for _ in range(4 if dev.type == "cuda" else 1)]
        if dev.type == "cuda":
            self._ring = [h.pin_memory() for h in self._ring]
        self._done = [None] * len(self._ring)
        self._at = 0
        # what the plans look at (FramePairsU8's surface): the arena stands for the frames, the table is part of the tape key
        self.cur, self.sup, self.mirror = self.arena, None, None
        self.decimate = (self._KEY, self.table.data_ptr())
        self.pixel_format = self._KEY                                # per row, in the table
        self.upload()

    def set_row(self, b, frame, mirror=False, decimate=None, divisor=None, pixel_format="bgr"):
        """Row b of the next upload() (host table; the pixels go to the arena on the current stream): `frame` uint8 [Hs, Ws, 3]
        (array or tensor, host or device; pixel_format "bgr" or "rgb") or uint8 [Hs*3/2, Ws] ("nv12", Hs and Ws even) or None =
        no frame.  decimate as FramePairsU8 (None: by size, see row_geometry); divisor: what the row's boxes are divided by
        (default: the letterbox ratio r).  ValueError — before anything is written — for a frame this object cannot hold or
        the kernel would refuse."""
        fmt = pixel_format_code(pixel_format)
        if not 0 <= b < self.batch:
            raise ValueError("FrameRowsU8: row %r of %d" % (b, self.batch))
        if frame is None:
            self._rows[b] = self._staged_row(0, 0, 0, 0, 1, 0, 0)
            self._div[b] = 1.0
            return
        f = torch.as_tensor(frame)
        if fmt == PIX_NV12:
            if f.dtype != torch.uint8 or f.dim() != 2 or f.shape[0] % 3 or f.shape[1] % 2:
                raise ValueError("FrameRowsU8: NV12 frames must be uint8 [Hs*3/2, Ws] with Hs and Ws even, got %s %s"
                                 % (f.dtype, tuple(f.shape)))
            hs, ws = int(f.shape[0]) // 3 * 2, int(f.shape[1])
        elif f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise ValueError("FrameRowsU8: frames must be uint8 [Hs, Ws, 3], got %s %s" % (f.dtype, tuple(f.shape)))
        else:
            hs, ws = int(f.shape[0]), int(f.shape[1])
        if hs > self.max_frame_hw[0] or ws > self.max_frame_hw[1]:
            raise ValueError("FrameRowsU8: a %dx%d frame is above max_frame_hw %dx%d" % ((hs, ws) + self.max_frame_hw))
        dec, r = row_geometry((hs, ws), self.canvas, decimate)
        if divisor is None:
            if r is None:
                raise ValueError("FrameRowsU8: decimate -1 has no single ratio, pass divisor")
            divisor = r
        if fmt == PIX_NV12:
            self.arena[b, :hs * ws * 3 // 2].view(hs * 3 // 2, ws).copy_(f, non_blocking=True)
        else:
            self.arena[b, :hs * ws * 3].view(hs, ws, 3).copy_(f, non_blocking=True)
        self._rows[b] = self._staged_row(self.arena.data_ptr() + b * self.arena.stride(0), hs, ws,
                                         ws if fmt == PIX_NV12 else ws * 3, dec, 1 if mirror else 0, fmt)
        self._div[b] = divisor

    @staticmethod
    def _staged_row(ptr, hs, ws, row_stride, dec, mirror, fmt):
        """One table row of a frame in the single-allocation layout (all zeros, decimate 1: no frame)."""
        return (ptr, hs, ws, row_stride, dec, mirror, fmt)

    def upload(self):
        """The rows as set_row left them -> the device table: ONE non-blocking copy on the current stream."""
        self._at = (self._at + 1) % len(self._ring)
        if self._done[self._at] is not None:
            self._done[self._at].synchronize()                       # (only when the device is a whole ring of ticks behind)
        host = self._ring[self._at].numpy()
        n = self._DESC.itemsize * self.batch
        host[:n] = self._rows.view(np.uint8)
        host[n:] = self._div.view(np.uint8)
        self._buf.copy_(self._ring[self._at], non_blocking=True)
        if self._buf.is_cuda:
            ev = self._done[self._at] or torch.cuda.Event()
            ev.record()
            self._done[self._at] = ev

    # ---- FramePairsU8's surface ----------------------------------------------------------------------------
    def resized(self, tsize):
        """Same rows (shared arena and table), run at `tsize`."""
        other = copy.copy(self)
        other.out_size = (int(tsize[0]), int(tsize[1]))
        return other

    def paired_with_self(self):
        raise ValueError("FrameRowsU8 is an on_pipe input (one frame per row)")

    def to_nchw(self):
        """fp32 [batch, 3, Ho, Wo] of the rows last uploaded."""
        out = torch.empty(tuple(self.shape), dtype=torch.float32, device=self.device)
        self._pack(out)
        return out

    def pack_focus(self, cur_view, sup_view=None):
        """Write the stem operand (Focus-packed NHWC16 View of the plan) straight from the rows last uploaded."""
        assert sup_view is None
        self._pack(cur_view)

    def _pack(self, out):
        ops.frames_u8_pack_rows(self.table, self.batch, self.canvas, self.out_size, out)


_INT16 = tuple(t for t in (torch.int16, getattr(torch, "uint16", None)) if t is not None)


class Surface:
    """One camera frame as a hardware decoder hands it over, to be read WHERE IT LIES (FrameSurfacesU8, sy_frame_surf): no copy
    into a staging arena, no repacking of a padded surface.

    planes, by pixel_format:
      "bgr" / "rgb"  one uint8 tensor [Hs, Ws, 3] with strides (pitch, 3, 1), pitch >= 3 Ws (a column slice of a wider image);
      "nv12"         (luma [Hs, Ws], chroma [Hs/2, Ws]) uint8, strides (pitch, 1) each; Hs, Ws even; the chroma rows hold the
                     interleaved (U, V) pairs.  The two pitches may differ, the planes may be views of one allocation (a luma
                     plane padded to 1088 rows, chroma behind it) or separate tensors;
      "p010"         the same two planes of little-endian 16-bit samples with the significant bits on top, as byte views
                     [Hs, 2 Ws] / [Hs/2, 2 Ws] or as 16-bit integer tensors [Hs, Ws] / [Hs/2, Ws].  The pipeline uses each
                     word's high byte (word >> 8, truncation) as the 8-bit sample and then treats the frame as NV12 — the
                     project's own definition, see DESIGN.md.
    ValueError for anything else.  The tensors are kept (not copied): whoever owns them must not rewrite them until the tick
    that reads them has run on the device (FrameSurfacesU8)."""

    def __init__(self, planes, pixel_format):
        fmt = pixel_format_code(pixel_format, surfaces=True)
        planes = (planes,) if isinstance(planes, torch.Tensor) else tuple(planes)
        yuv = fmt in (PIX_NV12, PIX_P010)
        if len(planes) != (2 if yuv else 1) or not all(isinstance(p, torch.Tensor) for p in planes):
            raise ValueError("Surface: %r takes %s, got %d object(s)" % (pixel_format, "(luma, chroma) tensors" if yuv else "one tensor",
                                                                        len(planes)))
        if fmt == PIX_P010:                                          # 16-bit samples -> the bytes they are stored as
            planes = tuple(self._bytes(p) for p in planes)
        for p in planes:
            if p.dtype != torch.uint8 or p.dim() != (2 if yuv else 3) or p.stride(-1) != 1 or p.shape[0] < 1 or p.shape[1] < 1:
                raise ValueError("Surface: %r planes are uint8 %s with innermost stride 1, got %s %s strides %s"
                                 % (pixel_format, "[rows, bytes]" if yuv else "[Hs, Ws, 3]", p.dtype, tuple(p.shape), p.stride()))
            if p.device != planes[0].device:
                raise ValueError("Surface: planes on %s and %s" % (planes[0].device, p.device))
        y = planes[0]
        if yuv:
            step = 2 if fmt == PIX_P010 else 1
            hs, row_bytes = int(y.shape[0]), int(y.shape[1])
            ws = row_bytes // step
            if hs % 2 or ws % 2 or row_bytes != ws * step:
                raise ValueError("Surface: %r frames have even sizes, got a luma plane of %d rows of %d bytes" % (pixel_format, hs, row_bytes))
            if tuple(planes[1].shape) != (hs // 2, row_bytes):
                raise ValueError("Surface: a %s luma plane %s goes with a chroma plane %s, got %s"
                                 % (pixel_format, tuple(y.shape), (hs // 2, row_bytes), tuple(planes[1].shape)))
        else:
            hs, ws, row_bytes = int(y.shape[0]), int(y.shape[1]), 3 * int(y.shape[1])
            if y.shape[2] != 3 or y.stride(1) != 3:
                raise ValueError("Surface: %r pixels are [Hs, Ws, 3] with strides (pitch, 3, 1), got %s strides %s"
                                 % (pixel_format, tuple(y.shape), y.stride()))
        # (torch leaves the stride of a one-row dimension undefined: such a plane has no second row to find)
        pitches = tuple(int(p.stride(0)) if p.shape[0] > 1 else max(int(p.stride(0)), row_bytes) for p in planes)
        if min(pitches) < row_bytes or max(pitches) >= 1 << 31:
            raise ValueError("Surface: pitches %r for rows of %d bytes" % (pitches, row_bytes))
        self.planes, self.pixel_format, self.format = planes, pixel_format, fmt
        self.hw, self.pitch, self.chroma_pitch = (hs, ws), pitches[0], pitches[-1] if yuv else 0

    @staticmethod
    def _bytes(p):
        if p.dtype in _INT16 and p.dim() == 2 and p.stride(1) == 1:
            return p.view(torch.uint8)                               # [rows, Ws] words -> [rows, 2 Ws] bytes, little endian
        return p

    @classmethod
    def from_buffer(cls, buf, hs, ws, pixel_format, chroma_row=None):
        """The usual single-buffer surface: `buf` uint8 [rows, pitch]; the frame's rows start at row 0 and — "nv12" / "p010" —
        its chroma rows at row `chroma_row` (default hs; a decoder that pads the luma plane: the padded height)."""
        fmt = pixel_format_code(pixel_format, surfaces=True)
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 2:
            raise ValueError("Surface.from_buffer: buf is a uint8 tensor [rows, pitch]")
        hs, ws = int(hs), int(ws)
        row_bytes = ws * (1 if fmt == PIX_NV12 else 2 if fmt == PIX_P010 else 3)
        if fmt not in (PIX_NV12, PIX_P010):
            if hs < 1 or ws < 1 or buf.shape[0] < hs or buf.shape[1] < row_bytes:
                raise ValueError("Surface.from_buffer: a %dx%d %s frame in a buffer %s" % (hs, ws, pixel_format, tuple(buf.shape)))
            return cls(buf[:hs, :row_bytes].unflatten(1, (ws, 3)), pixel_format)
        c0 = hs if chroma_row is None else int(chroma_row)
        if hs < 2 or ws < 2 or hs % 2 or c0 < hs or buf.shape[0] < c0 + hs // 2 or buf.shape[1] < row_bytes:
            raise ValueError("Surface.from_buffer: a %dx%d %s frame with chroma at row %d in a buffer %s"
                             % (hs, ws, pixel_format, c0, tuple(buf.shape)))
        return cls((buf[:hs, :row_bytes], buf[c0:c0 + hs // 2, :row_bytes]), pixel_format)

    @property
    def device(self):
        return self.planes[0].device

    def clone(self):
        """A copy in memory of its own (on the same device, copied on the current stream) with the same format, sizes and
        pitches: every plane gets its own allocation of rows x pitch bytes.  What to draw on (overlay.py) while the decoder may
        still hold the original as a reference frame."""
        planes = []
        for p, pitch in zip(self.planes, (self.pitch, self.chroma_pitch)):
            buf = torch.empty((p.shape[0], pitch), dtype=torch.uint8, device=p.device)
            q = buf[:, :p.shape[1] * (3 if p.dim() == 3 else 1)]
            q = q.unflatten(1, (p.shape[1], 3)) if p.dim() == 3 else q
            q.copy_(p)
            planes.append(q)
        return Surface(planes[0] if len(planes) == 1 else tuple(planes), self.pixel_format)


# sy_frame_surf (include/streamyolo_hip.h), one per batch row
_SURF_DTYPE = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("Hs", "<i4"), ("Ws", "<i4"), ("row_stride", "<i4"),
                        ("chroma_stride", "<i4"), ("decimate", "<i4"), ("mirror", "<i4"), ("format", "<i4"), ("reserved", "<i4")])
assert _SURF_DTYPE.itemsize == 48


class FrameSurfacesU8(FrameRowsU8):
    """FrameRowsU8 whose rows may be decoder surfaces read in place: the table holds sy_frame_surf descriptors (both planes'
    addresses and pitches) and the launch is sy_frames_u8_pack_surfaces — still ONE launch for any mix of rows.

    set_row(b, Surface(...)) writes the planes' addresses and pitches into the table and copies NOTHING: the arena is not touched.
    set_row with a plain array or tensor stages it into the arena exactly as FrameRowsU8 does (a descriptor with plane1 = NULL);
    "p010" frames come as a Surface only.  upload / to_nchw / pack_focus / resized are FrameRowsU8's.

    Lifetime.  The object keeps a reference to a row's plane tensors until that row is set again, so their memory cannot be
    freed under a pending launch.  What it cannot do is stop the owner from WRITING to them: a surface must not be rewritten
    (handed back to the decoder) until the tick that reads it has run on the device — record an event on the tick's stream after
    the tick and wait for it, as with any zero-copy input.

        rows = FrameSurfacesU8(batch, (Hmax, Wmax), canvas, device)
        rows.set_row(0, Surface.from_buffer(decoded, 1080, 1920, "nv12", chroma_row=1088)); rows.set_row(1, frame_b)
        rows.upload(); model(rows, mode="on_pipe")"""

    _DESC = _SURF_DTYPE
    _KEY = "surfaces"

    def __init__(self, batch, max_frame_hw, canvas, device, out_size=None):
        self._held = [None] * int(batch)                             # row -> the plane tensors its descriptor points into
        super().__init__(batch, max_frame_hw, canvas, device, out_size)

    @staticmethod
    def _staged_row(ptr, hs, ws, row_stride, dec, mirror, fmt):
        return (ptr, 0, hs, ws, row_stride, 0, dec, mirror, fmt, 0)  # plane1 = NULL: chroma at row hs, the same pitch

    def _pack(self, out):
        ops.frames_u8_pack_surfaces(self.table, self.batch, self.canvas, self.out_size, out)

    def set_row(self, b, frame, mirror=False, decimate=None, divisor=None, pixel_format=None):
        """FrameRowsU8.set_row; `frame` may also be a Surface (pixel_format None or the surface's own), which must live on this
        object's device.  ValueError — before anything is written — for what the object or the kernel would refuse."""
        if not isinstance(frame, Surface):
            super().set_row(b, frame, mirror, decimate, divisor, "bgr" if pixel_format is None else pixel_format)
            self._held[b] = None
            return
        if not 0 <= b < self.batch:
            raise ValueError("FrameSurfacesU8: row %r of %d" % (b, self.batch))
        if pixel_format is not None and pixel_format != frame.pixel_format:
            raise ValueError("FrameSurfacesU8: a %r surface given as %r" % (frame.pixel_format, pixel_format))
        if frame.device != self.arena.device:
            raise ValueError("FrameSurfacesU8: a surface on %s cannot be read in place from %s (copy it, or pass the array to have "
                             "it staged)" % (frame.device, self.arena.device))
        dec, r = row_geometry(frame.hw, self.canvas, decimate)
        if divisor is None:
            if r is None:
                raise ValueError("FrameSurfacesU8: decimate -1 has no single ratio, pass divisor")
            divisor = r
        yuv = len(frame.planes) == 2
        self._rows[b] = (frame.planes[0].data_ptr(), frame.planes[1].data_ptr() if yuv else 0, frame.hw[0], frame.hw[1],
                         frame.pitch, frame.chroma_pitch, dec, 1 if mirror else 0, frame.format, 0)
        self._div[b] = divisor
        self._held[b] = frame.planes


def preprocess(inputs, targets, tsize, input_size):
    """`Exp.preprocess(inputs, targets, tsize)` (cfgs/l_s50_onex_dfp_tal_filp.py:161-172) with `self.input_size`
    passed explicitly: resize the batch to `tsize` (bilinear, align_corners=False) and scale both target tensors
    IN PLACE (x columns 1::2 by scale_x, y columns 2::2 by scale_y), or return everything unchanged when
    tsize == input_size.  `inputs`: the reference's fp32 [B,6,H,W] tensor (resized by sy_resize_bilinear_nchw) or a
    FramePairsU8 (the resize is deferred into the pack kernel)."""
    scale_y = tsize[0] / input_size[0]
    scale_x = tsize[1] / input_size[1]
    if scale_x != 1 or scale_y != 1:
        if isinstance(inputs, FramePairsU8):
            inputs = inputs.resized(tsize)
        else:
            x = inputs.float().contiguous()
            out = torch.empty((x.shape[0], x.shape[1], int(tsize[0]), int(tsize[1])), dtype=torch.float32, device=x.device)
            ops.resize_bilinear_nchw(x, out)
            inputs = out.to(inputs.dtype)
        targets[0][..., 1::2] = targets[0][..., 1::2] * scale_x
        targets[0][..., 2::2] = targets[0][..., 2::2] * scale_y
        targets[1][..., 1::2] = targets[1][..., 1::2] * scale_x
        targets[1][..., 2::2] = targets[1][..., 2::2] * scale_y
    return inputs, targets


class DevicePrefetcher:
    """`DataPrefetcher` (exps/train_utils/double_data_prefetcher.py:8-56) for uint8 frame batches: the next batch's
    H2D copies run on a side stream while the current step computes; `next()` makes the current stream wait for
    them and pins their memory to it (`record_stream`), exactly as the reference hands its fp32 batch over.

    `loader` yields ((cur_u8 [B,Hs,Ws,3], sup_u8, mirror [B] or None), (labels, support_labels), ...); with
    pixel_format "nv12" the frames are [B,Hs*3/2,Ws] (decoder output), see FramePairsU8."""

    def __init__(self, loader, canvas, decimate=1, device="cuda", pixel_format="bgr"):
        self.loader = iter(loader)
        self.canvas, self.decimate, self.device = canvas, decimate, torch.device(device)
        pixel_format_code(pixel_format)                              # (ValueError for an unknown one, before the first batch)
        self.pixel_format = pixel_format
        self.stream = torch.cuda.Stream(self.device)
        self.preload()

    def preload(self):
        try:
            item = next(self.loader)
        except StopIteration:
            self.next_input = self.next_target = None
            return
        (cur, sup, mirror), target = item[0], item[1]
        with torch.cuda.stream(self.stream):
            cur = cur.to(self.device, non_blocking=True)
            sup = None if sup is None else sup.to(self.device, non_blocking=True)
            mirror = None if mirror is None else torch.as_tensor(mirror, dtype=torch.uint8).to(self.device, non_blocking=True)
            self.next_input = FramePairsU8(cur, sup, self.canvas, self.decimate, mirror, pixel_format=self.pixel_format)
            self.next_target = (target[0].to(self.device, non_blocking=True), target[1].to(self.device, non_blocking=True))

    def next(self):
        cs = torch.cuda.current_stream(self.device)
        cs.wait_stream(self.stream)
        inp, target = self.next_input, self.next_target
        if inp is not None:
            for t in (inp.cur, inp.sup, inp.mirror):
                if t is not None:
                    t.record_stream(cs)
        if target is not None:
            target[0].record_stream(cs)
            target[1].record_stream(cs)
        self.preload()
        return inp, target

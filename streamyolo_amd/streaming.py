"""Streaming harness + evaluator glue: the callers on either side of the on_pipe hot path.

Mirrors, name for name where the reference has a name:
  inference()                 sAP/streamyolo/streamyolo_det.py:62-83     decoded output -> (boxes / in_scale, scores, labels, None)
  StreamingDetector           streamyolo_det.py:96-124, :176-181         model.half() on_pipe loop state (buffer), warm-up, one frame
  MultiStreamDetector         the same loop state for MANY cameras       one batched on_pipe plan, per-stream buffers in device pools
  run_sequence()              streamyolo_det.py:138-199                  the real-time scheduling loop of one sequence
  runtime_summary()           streamyolo_det.py:201-229 + sAP/util print_stats   timing statistics
  pair_with_ground_truth()    sAP/streamyolo/streaming_eval.py:74-139    time-based prediction / ground-truth pairing -> COCO dicts
  convert_to_coco_format()    exps/evaluators/onex_stream_evaluator.py:167-209   offline evaluator rows with the +1 frame-id shift

Per-pixel and per-box arithmetic is on the device (sy_frames_u8_pack, the on_pipe plan, sy_postprocess); this file is the
Python control flow the reference also keeps in Python.  Dataset access (pycocotools) and image decoding (cv2.imread)
stay with the caller: every function takes plain lists / arrays.
"""
import os
import time

import numpy as np
import torch

from . import ops
from ._lib import PIX_NV12, pixel_format_code
from .data import FramePairsU8, FrameRowsU8, FrameSurfacesU8, Surface, row_geometry
from .postprocess import DetectionPolicy, _as_policy, postprocess_device


def inference(outputs, num_classes=8, conf_thre=0.01, nms_thresh=0.65, in_scale=0.5):
    """`inference(result[0])` of streamyolo_det.py:62-83 for ONE image's decoded rows [A, 5+nc] (or [1, A, 5+nc]):
    returns (bboxes xyxy / in_scale, scores = obj * class_conf, labels int32, None) as numpy arrays in descending
    score order.  Filter + class-aware NMS run in sy_postprocess; one D2H copy of the kept rows."""
    pred = outputs if outputs.dim() == 3 else outputs.unsqueeze(0)
    det, _, cnt = postprocess_device(pred, num_classes, conf_thre, nms_thresh)
    return _parse(det, cnt, in_scale)


def frame_shape(frame_hw, pixel_format="bgr"):
    """Shape of one uint8 camera frame of size frame_hw = (h, w): (h, w, 3) for "bgr" / "rgb", (h * 3 / 2, w) for "nv12" (luma
    rows, then the interleaved chroma rows).  ValueError for an unknown format or an odd NV12 size."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    if pixel_format_code(pixel_format) != PIX_NV12:
        return (h, w, 3)
    if h % 2 or w % 2:
        raise ValueError("NV12 frames have even sizes, got %dx%d" % (h, w))
    return (h * 3 // 2, w)


def _stream_shape(frame_hw, pixel_format, surfaces):
    """frame_shape() for a stream of a detector; surfaces=True knows "p010" too, whose frames come as data.Surface only: None."""
    if surfaces and pixel_format == "p010":
        if int(frame_hw[0]) % 2 or int(frame_hw[1]) % 2:
            raise ValueError("P010 frames have even sizes, got %dx%d" % (int(frame_hw[0]), int(frame_hw[1])))
        return None
    return frame_shape(frame_hw, pixel_format)


def _parse(det, cnt, in_scale):
    """Kept rows [n, 7] of image 0 -> the reference's (bboxes / in_scale, scores, labels, None) host arrays."""
    n = int(cnt[0])
    d = det[0, :n].cpu().numpy()
    return d[:, :4] / in_scale, d[:, 4] * d[:, 5], d[:, 6].astype(np.int32), None


class TrackConfig:
    """Options of the device tracker behind the NMS (MultiStreamDetector(track=...); csrc/track.hip).  The defaults are the
    reference's constants: match_iou_th (pps_forecast_kf.py:40), r / q / p_init = the diagonals of kf_R, kf_Q and kf_P_init
    (:129-132), min_size (extrap_clean_up, sAP/forecast/__init__.py:33).  max_tracks: tracks kept per stream, at most 256; a
    frame's detections beyond it (the lowest scores) are dropped by the tracker."""

    def __init__(self, match_iou_th=0.3, r=10.0, q=1.0, p_init=100.0, min_size=75, max_tracks=256):
        from ._lib import TRACK_MAX_TRACKS
        if not 1 <= int(max_tracks) <= TRACK_MAX_TRACKS:
            raise ValueError("TrackConfig: max_tracks must be in 1..%d, got %r" % (TRACK_MAX_TRACKS, max_tracks))
        if not float(match_iou_th) > 0.0:
            raise ValueError("TrackConfig: match_iou_th must be positive, got %r" % (match_iou_th,))
        self.match_iou_th, self.r, self.q, self.p_init = float(match_iou_th), float(r), float(q), float(p_init)
        self.min_size, self.max_tracks = int(min_size), int(max_tracks)

    def __repr__(self):
        return "TrackConfig(match_iou_th=%r, r=%r, q=%r, p_init=%r, min_size=%r, max_tracks=%r)" % (
            self.match_iou_th, self.r, self.q, self.p_init, self.min_size, self.max_tracks)


class StreamingDetector:
    """The model-side state of streamyolo_det.py's loop: `model.eval().half()` (:104-109), ten warm-up calls (:113-120),
    then per camera frame `preproc` -> `model(frame, buffer=buffer, mode='on_pipe')` -> `inference` (:176-181), the
    buffer being reset at every sequence start (:150).

    Frames are the raw uint8 HWC arrays `cv2.imread` returns.  The reference resizes every frame to
    (h_img, w_img) = (int(H * in_scale), int(W * in_scale)) with cv2.resize(img, (w_img, h_img)) (:176-178: truncation, each
    axis stretched on its own): with in_scale = 0.5 on even frames that is the exact 2x decimation, with any other in_scale
    OpenCV's fixed-point bilinear resize — both done on the device together with the Focus packing (sy_frames_u8_pack,
    csrc/input_pipeline.hip).  pixel_format "rgb" / "nv12": the frames arrive in that format (frame_shape()) and the same
    launch converts them, as cv2.cvtColor in front of the loop would.

    Every frame is copied into the detector's own slot: its tape carries the frame pointer by value, so a per-frame pointer cannot
    ride in it.  A single camera whose decoder surfaces should be read in place (data.Surface) uses
    MultiStreamDetector(batch=1, surfaces=True), whose pointers are table data.

    policy=DetectionPolicy(...): what counts as a detection beyond the two thresholds — a class list, class-agnostic NMS, caps on
    the candidates and on the detections; the post step is then sy_postprocess_rows over a one-row table."""

    def __init__(self, model, frame_hw, in_scale=0.5, num_classes=8, conf_thre=0.01, nms_thresh=0.65, dtype="fp16",
                 device="cuda", pixel_format="bgr", policy=None):
        self.pixel_format = pixel_format
        self._frame_shape = frame_shape(frame_hw, pixel_format)      # (ValueError before anything is built)
        self.policy = None if policy is None else _as_policy(policy)
        row = None if policy is None else self.policy.record(num_classes, conf_thre, nms_thresh)
        self.model = model.to(device).eval().set_compute_dtype(dtype)
        self.device = torch.device(device)
        self.in_scale = in_scale
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        # h_img, w_img = int(1200 * in_scale), int(1920 * in_scale) (streamyolo_det.py:177): truncation, per axis
        self.canvas = (int(self.frame_hw[0] * in_scale), int(self.frame_hw[1] * in_scale))
        if self.canvas[0] % 2 or self.canvas[1] % 2:
            raise ValueError("StreamingDetector: in_scale %r gives an odd %dx%d network input (the Focus stem needs even sizes)"
                             % (in_scale, self.canvas[0], self.canvas[1]))
        if self.canvas == self.frame_hw:
            self.decimate = 1
        elif (2 * self.canvas[0], 2 * self.canvas[1]) == self.frame_hw:
            self.decimate = 2
        else:
            self.decimate = -1                                    # per-axis fixed-point bilinear stretch to the canvas
        self.num_classes, self.conf_thre, self.nms_thresh = num_classes, conf_thre, nms_thresh
        self._slot = torch.empty((1,) + self._frame_shape, dtype=torch.uint8, device=self.device)
        self._in = FramePairsU8(self._slot, None, self.canvas, self.decimate, pixel_format=pixel_format)
        # 16-bit speed modes: the deep small-map layers may run as split-K (different fp32 summation order than the facade's
        # exact path — a plan object of its own); the fp32 parity mode keeps the single-pass kernels
        split_k = str(dtype) not in ("fp32", "torch.float32") and os.environ.get("STREAMYOLO_STREAM_SPLITK", "1") != "0"
        self.plan = model._plans.inference(model.backbone, model.head, "on_pipe", self._in, owner=model, split_k=split_k)
        self._first = True
        self._last = None                                            # (det, cnt) of the latest frame (draw)
        self._overlay = self._style = None
        self._crop_rows, self._crop_spec, self._crop_out = None, None, None  # crops(): the sy_crop_row table, the default spec, crops.CropCache
        self._redact_rows = self._redact_spec = None                 # redact(): the sy_redact_row table, the default spec
        self._post = lambda out: postprocess_device(out, num_classes, conf_thre, nms_thresh)   # one object: part of the tape key
        if row is not None:
            # a DetectionPolicy (class list, class-agnostic NMS, caps): the post step is sy_postprocess_rows over a one-row table
            self._table = ops.det_policy_table([row], self.device)
            self._ws = ops.PostprocessWorkspace(1, self.plan.A, self.device)
            self._post = lambda out: ops.postprocess_rows(out, num_classes, self._table, self._ws)

    def warm_up(self, n=10):
        """streamyolo_det.py:113-120 (ten calls on a dummy frame; here they also build / tune the plan)."""
        self._slot.fill_(1)
        with torch.no_grad():
            for i in range(n):
                self.plan.run_stream(self._in, first=(i == 0))
        torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        self.reset()

    def reset(self):
        """`buffer = None` at the start of a sequence (:150): the next frame fuses with itself (node 'star')."""
        self._first = True

    def __call__(self, frame):
        """One camera frame (uint8 [H, W, 3] numpy array or tensor; [H*3/2, W] for "nv12") -> (bboxes, scores, labels, None),
        host arrays.  Ends with the device synchronised (the D2H copy of the detections), as the reference's loop does (:183)."""
        f = torch.as_tensor(frame)
        assert f.dtype == torch.uint8 and tuple(f.shape) == self._frame_shape
        self._slot[0].copy_(f, non_blocking=True)
        with torch.no_grad():
            if self._first:                                   # node 'star': extra fan-in copies, through the wrappers
                self._first = False
                out = self.plan.run_stream(self._in, first=True)
                det, _, cnt = self._post(out)                     # (without a policy: exactly inference(out, ...)'s NMS call)
                self._last = (det, cnt)
                return _parse(det, cnt, self.in_scale)
            # steady state: the ~140 launches of the frame (pack, network, decode, NMS) replayed from a launch tape
            det, _, cnt = self.plan.run_stream_taped(self._in, post=self._post, check_params=False)
            self._last = (det, cnt)
            return _parse(det, cnt, self.in_scale)

    def draw(self, surface, style=None):
        """Draw the latest frame's detections into `surface` (a data.Surface, or a uint8 device tensor [H, W, 3] taken as BGR, of
        the camera's size), in place, and return it: MultiStreamDetector.draw over this detector's one row."""
        from .overlay import OverlayRows, OverlayStyle, as_target, draw_rows
        if style is None:
            style = self._style = self._style or OverlayStyle()
        elif not isinstance(style, OverlayStyle):
            raise ValueError("StreamingDetector: style must be an OverlayStyle, got %r" % (style,))
        if self._last is None:
            raise ValueError("StreamingDetector: no frame has been detected yet")
        det, cnt = self._last
        target = as_target(surface, det.device, self.frame_hw, "StreamingDetector")
        if self._overlay is None:
            self._overlay = OverlayRows(1, det.device)
        self._overlay.set_row(0, target, self.in_scale, style)
        self._overlay.upload()
        draw_rows(self._overlay, self.frame_hw, det, 0, None, cnt, style)
        return surface

    def redact(self, surface, spec=None):
        """Pixelate or fill the latest frame's detections in `surface` (a data.Surface, or a uint8 device tensor [H, W, 3] taken
        as BGR, of the camera's size), in place, and return it: MultiStreamDetector.redact over this detector's one row.  IN
        PLACE — redact a `clone()` while the decoder may still hold the surface as a reference frame; redact() before draw()."""
        from .redact import RedactRows, RedactSpec, as_target, check_spec, redact_rows
        if spec is None:
            spec = self._redact_spec = self._redact_spec or RedactSpec()
        check_spec(spec, "StreamingDetector")
        if self._last is None:
            raise ValueError("StreamingDetector: no frame has been detected yet")
        det, cnt = self._last
        target = as_target(surface, det.device, self.frame_hw, "StreamingDetector")
        if self._redact_rows is None:
            self._redact_rows = RedactRows(1, det.device)
        self._redact_rows.set_row(0, target, self.in_scale, spec)
        self._redact_rows.upload()
        redact_rows(self._redact_rows, self.frame_hw, det, 0, cnt)
        return surface

    def crops(self, surface, spec=None):
        """Crop the latest frame's detections out of `surface` (a data.Surface, or a uint8 device tensor [H, W, 3] taken as BGR,
        of the camera's size) -> crops.Crops: MultiStreamDetector.crops over this detector's one row (row_sids = (0,))."""
        from .crops import CropCache, CropRows, CropSpec, as_source, check_spec, gather_rows
        if spec is None:
            spec = self._crop_spec = self._crop_spec or CropSpec()
        check_spec(spec, "StreamingDetector")
        if self._last is None:
            raise ValueError("StreamingDetector: no frame has been detected yet")
        det, cnt = self._last
        source = as_source(surface, det.device, self.frame_hw, "StreamingDetector")
        if self._crop_rows is None:
            self._crop_rows = CropRows(1, det.device)
        if self._crop_out is None:
            self._crop_out = CropCache()
        out = self._crop_out.get(spec, 1, det.device)
        out.row_sids, spec = (0,), out.spec
        self._crop_rows.set_row(0, source, self.in_scale, spec)
        self._crop_rows.upload()
        return gather_rows(self._crop_rows, det, 0, None, cnt, spec, out)


class MultiStreamDetector:
    """StreamingDetector for many cameras at once: ONE on_pipe plan of `batch` rows serves whichever of up to `max_streams`
    open streams have a frame ready.  Every stream keeps its own `buffer` (streamyolo_det.py:150, :180: reset at its sequence
    start, carried from its previous frame) as a slot of per-level device pools; a tick names, per batch row, the slot it
    belongs to and whether its sequence starts here, in two small device tables the state kernels read
    (sy_stream_state_gather / _scatter).  Cameras need not tick in lockstep: a stream that has no frame in a tick is simply
    not in it, and its state stays as it is.  First frames are data, not control flow: after warm_up() every tick is one
    replay of the same launch tape.

        det = MultiStreamDetector(model, (1200, 1920), max_streams=16, batch=8); det.warm_up()
        a, b = det.open(), det.open()
        (boxes_a, scores_a, labels_a, _), (boxes_b, scores_b, labels_b, _) = det([frame_a, frame_b], [a, b])

    Without `max_frame_hw` all streams share the one frame size `frame_hw`.  With max_frame_hw=(Hmax, Wmax) the detector runs
    in mixed mode: open(frame_hw=(h, w)) fixes a stream's own camera size for its lifetime, and cameras of different
    resolutions share the ticks — every batch row is the same canvas-sized network input, and the pack kernel reads each row's
    size, resize mode and pixels from a device table (sy_frames_u8_pack_rows, data.FrameRowsU8), so the mix is data too and
    the tape stays the one tape.  A stream opened with a size is letterboxed the way `preproc` does it (a frame of the canvas
    size is copied, one of exactly twice the canvas decimated 2x, any other resized by r = min(H / h, W / w) onto the 114
    canvas) and its boxes are divided by that r, as the evaluators do; a stream opened without one is a `frame_hw` camera
    treated exactly as in the uniform mode.

    pixel_format ("bgr", "rgb", "nv12") is the format the cameras deliver (frame_shape()); the pack launch converts.  In mixed
    mode it is the default of open(), which may name another per stream: the format sits in the row table beside the size, so
    cameras of different formats share ticks and the one tape too.

        det = MultiStreamDetector(model, (1200, 1920), max_streams=16, batch=8, max_frame_hw=(2048, 2048)); det.warm_up()
        ring, side = det.open(), det.open(frame_hw=(1550, 2048))
        (boxes_r, ...), (boxes_s, ...) = det([ring_frame, side_frame], [ring, side])

    surfaces=True is the mixed mode over data.FrameSurfacesU8 (max_frame_hw defaults to frame_hw): a tick's frames may mix plain
    arrays (staged, as above) and data.Surface objects — decoder output read where it lies, padded or split planes included,
    nothing copied — and open(pixel_format="p010") is accepted (10-bit decoders; Surface only).  The pack launch is
    sy_frames_u8_pack_surfaces, still one per tick and the one tape.  A Surface must stay unwritten until its tick has run on the
    device (FrameSurfacesU8).

        det = MultiStreamDetector(model, (1080, 1920), batch=4, surfaces=True); det.warm_up()
        cam = det.open(pixel_format="nv12")
        det([Surface.from_buffer(decoded, 1080, 1920, "nv12", chroma_row=1088)], [cam])

    track=TrackConfig() (or True for its defaults) adds the reference's streaming post-processing step (pps_forecast_kf.py with
    --forecast-before-assoc) on the device: per stream, a Kalman filter per track, greedy IoU association of each frame's
    detections with the predicted tracks, and the boxes forecast `horizon` frames ahead, clipped to the stream's camera — one
    more launch on the same tape (sy_track_update), state in one more per-slot pool (engine.TrackSlots).  Calls then take
    frame_idx (one int per frame; default: the stream's previous index + 1; the filter's dt is the difference to the previous
    index, which must be >= 1 except at a sequence start) and horizon (a float or one per frame, default 0), results are
    5-tuples (bboxes, scores, labels, None, track_ids) — the forecast boxes in camera coordinates — and forecast(sids, horizon)
    moves the current tracks to another time without a frame.

        det = MultiStreamDetector(model, (1200, 1920), batch=8, track=True); det.warm_up()
        cam = det.open()
        (boxes, scores, labels, _, ids), = det([frame], [cam], frame_idx=[12], horizon=1.0)

    policy=DetectionPolicy(...) (or True for the defaults) makes what counts as a detection per-stream data as well: the tape
    holds sy_postprocess_rows, which reads one record per batch row — thresholds, the classes reported, class-agnostic NMS, caps
    on the candidates and on the detections (engine.PolicyTable, uploaded beside the slot table).  open(policy=...) gives a
    stream its own, set_policy(sid, policy) changes it between two ticks on the same tape; a stream without one follows the
    detector's.  Without policy= the tape holds sy_postprocess as before and per-stream policies are a ValueError.

        det = MultiStreamDetector(model, (1200, 1920), batch=8, policy=True); det.warm_up()
        cars = det.open(policy=DetectionPolicy(conf_thre=0.3, classes=[2, 3]))
        feed = det.open(policy=DetectionPolicy(class_agnostic=True, max_det=100))
        det.set_policy(cars, DetectionPolicy(conf_thre=0.5, classes=[2]))

    Which frames go into a tick is the caller's scheduling policy."""

    def __init__(self, model, frame_hw, max_streams=16, batch=8, in_scale=0.5, num_classes=8, conf_thre=0.01, nms_thresh=0.65,
                 dtype="fp16", device="cuda", max_frame_hw=None, pixel_format="bgr", surfaces=False, track=None, policy=None):
        self.pixel_format, self.surfaces = pixel_format, bool(surfaces)
        self.policy = None if policy is None or policy is False else _as_policy(policy)      # the default of its streams
        if self.policy is not None:
            self.policy.record(num_classes, conf_thre, nms_thresh)                  # (ValueError before anything is built)
        self._frame_shape = _stream_shape(frame_hw, pixel_format, self.surfaces)     # (ValueError before anything is built)
        if int(batch) < 1 or int(max_streams) < 1:
            raise ValueError("MultiStreamDetector: batch and max_streams must be positive")
        if max_frame_hw is not None:
            max_frame_hw = (int(max_frame_hw[0]), int(max_frame_hw[1]))
            if max_frame_hw[0] < int(frame_hw[0]) or max_frame_hw[1] < int(frame_hw[1]):
                raise ValueError("MultiStreamDetector: max_frame_hw %r is below frame_hw %r" % (max_frame_hw, tuple(frame_hw)))
        elif self.surfaces:
            max_frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.max_frame_hw = max_frame_hw
        self.model = model.to(device).eval().set_compute_dtype(dtype)
        self.device = torch.device(device)
        self.in_scale, self.batch, self.max_streams = in_scale, int(batch), int(max_streams)
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.canvas = (int(self.frame_hw[0] * in_scale), int(self.frame_hw[1] * in_scale))      # streamyolo_det.py:177
        if self.canvas[0] % 2 or self.canvas[1] % 2:
            raise ValueError("MultiStreamDetector: in_scale %r gives an odd %dx%d network input (the Focus stem needs even sizes)"
                             % (in_scale, self.canvas[0], self.canvas[1]))
        if self.canvas == self.frame_hw:
            self.decimate = 1
        elif (2 * self.canvas[0], 2 * self.canvas[1]) == self.frame_hw:
            self.decimate = 2
        else:
            self.decimate = -1
        self.num_classes, self.conf_thre, self.nms_thresh = num_classes, conf_thre, nms_thresh
        if self.max_frame_hw is None:
            # detector-owned staging: row b of a tick's frames (rows without a frame keep stale pixels; their outputs are ignored)
            self._stage = torch.zeros((self.batch,) + self._frame_shape, dtype=torch.uint8, device=self.device)
            self._in = FramePairsU8(self._stage, None, self.canvas, self.decimate, pixel_format=pixel_format)
        else:
            # mixed mode: a byte arena per row and the per-row descriptor table (rows without a frame are the plain canvas)
            self._stage = None
            self._in = (FrameSurfacesU8 if self.surfaces else FrameRowsU8)(self.batch, self.max_frame_hw, self.canvas, self.device)
        self._geom = {}                                          # mixed mode: open stream id -> (frame hw, decimate, box divisor)
        self._fmt = {}                                           # open stream id -> (pixel format, shape of its frames)
        split_k = str(dtype) not in ("fp32", "torch.float32") and os.environ.get("STREAMYOLO_STREAM_SPLITK", "1") != "0"
        self.plan = model._plans.inference(model.backbone, model.head, "on_pipe", self._in, owner=model, split_k=split_k)
        from .engine import StreamSlots
        self.state = StreamSlots(self.plan, self.max_streams)
        self._ws = ops.PostprocessWorkspace(self.batch, self.plan.A, self.device)          # its own: results live until the next tick
        self._post = lambda out: ops.postprocess(out, num_classes, conf_thre, nms_thresh, self._ws)   # one object: part of the tape key
        self.policies = None
        self._pol = {}                                           # open stream id -> its sy_det_policy record
        nms = self._post                                         # the NMS step of the tape: (det, index, cnt)
        if self.policy is not None:
            # per-stream policies: the tape holds sy_postprocess_rows, and what each row asks for is table data like its slot
            from .engine import PolicyTable
            self.policies = PolicyTable(self.batch, self.device)
            nms = self._post = lambda out: ops.postprocess_rows(out, num_classes, self.policies, self._ws)
        self.track = TrackConfig() if track is True else (track or None)
        self.tracks = None
        if self.track is not None:
            from .engine import TrackSlots
            cfg = self.track
            self.tracks = TrackSlots(self.plan, self.max_streams, cfg.max_tracks)
            self._track_prm = ops.track_params(cfg.match_iou_th, cfg.r, cfg.q, cfg.p_init, cfg.min_size)

            def post(out):                                       # the NMS, then the tracker on its output: one more launch
                det, index, cnt = nms(out)
                ops.track_update(det, cnt, self.state.row_slot, self.state.row_first, self.tracks.ticks, self.tracks.state,
                                 self._track_prm, self.tracks.out, self.tracks.out_id, self.tracks.out_cnt)
                return det, index, cnt
            self._post = post
        self._fidx = {}                                          # open stream id -> frame index of its previous frame (tracking)
        self._slot_of = {}                                       # open stream id -> pool slot
        self._first = {}                                         # open stream id -> its next frame starts a sequence
        self._free = list(range(self.max_streams))
        self._next_id = 0                                        # ids are never reused: a closed id stays invalid
        self._row_of = {}                                        # stream id -> its batch row in the latest tick (draw)
        self._last = None                                        # (det, cnt) of the latest tick
        self._overlay = self._style = None                       # draw(): the sy_overlay_row table, the default style
        self._crop_rows, self._crop_spec, self._crop_out = None, None, None  # crops(): the sy_crop_row table, the default spec, crops.CropCache
        self._redact_rows = self._redact_spec = None                 # redact(): the sy_redact_row table, the default spec

    # ---- stream bookkeeping (host side only) --------------------------------------------------------------------
    def _policy_record(self, policy):
        """The table record of a stream's policy (None: the detector's default).  ValueError: the detector has no policy table,
        or the policy does not fit it (class ids)."""
        if self.policy is None:
            if policy is None:
                return None
            raise ValueError("MultiStreamDetector: per-stream policies need a detector built with policy=... (True for the defaults)")
        if policy is not None and not isinstance(policy, DetectionPolicy):
            raise ValueError("MultiStreamDetector: policy must be a DetectionPolicy or None, got %r" % (policy,))
        return (self.policy if policy is None else policy).record(self.num_classes, self.conf_thre, self.nms_thresh)

    def set_policy(self, sid, policy):
        """Stream `sid` reports by `policy` (a DetectionPolicy; None: the detector's default) from its next tick on.  Table data:
        the launch tape stays the one it is.  ValueError — nothing changes — on a detector built without policy=."""
        self._known(sid)
        if self.policy is None:
            raise ValueError("MultiStreamDetector: set_policy needs a detector built with policy=... (True for the defaults)")
        self._pol[sid] = self._policy_record(policy)

    def open(self, frame_hw=None, pixel_format=None, policy=None):
        """A new stream: its id.  Its first frame fuses with itself (`buffer = None`, streamyolo_det.py:150).  Mixed mode:
        frame_hw = (h, w) is this stream's camera size for its lifetime (None: the detector's frame_hw and in_scale) and
        pixel_format its format (None: the detector's).  policy: the stream's DetectionPolicy (None: the detector's; needs a
        detector built with policy=; set_policy changes it later).  ValueError — nothing is taken — for what the detector
        cannot serve."""
        record = self._policy_record(policy)
        geom = (self.frame_hw, self.decimate, self.in_scale)
        if pixel_format is None:
            pixel_format = self.pixel_format
        pixel_format_code(pixel_format, surfaces=self.surfaces)
        if self.max_frame_hw is None and pixel_format != self.pixel_format:
            raise ValueError("MultiStreamDetector: a uniform detector serves %r frames only (open(pixel_format=%r)); build it "
                             "with max_frame_hw for per-stream formats" % (self.pixel_format, pixel_format))
        if frame_hw is not None:
            if self.max_frame_hw is None:
                raise ValueError("MultiStreamDetector: open(frame_hw=...) needs a detector built with max_frame_hw")
            hw = (int(frame_hw[0]), int(frame_hw[1]))
            if hw[0] > self.max_frame_hw[0] or hw[1] > self.max_frame_hw[1]:
                raise ValueError("MultiStreamDetector: a %dx%d camera is above max_frame_hw %dx%d" % (hw + self.max_frame_hw))
            decimate, r = row_geometry(hw, self.canvas)          # (ValueError: nothing of the frame is left on the canvas)
            geom = (hw, decimate, r)
        shape = _stream_shape(geom[0], pixel_format, self.surfaces)      # (ValueError: an odd NV12 / P010 size)
        if not self._free:
            raise RuntimeError("MultiStreamDetector: all %d streams are open" % self.max_streams)
        sid = self._next_id
        self._next_id += 1
        self._slot_of[sid] = self._free.pop(0)
        self._first[sid] = True
        self._geom[sid] = geom
        self._fmt[sid] = (pixel_format, shape)
        self._fidx[sid] = None
        if record is not None:
            self._pol[sid] = record
        return sid

    def _known(self, sid):
        if sid not in self._slot_of:
            raise ValueError("MultiStreamDetector: stream id %r is not open" % (sid,))

    def reset(self, sid):
        """A new sequence starts on stream `sid`: its next frame fuses with itself."""
        self._known(sid)
        self._first[sid] = True

    def close(self, sid):
        """Stream `sid` ends: its slot is free for the next open()."""
        self._known(sid)
        self._free.append(self._slot_of.pop(sid))
        self._free.sort()
        del self._first[sid]
        del self._geom[sid]
        del self._fmt[sid]
        del self._fidx[sid]
        self._pol.pop(sid, None)
        self._row_of.pop(sid, None)

    def warm_up(self, n=10):
        """streamyolo_det.py:113-120 on a dummy batch (no row carries a frame: no stream's state is written); builds, tunes and
        records the plan.  Afterwards every open stream starts a new sequence."""
        if self._stage is not None:
            self._stage.fill_(1)
        else:
            for b in range(self.batch):
                self._in.set_row(b, None)
            self._in.upload()
        self.state.set_rows((), ())
        self.state.upload()
        if self.tracks is not None:
            self.tracks.set_rows(())
            self.tracks.upload()
        if self.policies is not None:
            self.policies.set_rows(())
            self.policies.upload()
        with torch.no_grad():
            for _ in range(max(int(n), 2)):                      # (a tuning + recording tick, then at least one replay)
                self.plan.run_stream_slots_taped(self._in, self.state, post=self._post)
        torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        for sid in self._first:
            self._first[sid] = True
        self._row_of = {}

    # ---- ticks -----------------------------------------------------------------------------------------------
    def _check(self, frames, sids):
        """Everything that can be wrong with a call, found BEFORE anything is written."""
        if len(frames) != len(sids):
            raise ValueError("MultiStreamDetector: %d frames for %d stream ids" % (len(frames), len(sids)))
        for t0 in range(0, len(sids), self.batch):
            tick = list(sids[t0:t0 + self.batch])
            for sid in tick:
                self._known(sid)
            if len(set(tick)) != len(tick):
                raise ValueError("MultiStreamDetector: a stream id appears twice in one tick: %r" % (tick,))
        fs = []
        for f, sid in zip(frames, sids):
            fmt, shape = self._fmt[sid]                          # its stream's format and camera size (uniform mode: frame_hw)
            if isinstance(f, Surface):
                if not self.surfaces:
                    raise ValueError("MultiStreamDetector: a Surface needs a detector built with surfaces=True")
                if f.pixel_format != fmt or f.hw != self._geom[sid][0] or f.device != self._in.device:
                    raise ValueError("MultiStreamDetector: stream %r takes %s surfaces of %dx%d on %s, got %s %dx%d on %s"
                                     % ((sid, fmt) + self._geom[sid][0] + (self._in.device, f.pixel_format) + f.hw + (f.device,)))
                fs.append(f)
                continue
            if shape is None:
                raise ValueError("MultiStreamDetector: frames of stream %r (%s) come as data.Surface" % (sid, fmt))
            f = torch.as_tensor(f)
            if f.dtype != torch.uint8 or tuple(f.shape) != shape:
                raise ValueError("MultiStreamDetector: frames of stream %r (%s) must be uint8 %s, got %s %s"
                                 % (sid, fmt, list(shape), f.dtype, tuple(f.shape)))
            fs.append(f)
        return fs

    def _check_times(self, sids, frame_idx, horizon):
        """Per frame (frame index, dt, horizon) of a call with tracking — found wrong BEFORE anything is written: ValueError."""
        n = len(sids)
        if self.tracks is None:
            if frame_idx is not None or horizon is not None:
                raise ValueError("MultiStreamDetector: frame_idx / horizon need a detector built with track=...")
            return [None] * n
        if frame_idx is not None and len(frame_idx) != n:
            raise ValueError("MultiStreamDetector: %d frame indices for %d frames" % (len(frame_idx), n))
        if horizon is None:
            horizon = 0.0
        hs = [float(horizon)] * n if np.isscalar(horizon) else [float(h) for h in horizon]
        if len(hs) != n:
            raise ValueError("MultiStreamDetector: %d horizons for %d frames" % (len(hs), n))
        prev, first, out = dict(self._fidx), dict(self._first), []
        for k, sid in enumerate(sids):
            start = first[sid] or prev[sid] is None
            idx = int(frame_idx[k]) if frame_idx is not None else (0 if prev[sid] is None else prev[sid] + 1)
            dt = 0 if start else idx - prev[sid]
            if not start and dt < 1:
                raise ValueError("MultiStreamDetector: frame index %d of stream %r does not follow its previous frame %d"
                                 % (idx, sid, prev[sid]))
            prev[sid], first[sid] = idx, False
            out.append((idx, dt, hs[k]))
        return out

    def _tick(self, frames, sids, times=None):
        n = len(sids)
        if self._stage is not None:
            for b, f in enumerate(frames):
                self._stage[b].copy_(f, non_blocking=True)
        else:
            for b in range(self.batch):
                if b < n:
                    _, decimate, div = self._geom[sids[b]]
                    self._in.set_row(b, frames[b], decimate=decimate, divisor=div, pixel_format=self._fmt[sids[b]][0])
                else:
                    self._in.set_row(b, None)
            self._in.upload()
        self.state.set_rows([self._slot_of[s] for s in sids], [self._first[s] for s in sids])
        self.state.upload()
        if self.policies is not None:
            self.policies.set_rows([self._pol[s] for s in sids])
            self.policies.upload()
        if self.tracks is not None:
            rows = []
            for s, (idx, dt, horizon) in zip(sids, times):
                (h, w), _, div = self._geom[s]
                rows.append((dt, horizon, w, h, div))
                self._fidx[s] = idx
            self.tracks.set_rows(rows)
            self.tracks.upload()
        for s in sids:
            self._first[s] = False
        with torch.no_grad():
            det, _, cnt = self.plan.run_stream_slots_taped(self._in, self.state, post=self._post)
        self._last, self._row_of = (det, cnt), {s: b for b, s in enumerate(sids)}
        return det, cnt, n

    def detect_device(self, frames, sids, frame_idx=None, horizon=None):
        """One tick (len(frames) <= batch) without any host read: (det [batch, A, 7], cnt [batch], rows) — rows 0..rows-1 of
        the device tensors belong to `sids` in order (kept detections det[b, :cnt[b]]: x1, y1, x2, y2 on the network input,
        obj, class_conf, class), the other rows are meaningless.  The tensors are detector-owned and overwritten by the next
        tick.  Frames are copied into the staging tensor, the tables go up in one non-blocking copy from pinned memory.
        Mixed mode returns a fourth value: the device tensor div [batch] (float32, detector-owned) — the boxes of row b divided
        by div[b] are in that stream's camera coordinates (what __call__ does on the host).
        With tracking, three more values follow: the tracker's device tensors out [batch, max_tracks, 6] (x1, y1, x2, y2, score,
        label of the forecast tracks, camera coordinates), out_id [batch, max_tracks] and out_cnt [batch] (engine.TrackSlots)."""
        if len(sids) > self.batch:
            raise ValueError("MultiStreamDetector: %d frames in one tick of batch %d" % (len(sids), self.batch))
        fs, sids = self._check(frames, sids), list(sids)
        res = self._tick(fs, sids, self._check_times(sids, frame_idx, horizon))
        if self._stage is None:
            res = res + (self._in.divisor,)
        return res if self.tracks is None else res + (self.tracks.out, self.tracks.out_id, self.tracks.out_cnt)

    def _parse_tracks(self, out, out_id, out_cnt, n):
        """Rows 0..n-1 of a tracker output -> (bboxes, scores, labels, None, track_ids) host tuples (one copy each: synchronises)."""
        counts = out_cnt[:n].cpu().numpy()
        top = max(int(counts.max()), 1)
        rows, ids = out[:n, :top].cpu().numpy(), out_id[:n, :top].cpu().numpy()
        return [(rows[b, :c, :4], rows[b, :c, 4], rows[b, :c, 5].astype(np.int32), None, ids[b, :c])
                for b, c in ((b, int(counts[b])) for b in range(n))]

    def forecast(self, sids, horizon=0.0):
        """The current tracks of the streams `sids` moved `horizon` frames (a float or one per stream) past their last frame,
        without a tick: (bboxes, scores, labels, None, track_ids) per stream, as __call__ returns them (sy_track_forecast; the
        tracker's state is only read).  What the reference does for every output frame between two detections."""
        if self.tracks is None:
            raise ValueError("MultiStreamDetector: forecast() needs a detector built with track=...")
        sids = list(sids)
        for sid in sids:
            self._known(sid)
        hs = [float(horizon)] * len(sids) if np.isscalar(horizon) else [float(h) for h in horizon]
        if len(hs) != len(sids):
            raise ValueError("MultiStreamDetector: %d horizons for %d streams" % (len(hs), len(sids)))
        res = []
        for t0 in range(0, len(sids), self.max_streams):
            part = sids[t0:t0 + self.max_streams]
            entries = [(self._slot_of[s], h, self._geom[s][0][1], self._geom[s][0][0]) for s, h in zip(part, hs[t0:])]
            res += self._parse_tracks(*self.tracks.forecast(entries, self._track_prm), len(part))
        return res

    def draw(self, surfaces, sids, style=None):
        """Draw the latest tick's results of the streams `sids` into `surfaces`, in place, and return them (overlay.py; the
        rendering rule: include/streamyolo_hip.h).  A target is a data.Surface (bgr / rgb / nv12 / p010) or a uint8 device tensor
        [H, W, 3] taken as BGR, of the stream's camera size, on the detector's device; it need not be the frame the tick read —
        a decoder surface still held as a reference frame must NOT be drawn on: pass `[s.clone() for s in ...]`.  With tracking
        the tracker's forecast output is drawn (camera coordinates, track ids), without it the detections (divided by the
        stream's box divisor).  style: an overlay.OverlayStyle (None: the defaults).  ONE launch on the current stream behind
        the tick, its table one non-blocking copy from pinned memory: no host read, no synchronisation, and not on the tick's
        tape.  ValueError — before anything is written — for a stream without a frame in the latest tick, a stream named twice,
        a target on another device or of another size."""
        from .overlay import OverlayRows, OverlayStyle, as_target, draw_rows
        surfaces, sids = list(surfaces), list(sids)
        if len(surfaces) != len(sids):
            raise ValueError("MultiStreamDetector: %d targets for %d stream ids" % (len(surfaces), len(sids)))
        if style is None:
            style = self._style = self._style or OverlayStyle()
        elif not isinstance(style, OverlayStyle):
            raise ValueError("MultiStreamDetector: style must be an OverlayStyle, got %r" % (style,))
        if len(set(sids)) != len(sids):
            raise ValueError("MultiStreamDetector: a stream id appears twice in one draw: %r" % (sids,))
        targets = []
        for t, sid in zip(surfaces, sids):
            self._known(sid)
            if sid not in self._row_of:
                raise ValueError("MultiStreamDetector: stream %r had no frame in the latest tick" % (sid,))
            targets.append(as_target(t, self.device if self._last is None else self._last[0].device, self._geom[sid][0],
                                     "MultiStreamDetector"))
        if not sids:
            return surfaces
        if self._overlay is None:
            self._overlay = OverlayRows(self.batch, self._last[0].device)
        self._overlay.clear()
        for t, sid in zip(targets, sids):
            self._overlay.set_row(self._row_of[sid], t, 1.0 if self.tracks is not None else self._geom[sid][2], style)
        self._overlay.upload()
        max_hw = self.max_frame_hw or self.frame_hw
        if self.tracks is not None:
            draw_rows(self._overlay, max_hw, self.tracks.out, 1, self.tracks.out_id, self.tracks.out_cnt, style)
        else:
            draw_rows(self._overlay, max_hw, self._last[0], 0, None, self._last[1], style)
        return surfaces

    def redact(self, surfaces, sids, spec=None):
        """Pixelate or fill the latest tick's results of the streams `sids` in `surfaces`, in place, and return them (redact.py;
        the rule: include/streamyolo_hip.h).  A target is what draw() takes: a data.Surface (bgr / rgb / nv12 / p010) or a uint8
        device tensor [H, W, 3] taken as BGR, of the stream's camera size, on the detector's device.  Redaction is IN PLACE: a
        decoder surface still held as a reference frame must NOT be redacted — pass `[s.clone() for s in ...]`.  With tracking
        the tracker's forecast output is redacted (camera coordinates; a track survives a missed detection, so the object stays
        hidden through a flickered frame), without it the detections (divided by the stream's box divisor).  Every list entry is
        looked at: no cap.  spec: a redact.RedactSpec (None: the defaults).  Order: redact() BEFORE draw(), so that the drawing
        lies on top of the pixelated boxes and stays legible.  ONE launch on the current stream behind the tick, its table one
        non-blocking copy from pinned memory: no host read, no synchronisation, and not on the tick's tape.  ValueError — before
        anything is written — for a stream without a frame in the latest tick, a stream named twice, a target on another
        device or of another size."""
        from .redact import RedactRows, RedactSpec, as_target, check_spec, redact_rows
        surfaces, sids = list(surfaces), list(sids)
        if len(surfaces) != len(sids):
            raise ValueError("MultiStreamDetector: %d targets for %d stream ids" % (len(surfaces), len(sids)))
        if spec is None:
            spec = self._redact_spec = self._redact_spec or RedactSpec()
        check_spec(spec, "MultiStreamDetector")
        if len(set(sids)) != len(sids):
            raise ValueError("MultiStreamDetector: a stream id appears twice in one redact: %r" % (sids,))
        targets = []
        for t, sid in zip(surfaces, sids):
            self._known(sid)
            if sid not in self._row_of:
                raise ValueError("MultiStreamDetector: stream %r had no frame in the latest tick" % (sid,))
            targets.append(as_target(t, self.device if self._last is None else self._last[0].device, self._geom[sid][0],
                                     "MultiStreamDetector"))
        if not sids:
            return surfaces
        if self._redact_rows is None:
            self._redact_rows = RedactRows(self.batch, self._last[0].device)
        self._redact_rows.clear()
        for t, sid in zip(targets, sids):
            self._redact_rows.set_row(self._row_of[sid], t, 1.0 if self.tracks is not None else self._geom[sid][2], spec)
        self._redact_rows.upload()
        max_hw = self.max_frame_hw or self.frame_hw
        if self.tracks is not None:
            redact_rows(self._redact_rows, max_hw, self.tracks.out, 1, self.tracks.out_cnt)
        else:
            redact_rows(self._redact_rows, max_hw, self._last[0], 0, self._last[1])
        return surfaces

    def crops(self, surfaces, sids, spec=None):
        """Crop the latest tick's results of the streams `sids` out of `surfaces` -> crops.Crops (images [capacity, 3, Ch, Cw],
        index, rect, count: device tensors; the rule: include/streamyolo_hip.h).  A source is what draw() takes as a target — a
        data.Surface (bgr / rgb / nv12 / p010) or a uint8 device tensor [H, W, 3] taken as BGR, of the stream's camera size, on
        the detector's device — and is only read: the decoder's own surface will do.  With tracking the tracker's forecast
        output is cropped (camera coordinates, track ids in index[:, 2]), without it the detections (divided by the stream's box
        divisor).  spec: a crops.CropSpec (None: the defaults).  Crops come with batch rows ascending and list index ascending
        within a row; index[:, 0] is the BATCH ROW and the result's row_sids[b] names the stream that row served (None: not
        asked for).  ONE C call on the current stream behind the tick (two launches), its table one non-blocking copy from
        pinned memory: no host read, no synchronisation, and not on the tick's tape.  The result's tensors are allocated once
        per spec VALUE (a CropSpec built again with the same arguments reuses them; the detector keeps those of its four most
        recently used specs) and overwritten by the next crops() with an equal spec.  ValueError — before anything is written — for a stream
        without a frame in the latest tick, a stream named twice, a source on another device or of another size."""
        from .crops import CropCache, CropRows, CropSpec, as_source, check_spec, gather_rows
        surfaces, sids = list(surfaces), list(sids)
        if len(surfaces) != len(sids):
            raise ValueError("MultiStreamDetector: %d sources for %d stream ids" % (len(surfaces), len(sids)))
        if spec is None:
            spec = self._crop_spec = self._crop_spec or CropSpec()
        check_spec(spec, "MultiStreamDetector")
        if len(set(sids)) != len(sids):
            raise ValueError("MultiStreamDetector: a stream id appears twice in one crops: %r" % (sids,))
        sources = []
        for t, sid in zip(surfaces, sids):
            self._known(sid)
            if sid not in self._row_of:
                raise ValueError("MultiStreamDetector: stream %r had no frame in the latest tick" % (sid,))
            sources.append(as_source(t, self.device if self._last is None else self._last[0].device, self._geom[sid][0],
                                     "MultiStreamDetector"))
        dev = self.device if self._last is None else self._last[0].device
        if self._crop_out is None:
            self._crop_out = CropCache()
        out = self._crop_out.get(spec, self.batch, dev)
        spec = out.spec                                          # (equal by value; the one whose device tables exist)
        row_sids = [None] * self.batch
        if not sids:
            out.count.zero_()
            out.row_sids = tuple(row_sids)
            return out
        if self._crop_rows is None:
            self._crop_rows = CropRows(self.batch, dev)
        self._crop_rows.clear()
        for t, sid in zip(sources, sids):
            row_sids[self._row_of[sid]] = sid
            self._crop_rows.set_row(self._row_of[sid], t, 1.0 if self.tracks is not None else self._geom[sid][2], spec)
        self._crop_rows.upload()
        out.row_sids = tuple(row_sids)
        if self.tracks is not None:
            return gather_rows(self._crop_rows, self.tracks.out, 1, self.tracks.out_id, self.tracks.out_cnt, spec, out)
        return gather_rows(self._crop_rows, self._last[0], 0, None, self._last[1], spec, out)

    def __call__(self, frames, sids, frame_idx=None, horizon=None):
        """n camera frames (uint8 [H, W, 3] arrays or tensors; surfaces=True: data.Surface too) and the ids of their streams -> n (bboxes, scores, labels, None)
        host tuples in the order given, each what StreamingDetector returns for that frame.  n > batch: consecutive ticks.
        Every tick ends with the device synchronised by the copy of its counts and kept rows.
        With tracking: 5-tuples (bboxes, scores, labels, None, track_ids) of the tracker's forecast output (see the class)."""
        fs, sids = self._check(frames, sids), list(sids)
        times = self._check_times(sids, frame_idx, horizon)
        res = []
        for t0 in range(0, len(sids), self.batch):
            det, cnt, n = self._tick(fs[t0:t0 + self.batch], sids[t0:t0 + self.batch], times[t0:t0 + self.batch])
            if self.tracks is not None:
                res += self._parse_tracks(self.tracks.out, self.tracks.out_id, self.tracks.out_cnt, n)
                continue
            counts = cnt[:n].cpu().numpy()
            rows = det[:n, :max(int(counts.max()), 1)].cpu().numpy()
            for b in range(n):
                d = rows[b, :int(counts[b])]
                res.append((d[:, :4] / self._geom[sids[t0 + b]][2], d[:, 4] * d[:, 5], d[:, 6].astype(np.int32), None))
        return res


def run_sequence(frames, detect, fps=30.0, det_stride=1, dynamic_schedule=False, clock=time.perf_counter, reset=None):
    """The scheduling loop of one sequence (streamyolo_det.py:138-199): real time runs at `fps`; whenever the detector is
    free it takes the LATEST frame (index floor(t * fps)), skipping it if already seen, if the stride counter says so, or
    — dynamic schedule — if more than half of that frame's interval has passed; results are stamped with their finish
    time.  `detect(frame)` returns the parsed result and must have finished its device work on return.  `clock` is
    injectable (tests drive it with a simulated clock; it is read exactly where the reference reads perf_counter).
    Returns the reference's per-sequence pickle dict (minus `results_raw`, the undecoded device tensors)."""
    duration = len(frames) / fps                     # the sequence's length in real time
    log = {"results_parsed": [], "timestamps": [], "input_fidx": [], "runtime": []}
    seen = None                                      # index of the frame looked at last
    since_det = 0                                    # fixed-stride schedule: frames since the last detection (0 = none yet)
    if reset is not None:
        reset()
    t0 = clock()
    while True:
        began = clock()
        now = began - t0
        if now >= duration:
            break
        pos = now * fps                              # fractional frame position of "now"
        latest = int(np.floor(pos))
        if latest == seen:
            continue                                 # nothing new yet: poll again
        seen = latest
        if dynamic_schedule:
            if pos - latest > 0.5:                   # too far into this frame's interval: wait for the next one
                continue
        else:
            take = since_det % det_stride == 0
            since_det = 1 if take else since_det + 1
            if not take:
                continue
        parsed = detect(frames[latest])
        ended = clock()
        finish = ended - t0
        if finish >= duration:
            break                                    # finished after the sequence ended: not recorded
        log["timestamps"].append(finish)
        log["results_parsed"].append(parsed)
        log["input_fidx"].append(latest)
        log["runtime"].append(ended - began)
    return log


def runtime_summary(runtime_all, n_total, fps=30.0):
    """streamyolo_det.py:201-229: the `time_info.pkl` dict plus print_stats' numbers (sAP/util/__init__.py:13-36) in ms."""
    r = np.asarray(runtime_all, dtype=np.float64)
    out = {"runtime_all": list(runtime_all), "n_processed": int(r.size), "n_total": int(n_total),
           "n_small_runtime": int((r < 1.0 / fps).sum())}
    if r.size > 1:
        out["stats_ms"] = {"mean": 1e3 * r.mean(), "std": 1e3 * r.std(ddof=1), "min": 1e3 * r.min(), "max": 1e3 * r.max()}
    elif r.size == 1:
        out["stats_ms"] = {"scalar": 1e3 * float(r[0])}
    return out


def ltrb2ltwh(bboxes):
    """sAP/util/bbox.py:15-21,74-76 (copying form)."""
    b = np.array(bboxes, copy=True)
    if len(b):
        if b.ndim == 1:
            b[2:] -= b[:2]
        else:
            b[:, 2:] -= b[:, :2]
    return b


def pair_with_ground_truth(results, image_ids, fps=30.0, eta=0.0):
    """streaming_eval.py:74-139 for one sequence: ground-truth frame number n (time (n - eta) / fps) is paired with the
    LAST result whose timestamp is <= that time.  `results` = run_sequence's dict, `image_ids` = the dataset ids of the
    sequence's frames in order.  Returns (coco_rows, {"in_time", "miss", "mismatch"})."""
    stamps, sources, parsed = results["timestamps"], results["input_fidx"], results["results_parsed"]
    rows = []
    stats = {"in_time": 0, "miss": 0, "mismatch": 0}
    ready = 0                                        # results finished by the current query time (monotone cursor)
    for n, image_id in enumerate(image_ids):
        query = (n - eta) / fps
        while ready < len(stamps) and stamps[ready] <= query:
            ready += 1
        if ready == 0:                               # nothing has been produced yet
            stats["miss"] += 1
            continue
        src = sources[ready - 1]
        stats["in_time"] += int(src == n)
        stats["mismatch"] += n - src
        boxes, scores, labels, masks = parsed[ready - 1][:4]
        if not len(boxes):
            continue
        ltwh = ltrb2ltwh(boxes)
        for j in range(len(boxes)):
            row = {"image_id": image_id, "bbox": ltwh[j], "score": scores[j], "category_id": labels[j]}
            if masks is not None:
                row["segmentation"] = masks[j]
            rows.append(row)
    return rows, stats


def convert_to_coco_format(outputs, info_imgs, ids, img_size, class_ids, images, skip_ids=(15060, 15061)):
    """ONEX_COCOEvaluator.convert_to_coco_format (exps/evaluators/onex_stream_evaluator.py:167-209), dataset access
    replaced by plain arguments: `class_ids` = dataset.class_ids, `images` = coco.dataset['images'] (each with 'fid').
    A detection made on frame t is scored against frame t+1 (`image_id = img_id + 1`); frames whose successor starts a
    new sequence are dropped, and so — exactly as in the reference, whose append sits inside the final `else` — are
    the detections of every sequence's first frame, and the two hard-coded ids."""
    rows = []
    for det, h, w, img_id in zip(outputs, info_imgs[0], info_imgs[1], ids):
        if det is None:
            continue
        t = int(img_id)
        if t in skip_ids or images[t + 1]["fid"] == 0 or images[t]["fid"] == 0:
            continue                                 # (reference :183-187: no row is ever emitted for these frames)
        det = det.cpu()
        r = min(img_size[0] / float(h), img_size[1] / float(w))      # undo the letterbox scale
        xywh = det[:, 0:4] / r
        xywh[:, 2:4] -= xywh[:, 0:2]                                  # yolox.utils.xyxy2xywh
        conf = det[:, 4] * det[:, 5]
        for k in range(det.shape[0]):
            rows.append({"image_id": t + 1, "category_id": class_ids[int(det[k, 6])], "bbox": xywh[k].numpy().tolist(),
                         "score": conf[k].numpy().item(), "segmentation": []})
    return rows

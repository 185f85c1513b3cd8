"""NV12 and RGB camera frames in the device input pipeline (sy_frames_u8_pack_fmt, sy_frame_src.format; csrc/input_pipeline.hip).

The contract: for any pixel format the pack entry points write, bit for bit, what the BGR path writes for the frame first
converted to uint8 [Hs, Ws, 3] BGR — per source pixel, before any decimation or bilinear tap.  So the yardstick throughout is
torch.equal against the BGR path on the converted frame; the conversion itself is stated below in int64 numpy (BT.601 limited
range in the fixed point OpenCV publishes for COLOR_YUV2BGR_NV12 — restated from published source, not pinned against a cv2
binary).  The resize bounds of the existing tests are not re-derived here: the BGR path is their subject."""
import numpy as np
import pytest
import torch

from streamyolo_amd import _lib, ops
from streamyolo_amd import streaming as S
from streamyolo_amd.data import FramePairsU8, FrameRowsU8
from streamyolo_amd.ops import View

CANVAS = (32, 64)


# ---- the yardstick -------------------------------------------------------------------------------------------------------------
def _terms(nv12):
    """uint8 [Hs*3/2, Ws] -> the three UNCLAMPED int64 values (B, G, R) [Hs, Ws, 3] of the issue's formula."""
    rows, ws = nv12.shape
    hs = rows // 3 * 2
    assert rows * 2 == hs * 3 and hs % 2 == 0 and ws % 2 == 0
    y = np.maximum(nv12[:hs].astype(np.int64) - 16, 0)
    uv = nv12[hs:].astype(np.int64).reshape(hs // 2, ws // 2, 2) - 128
    u = np.repeat(np.repeat(uv[..., 0], 2, axis=0), 2, axis=1)          # chroma of (y, x) = pair (y >> 1, x >> 1)
    v = np.repeat(np.repeat(uv[..., 1], 2, axis=0), 2, axis=1)
    b = (1220542 * y + 2116026 * u + (1 << 19)) >> 20
    g = (1220542 * y - 409993 * u - 852492 * v + (1 << 19)) >> 20
    r = (1220542 * y + 1673527 * v + (1 << 19)) >> 20
    return np.stack([b, g, r], axis=-1)


def nv12_to_bgr(nv12):
    return np.clip(_terms(np.ascontiguousarray(nv12)), 0, 255).astype(np.uint8)


def _nv12(seed, hs, ws, n=None):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, ((hs * 3 // 2, ws) if n is None else (n, hs * 3 // 2, ws))).astype(np.uint8)


def _t(a, backend):
    """numpy -> a dense device tensor (a fresh one: numpy's a[None] would arrive with stride 0 in its batch dimension)."""
    t = torch.empty(a.shape, dtype=torch.uint8)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t.to(backend)


def _pack_all(x, out_size):
    """NCHW fp32 and Focus fp32 / fp16 / bf16 of one FramePairsU8 -> list of tensors."""
    B, pair = x.cur.shape[0], x.sup is not None
    res = [x.to_nchw()]
    for dt in ("fp32", "fp16", "bf16"):
        vc = View.alloc(B, out_size[0] // 2, out_size[1] // 2, 16, dt, x.device)
        vs = View.alloc(B, out_size[0] // 2, out_size[1] // 2, 16, dt, x.device) if pair else None
        x.pack_focus(vc, vs)
        res.append(vc.buf.clone())
        if pair:
            res.append(vs.buf.clone())
    return res


def _same_all(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (what, k)


# ---- 1: the conversion itself ---------------------------------------------------------------------------------------------------
def test_nv12_conversion_is_the_published_fixed_point(backend):
    """One frame in which Y takes all 256 values (along x) against the 7 x 7 lattice of (U, V) over {0, 16, 64, 128, 192, 240,
    255} (one pair per chroma row), decimate 1, NCHW: exactly the int64 statement of the formula.  Both clamps and Y < 16 occur."""
    lat = [0, 16, 64, 128, 192, 240, 255]
    pairs = [(u, v) for u in lat for v in lat]
    hs, ws = 2 * len(pairs), 256
    nv = np.zeros((hs * 3 // 2, ws), dtype=np.uint8)
    nv[:hs] = np.arange(256, dtype=np.uint8)[None, :]
    for r, (u, v) in enumerate(pairs):
        nv[hs + r, 0::2], nv[hs + r, 1::2] = u, v
    raw = _terms(nv)
    assert (raw < 0).any() and (raw > 255).any() and (nv[:hs] < 16).any()
    assert all(set(np.unique(nv[hs:, k::2])) == set(lat) for k in (0, 1)) and len(np.unique(nv[:hs])) == 256
    want = torch.from_numpy(nv12_to_bgr(nv)).permute(2, 0, 1).float().unsqueeze(0)
    x = FramePairsU8(_t(nv[None], backend), None, (hs, ws), 1, pixel_format="nv12")
    assert tuple(x.shape) == (1, 3, hs, ws)
    assert torch.equal(x.to_nchw().cpu(), want)


# ---- 2: pack equivalence --------------------------------------------------------------------------------------------------------
# (Hs, Ws, decimate, mirror) on canvas (32, 64)
GEOMS = [(32, 64, 1, 0),
         (64, 128, 2, 0),
         (40, 72, 0, 0),
         (50, 20, 0, 0),
         (34, 70, -1, 1),
         (64, 126, 2, 0),                                        # ws = 63 is odd: a Focus pixel straddles the letterbox edge
         (32, 62, 1, 0)]


@pytest.mark.parametrize("out_size", [(32, 64), (16, 32)])
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%d_d%d" % g[:3] for g in GEOMS])
def test_pack_equals_the_bgr_path_on_the_converted_frame(backend, geom, out_size):
    """Random bytes in all planes: NV12 == the BGR path on nv12_to_bgr(frame), RGB == the BGR path on frame[..., ::-1]; NCHW fp32
    and Focus fp32 / fp16 / bf16, at the canvas size and through the canvas resize."""
    hs, ws, dec, mir = geom
    nv = _nv12(hs * 1000 + ws, hs, ws)
    bgr = nv12_to_bgr(nv)
    mirror = torch.tensor([mir], dtype=torch.uint8, device=backend) if mir else None
    want = _pack_all(FramePairsU8(_t(bgr[None], backend), None, CANVAS, dec, mirror, out_size), out_size)
    got = _pack_all(FramePairsU8(_t(nv[None], backend), None, CANVAS, dec, mirror, out_size, pixel_format="nv12"), out_size)
    _same_all(got, want, "nv12")
    rgb = np.random.RandomState(hs + ws).randint(0, 256, (1, hs, ws, 3)).astype(np.uint8)
    want = _pack_all(FramePairsU8(_t(rgb[..., ::-1], backend), None, CANVAS, dec, mirror, out_size), out_size)
    x = FramePairsU8(_t(rgb, backend), None, CANVAS, dec, mirror, out_size, pixel_format="rgb")
    _same_all(_pack_all(x, out_size), want, "rgb")
    assert not torch.equal(want[0], FramePairsU8(x.cur, None, CANVAS, dec, mirror, out_size).to_nchw())    # (the order matters)


@pytest.mark.parametrize("out_size", [(32, 64), (16, 32)])
def test_pairs_with_per_pair_mirror_flags(backend, out_size):
    """(current, support) pairs of 64 x 128 frames, decimate 2, pair 0 mirrored and pair 1 not: both outputs of every layout;
    resized() and paired_with_self() carry the format."""
    cur, sup = _nv12(11, 64, 128, 2), _nv12(12, 64, 128, 2)
    mirror = torch.tensor([1, 0], dtype=torch.uint8, device=backend)
    conv = lambda a: np.stack([nv12_to_bgr(f) for f in a])       # noqa: E731
    want = _pack_all(FramePairsU8(_t(conv(cur), backend), _t(conv(sup), backend), CANVAS, 2, mirror, out_size), out_size)
    x = FramePairsU8(_t(cur, backend), _t(sup, backend), CANVAS, 2, mirror, pixel_format="nv12")
    assert tuple(x.shape) == (2, 6) + CANVAS
    _same_all(_pack_all(x.resized(out_size), out_size), want, "nv12 pair")
    for fmt, frames in (("nv12", cur), ("rgb", conv(cur)[..., ::-1])):
        one = FramePairsU8(_t(frames, backend), None, CANVAS, 2, mirror, out_size, pixel_format=fmt)
        two = one.paired_with_self()
        assert two.pixel_format == fmt and two.sup is two.cur and tuple(two.shape) == (2, 6) + out_size
        ref = FramePairsU8(_t(conv(cur), backend), _t(conv(cur), backend), CANVAS, 2, mirror, out_size)
        assert torch.equal(two.to_nchw(), ref.to_nchw()), fmt


# ---- 3: the fast path against the generic path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(64, 128, 2), (32, 64, 1)], ids=["64x128_d2", "32x64_d1"])
def test_fast_path_equals_the_generic_path(backend, geom):
    """The same two NV12 frames (row 0 mirrored) with pitch Ws (aligned: the fast path), with pitch Ws + 2 and at a base address
    one byte into a larger buffer (both: the generic path): all equal the yardstick in every layout.  Padding bytes and the bytes
    after the last chroma row are 255, the frames' own bytes are not all 255 there: an over-read would show."""
    hs, ws, dec = geom
    rows = hs * 3 // 2
    nv = _nv12(31 + dec, hs, ws, 2)
    mirror = torch.tensor([1, 0], dtype=torch.uint8, device=backend)
    bgr = np.stack([nv12_to_bgr(f) for f in nv])
    want = _pack_all(FramePairsU8(_t(bgr, backend), None, CANVAS, dec, mirror), CANVAS)

    def given(pitch, offset):
        img = rows * pitch + 64                                  # bytes between images: the tail stays 255
        flat = torch.full((offset + 2 * img,), 255, dtype=torch.uint8, device=backend)
        cur = flat[offset:].as_strided((2, rows, ws), (img, pitch, 1))
        cur.copy_(_t(nv, backend))
        assert cur.data_ptr() == flat.data_ptr() + offset and (cur.stride(1), cur.stride(2)) == (pitch, 1)
        return FramePairsU8(cur, None, CANVAS, dec, mirror, pixel_format="nv12")
    for pitch, offset in ((ws, 0), (ws + 2, 0), (ws, 1)):
        x = given(pitch, offset)
        assert x.cur.data_ptr() % 4 == offset
        _same_all(_pack_all(x, CANVAS), want, (pitch, offset))


# ---- 4: rows --------------------------------------------------------------------------------------------------------------------
# (format, Hs, Ws, decimate, mirror) of rows 0..4; row 5 has no frame
R_ROWS = [("bgr", 40, 72, 0, 0),
          ("rgb", 50, 20, 0, 0),
          ("nv12", 64, 128, 2, 0),
          ("nv12", 32, 64, 1, 1),
          ("nv12", 34, 70, -1, 0)]
R_B = len(R_ROWS) + 1


@pytest.mark.parametrize("out_size", [(32, 64), (16, 32)])
def test_rows_of_different_formats_share_one_launch(backend, out_size):
    """One sy_frames_u8_pack_rows launch over BGR, RGB and NV12 cameras of different sizes and an empty row: every row == that
    frame alone through FramePairsU8 of its format (NCHW fp32, Focus fp32 / fp16 / bf16).  Refilled in a permuted order the
    launch has the identical C-ABI arguments (all but the freshly allocated output) and the outputs are permuted: the format
    is data."""
    rng = np.random.RandomState(5)
    frames = [_nv12(50 + k, hs, ws) if fmt == "nv12" else rng.randint(0, 256, (hs, ws, 3)).astype(np.uint8)
              for k, (fmt, hs, ws, _, _) in enumerate(R_ROWS)]
    rows = FrameRowsU8(R_B, (64, 128), CANVAS, backend, out_size=out_size)

    def fill(order):
        for b, k in enumerate(order):
            if k is None:
                rows.set_row(b, None)
            else:
                fmt, _, _, dec, mir = R_ROWS[k]
                rows.set_row(b, frames[k], mirror=bool(mir), decimate=dec, divisor=1.0, pixel_format=fmt)
        rows.upload()

    def alone(k):
        fmt, _, _, dec, mir = R_ROWS[k]
        x = FramePairsU8(_t(frames[k][None], backend), None, CANVAS, dec, torch.tensor([mir], dtype=torch.uint8, device=backend),
                         out_size, pixel_format=fmt)
        return _pack_all(x, out_size)

    def launch():
        with _lib.record() as calls:
            nchw = rows.to_nchw()
        res = [nchw]
        for dt in ("fp32", "fp16", "bf16"):
            v = View.alloc(R_B, out_size[0] // 2, out_size[1] // 2, 16, dt, backend)
            rows.pack_focus(v)
            res.append(v.buf.reshape(R_B, -1, 16).clone())
        return calls, res
    order = [0, 1, 2, 3, 4, None]
    fill(order)
    assert [int(f) for f in rows._rows["format"]] == [0, 1, 2, 2, 2, 0]
    first_calls, got = launch()
    singles = [alone(k) for k in range(len(R_ROWS))]
    for b, k in enumerate(order):
        for lay in range(4):
            if k is None:
                want = torch.full_like(got[lay][b], 114.0)
                if lay:
                    want[..., 12:] = 0
                assert torch.equal(got[lay][b], want), ("empty", lay)
            else:
                assert torch.equal(got[lay][b].reshape(-1), singles[k][lay].reshape(-1)), (R_ROWS[k], lay)
    perm = [3, None, 4, 0, 2, 1]
    fill(perm)
    second_calls, got2 = launch()
    (_, a1, name1), (_, a2, name2) = first_calls[0], second_calls[0]
    assert len(first_calls) == len(second_calls) == 1 and name1 == name2 == "sy_frames_u8_pack_rows"
    assert a1[:7] + a1[8:] == a2[:7] + a2[8:]
    for b2, k in enumerate(perm):
        for lay in range(4):
            assert torch.equal(got2[lay][b2], got[lay][order.index(k)]), (b2, k, lay)


# ---- 5: rejections --------------------------------------------------------------------------------------------------------------
def test_entry_point_status_codes(backend):
    """sy_frames_u8_pack_fmt: SY_ERR_UNSUPPORTED (3) for an odd NV12 size, SY_ERR_ARG (1) for an unknown format, a pitch below Ws
    and an image stride below 1.5 Hs rows; only the good calls write."""
    lib = _lib.lib()
    buf = torch.full((2, 24, 16), 16, dtype=torch.uint8, device=backend)       # two 16 x 16 NV12 images: Y = 16 (black)
    buf[:, 16:] = 128
    out = torch.zeros((2, 3, 16, 16), dtype=torch.float32, device=backend)
    p, o, st = buf.data_ptr(), out.data_ptr(), ops.stream_of(out)

    def call(Hs=16, Ws=16, image_stride=24 * 16, row_stride=16, fmt=_lib.PIX_NV12, H=16, W=16):
        return lib.sy_frames_u8_pack_fmt(p, None, 2, Hs, Ws, image_stride, row_stride, 1, None, H, W, H, W, ops.FRAMES_NCHW, o, None,
                                         _lib.DT_F32, fmt, st)
    assert call(fmt=3) == 1 and call(fmt=-1) == 1
    assert call(Hs=15, H=15) == 3 and call(Ws=15, W=15) == 3
    assert call(image_stride=16 * 16) == 1 and call(image_stride=24 * 16 - 1) == 1       # enough for BGR's Hs rows only
    assert call(row_stride=15) == 1
    assert torch.equal(out.cpu(), torch.zeros(2, 3, 16, 16))
    assert call() == 0
    assert torch.equal(out.cpu(), torch.zeros(2, 3, 16, 16))                   # (written: limited-range black is 0, 0, 0)
    out.fill_(7.0)
    assert call(Hs=8, Ws=5, image_stride=24 * 16, row_stride=16, fmt=_lib.PIX_RGB, H=8, W=5) == 0     # [8, 5, 3] in 16-byte rows
    assert call(Hs=8, Ws=6, row_stride=16, fmt=_lib.PIX_RGB, H=8, W=6) == 1                            # 18 bytes do not fit
    with pytest.raises(ValueError):
        ops.frames_u8_pack(buf, None, (16, 16), (16, 16), out, pixel_format="yuyv")
    with pytest.raises(ValueError):
        FramePairsU8(buf[:, :, :15], None, (16, 16), pixel_format="nv12")


def test_impossible_descriptor_rows_are_the_plain_canvas(backend):
    """A descriptor with an unknown format, an odd NV12 size or a pitch below what its format needs is written as all-114 and
    never read through (its pointer is not a valid address); the good row beside them is written."""
    rows = FrameRowsU8(5, (16, 16), (16, 16), backend)
    nv = _nv12(3, 16, 16)
    rows.set_row(0, nv, pixel_format="nv12")
    good = rows._rows[0].copy()
    bad = rows.arena.data_ptr()                                  # (row 0's pixels: a descriptor read through would not give 114)
    rows._rows[1] = (bad, 16, 16, 48, 1, 0, 3)                   # unknown format
    rows._rows[2] = (bad, 16, 15, 16, 1, 0, _lib.PIX_NV12)       # odd NV12 width
    rows._rows[3] = (bad, 15, 16, 16, 1, 0, _lib.PIX_NV12)       # odd NV12 height
    rows._rows[4] = (bad, 16, 16, 15, 1, 0, _lib.PIX_NV12)       # pitch below Ws
    rows.upload()
    out = rows.to_nchw().cpu()
    assert tuple(good)[1:] == (16, 16, 16, 1, 0, _lib.PIX_NV12)
    assert torch.equal(out[0], torch.from_numpy(nv12_to_bgr(nv)).permute(2, 0, 1).float())
    assert torch.equal(out[1:], torch.full((4, 3, 16, 16), 114.0))
    v = View.alloc(5, 8, 8, 16, "fp16", backend)
    rows.pack_focus(v)
    f = v.buf.reshape(5, 64, 16).cpu().float()
    assert torch.equal(f[1:, :, :12], torch.full((4, 64, 12), 114.0)) and torch.equal(f[..., 12:], torch.zeros(5, 64, 4))


def _models(backend, dtype="fp32"):
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    cfg = O.OracleConfig.named("nano")
    sd = synth_state_dict(O.param_shapes(cfg), seed=0, bn_stats=load_bn_stats("nano"))
    model = sy.build_model("nano"); model.load_state_dict(sd, strict=True)
    return model


HW, D_CANVAS, OTHER = (128, 192), (64, 96), (90, 150)            # tests/test_multistream_mixed.py's sizes


def test_python_layer_rejects_before_anything_is_written(backend):
    """set_row: ValueError for an NV12 frame of a bad shape, an odd width, a size above max_frame_hw and an unknown format, the
    table, the divisors and the arena untouched.  open: ValueError for an unknown format, an odd NV12 size and — uniform mode —
    a format that is not the detector's, the stream bookkeeping untouched."""
    rows = FrameRowsU8(2, (16, 16), (16, 16), backend)
    rows.set_row(0, _nv12(1, 16, 16), pixel_format="nv12")
    rows.set_row(1, np.full((16, 16, 3), 9, np.uint8), pixel_format="rgb")
    table, div, arena = rows._rows.copy(), rows._div.copy(), rows.arena.clone()
    for frame, fmt in ((np.zeros((16, 16, 3), np.uint8), "nv12"),            # not [Hs*3/2, Ws]
                       (np.zeros((25, 16), np.uint8), "nv12"),               # rows not a multiple of 3
                       (np.zeros((24, 15), np.uint8), "nv12"),               # odd width
                       (np.zeros((27, 16), np.uint8), "nv12"),               # 18 x 16: above max_frame_hw
                       (np.zeros((24, 16), np.float32), "nv12"),
                       (np.zeros((24, 16), np.uint8), "rgb"),                # not [Hs, Ws, 3]
                       (np.zeros((16, 16, 3), np.uint8), "i420")):
        with pytest.raises(ValueError):
            rows.set_row(0, frame, pixel_format=fmt)
    assert np.array_equal(rows._rows, table) and np.array_equal(rows._div, div) and torch.equal(rows.arena, arena)

    model = _models(backend)
    with pytest.raises(ValueError):
        S.MultiStreamDetector(model, (127, 192), max_streams=2, batch=2, dtype="fp32", device=backend, pixel_format="nv12")
    with pytest.raises(ValueError):
        S.StreamingDetector(model, HW, dtype="fp32", device=backend, pixel_format="yuv")
    uniform = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend, pixel_format="nv12")
    assert tuple(uniform._stage.shape) == (2, 192, 192) and uniform._in.pixel_format == "nv12"
    with pytest.raises(ValueError):
        uniform.open(pixel_format="bgr")
    assert uniform.open(pixel_format="nv12") == 0 and uniform.open() == 1 and uniform._free == []
    mixed = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend, max_frame_hw=HW)
    a = mixed.open(frame_hw=OTHER, pixel_format="nv12")
    state = (list(mixed._free), mixed._next_id, dict(mixed._slot_of), dict(mixed._first), dict(mixed._geom), dict(mixed._fmt))
    with pytest.raises(ValueError):
        mixed.open(frame_hw=(91, 150), pixel_format="nv12")
    with pytest.raises(ValueError):
        mixed.open(frame_hw=(90, 149), pixel_format="nv12")
    with pytest.raises(ValueError):
        mixed.open(frame_hw=OTHER, pixel_format="nv21")
    assert state == (mixed._free, mixed._next_id, mixed._slot_of, mixed._first, mixed._geom, mixed._fmt)
    assert mixed.open(frame_hw=(91, 149), pixel_format="rgb") == a + 1           # (odd sizes are fine outside NV12)
    with pytest.raises(ValueError):
        mixed._check([np.zeros(OTHER + (3,), np.uint8)], [a])                    # a BGR-shaped frame on the NV12 stream
    assert len(mixed._check([np.zeros((135, 150), np.uint8)], [a])) == 1


# ---- 6: the tape key ------------------------------------------------------------------------------------------------------------
def test_tape_is_keyed_by_the_pixel_format(backend):
    """One plan, one staging buffer: run_stream_taped with a BGR FramePairsU8, then with an RGB one over the same bytes (in
    uniform mode the format is a scalar kernel argument held by the tape: a replay would silently use the recorded one).  Each
    equals the untaped run_stream of its own input, the two differ, and the tape was recorded anew."""
    model = _models(backend).to(backend).eval().set_compute_dtype("fp32")
    rng = np.random.RandomState(9)
    frame = rng.randint(0, 256, (1, 64, 128, 3)).astype(np.uint8)
    frame[..., 0] //= 4                                          # B and R far apart: the channel order matters
    stage = _t(frame, backend)
    x_bgr = FramePairsU8(stage, None, CANVAS, 2)
    x_rgb = FramePairsU8(stage, None, CANVAS, 2, pixel_format="rgb")
    assert x_bgr.cur.data_ptr() == x_rgb.cur.data_ptr()
    plan = model._plans.inference(model.backbone, model.head, "on_pipe", x_bgr, owner=model)
    with torch.no_grad():
        want = {}
        for x in (x_bgr, x_rgb):
            plan.run_stream(x, first=True)                       # the same frame every time: steady state at once
            want[x.pixel_format] = plan.run_stream(x).clone()
        assert not torch.equal(want["bgr"], want["rgb"])
        plan.run_stream(x_bgr, first=True)
        assert torch.equal(plan.run_stream_taped(x_bgr), want["bgr"])            # records
        tape = plan._stream_tape[2]
        plan.out.zero_()
        assert torch.equal(plan.run_stream_taped(x_bgr), want["bgr"]) and plan._stream_tape[2] is tape      # replays
        plan.run_stream(x_rgb, first=True)
        plan.out.zero_()
        assert torch.equal(plan.run_stream_taped(x_rgb), want["rgb"]) and plan._stream_tape[2] is not tape
        tape = plan._stream_tape[2]
        plan.out.zero_()
        assert torch.equal(plan.run_stream_taped(x_rgb), want["rgb"]) and plan._stream_tape[2] is tape


# ---- 7: the detectors -----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] is None


def test_streaming_detector_on_nv12_frames(backend):
    """StreamingDetector(pixel_format="nv12") over four frames with a reset == the BGR detector on the converted frames, bit for
    bit; the default detector's recorded launches start with the sy_frames_u8_pack call it always made."""
    model = _models(backend)
    nv = [_nv12(70 + t, *HW) for t in range(4)]
    det = S.StreamingDetector(model, HW, dtype="fp32", device=backend, pixel_format="nv12")
    ref = S.StreamingDetector(model, HW, dtype="fp32", device=backend)
    assert tuple(det._slot.shape) == (1, 192, 192) and tuple(ref._slot.shape) == (1,) + HW + (3,) and det.decimate == 2
    got, want = [], []
    for d, frames, res in ((det, nv, got), (ref, [nv12_to_bgr(f) for f in nv], want)):
        d.warm_up(2)
        for t in range(4):
            if t == 2:
                d.reset()
            res.append(d(frames[t]))
    assert sum(len(r[0]) for r in want) > 0
    for t in range(4):
        assert _same(got[t], want[t]), t
    for d, name, n_args in ((ref, "sy_frames_u8_pack", 17), (det, "sy_frames_u8_pack_fmt", 18)):
        with _lib.record() as calls, torch.no_grad():
            d.plan.run_stream(d._in)
        names = [c[2] for c in calls]
        assert names[0] == name and names.count(name) == 1 and len(calls[0][1]) == n_args
        assert ("sy_frames_u8_pack_fmt" in names) == (d is det)
    a = calls[0][1]                                              # the NV12 launch: one pitch of Ws bytes, 1.5 Hs rows per image
    assert a[:8] == (det._slot.data_ptr(), None, 1, 128, 192, 192 * 192, 192, 2) and a[17] == _lib.PIX_NV12


def test_default_detector_issues_the_launch_it_always_did(backend):
    """No pixel_format anywhere: the uniform MultiStreamDetector's tick starts with sy_frames_u8_pack and its seventeen arguments
    (no format among them) — the BGR launch, argument for argument."""
    model = _models(backend)
    det = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend)
    det.warm_up(2)
    assert det.pixel_format == "bgr" and type(det._in) is FramePairsU8 and tuple(det._stage.shape) == (2,) + HW + (3,)
    with _lib.record() as calls, torch.no_grad():
        det.plan.run_stream_slots(det._in, det.state)
    names = [c[2] for c in calls]
    assert names[0] == "sy_frames_u8_pack" and "sy_frames_u8_pack_fmt" not in names and "sy_frames_u8_pack_rows" not in names
    st = det._stage
    assert calls[0][1] == (st.data_ptr(), None, 2, HW[0], HW[1], st.stride(0), st.stride(1), 2, None, D_CANVAS[0], D_CANVAS[1],
                           D_CANVAS[0], D_CANVAS[1], ops.FRAMES_FOCUS, det.plan.f0.ptr(), None, det.plan.f0.dtype)


def test_mixed_detector_with_streams_of_three_formats(backend):
    """A BGR, an RGB and an NV12 stream of three sizes interleaved over ticks with an absent stream and a reset == a BGR-only
    mixed detector fed the converted frames in the same schedule, bit for bit; every tick after warm_up replays the one tape
    recorded there."""
    model = _models(backend)
    fmts, sizes = ["bgr", "rgb", "nv12"], [D_CANVAS, OTHER, HW]
    det = S.MultiStreamDetector(model, HW, max_streams=3, batch=3, dtype="fp32", device=backend, max_frame_hw=HW)
    ref = S.MultiStreamDetector(model, HW, max_streams=3, batch=3, dtype="fp32", device=backend, max_frame_hw=HW)
    det.warm_up(2); ref.warm_up(2)
    tape, rtape = det.plan._slots_tape[2], ref.plan._slots_tape[2]
    n_launch = tape.size()
    assert rtape.size() == n_launch
    sid = [det.open(frame_hw=hw, pixel_format=f) for hw, f in zip(sizes, fmts)]
    rid = [ref.open(frame_hw=hw) for hw in sizes]
    assert [det._fmt[s][0] for s in sid] == fmts and det._fmt[sid[2]][1] == (192, 192)
    seed = [300]

    def frame(i):
        """-> (what stream i's camera delivers, the same picture as BGR)"""
        seed[0] += 1
        if fmts[i] == "nv12":
            f = _nv12(seed[0], *sizes[i])
            return f, nv12_to_bgr(f)
        f = np.random.RandomState(seed[0]).randint(0, 256, sizes[i] + (3,)).astype(np.uint8)
        return (f, f) if fmts[i] == "bgr" else (f, np.ascontiguousarray(f[..., ::-1]))

    def tick(order):
        fs = [frame(i) for i in order]
        got = det([f[0] for f in fs], [sid[i] for i in order])
        want = ref([f[1] for f in fs], [rid[i] for i in order])
        assert len(got) == len(order)
        for b in range(len(order)):
            assert _same(got[b], want[b]), (seed[0], order, b)
        assert det.plan._slots_tape[2] is tape and tape.size() == n_launch
        return got
    tick([0, 1, 2])
    tick([2, 0])                                                 # stream 1 absent, the others in other rows
    tick([1, 2])
    det.reset(sid[2]); ref.reset(rid[2])                         # a new sequence on the NV12 stream
    tick([2, 1, 0])
    got = tick([1, 0, 2])
    assert sum(len(r[0]) for r in got) > 0
    assert [int(f) for f in det._in._rows["format"]] == [_lib.PIX_RGB, _lib.PIX_BGR, _lib.PIX_NV12]
    with _lib.record() as calls, torch.no_grad():
        det.plan.run_stream_slots(det._in, det.state)
    names = [c[2] for c in calls]
    assert names[0] == "sy_frames_u8_pack_rows" and names.count("sy_frames_u8_pack_rows") == 1
    assert "sy_frames_u8_pack" not in names and "sy_frames_u8_pack_fmt" not in names

"""sy_crop_gather (csrc/crop.hip) on hand-made box lists, on the SIMT emulator and on the MI355X.

The yardstick is `restate` below: the eight points of the rule as include/streamyolo_hip.h states it, written in plain numpy over
whole crops — a loop over batch rows and list entries that knows nothing of plans, tiles or column tables.  YUV sources are first
converted to a BGR frame by tests/test_pixel_formats.py's nv12_to_bgr (P010: on the high bytes), then the BGR rule applies.  The
comparison is np.array_equal on the ENTIRE out, out_index, out_rect and out_count buffers (as bytes), which are pre-filled with a
pseudo-random pattern: slots at or past out_count[0] are proven unwritten.  Every plane is backed by the exact minimum allocation
— (rows - 1) * pitch + the row's bytes — so nothing behind a surface's last payload byte can be read unnoticed where the memory
ends there.

No tolerance: the rule is integer arithmetic behind one float division and one floor.  To make that a fair demand of fp32 every
case asserts on ITS OWN INPUTS, in float64, that each c / divisor + 0.5 the launch looks at is at least 1e-3 away from an integer
and each score 1e-3 away from min_score.  Boxes are integers under the divisors 1 and 0.5; rows with the divisor 0.3 get
coordinates constructed to land a quarter pixel inside their cell."""
import ctypes as C

import numpy as np
import pytest
import torch

from streamyolo_amd import _lib, ops
from streamyolo_amd.crops import _CROP_DTYPE
from test_overlay_kernel import _round_px
from test_pixel_formats import nv12_to_bgr

MARGIN = 1e-3
BGR, RGB, NV12, P010 = _lib.PIX_BGR, _lib.PIX_RGB, _lib.PIX_NV12, _lib.PIX_P010
KEEP, RGB_OUT = _lib.CROP_KEEP_ASPECT, _lib.CROP_RGB_OUT
MAX_SIDE = _lib.CROP_MAX_SIDE
MIN_SCORE = 0.3
ALL = (0xFFFFFFFF,) * 4
SIZES = [(8, 8), (16, 24), (32, 8)]                                  # Ch x Cw
DTYPES = {"u8": torch.uint8, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NP_DTYPE = {"u8": np.uint8, "f32": np.float32, "f16": np.float16, "bf16": np.uint16}      # (bf16: its bits)
MEAN = np.array([103.53, 116.28, 123.675], dtype=np.float32)
SCALE = (np.float32(1.0) / np.array([57.375, 57.12, 58.395], dtype=np.float32)).astype(np.float32)


# ---- the rule, restated from the header --------------------------------------------------------------------------------
def possible(row):
    """Rule 8: a descriptor a surface can have."""
    hs, ws, fmt = row["hs"], row["ws"], row["fmt"]
    if row["p0"] is None or hs <= 0 or ws <= 0 or fmt not in (BGR, RGB, NV12, P010):
        return False
    yuv = fmt in (NV12, P010)
    row_bytes = ws * (1 if fmt == NV12 else 2 if fmt == P010 else 3)
    cpitch = row["cpitch"] if row["cpitch"] != 0 else row["pitch"]
    return not (row["pitch"] < row_bytes or (yuv and (hs % 2 or ws % 2 or row["cpitch"] < 0 or cpitch < row_bytes)))


def frame_of(row, bufs):
    """The row's surface as a BGR frame uint8 [hs, ws, 3], read from the backing buffers payload byte by payload byte."""
    hs, ws, fmt, pitch = row["hs"], row["ws"], row["fmt"], row["pitch"]
    b0, o0 = row["p0"]
    if fmt in (BGR, RGB):
        px = np.stack([bufs[b0][o0 + y * pitch:o0 + y * pitch + 3 * ws] for y in range(hs)]).reshape(hs, ws, 3)
        return px if fmt == BGR else px[:, :, ::-1]
    step = 2 if fmt == P010 else 1                                   # P010: the high byte of every little-endian word
    b1, o1 = row["p1"] if row["p1"] is not None else (b0, o0 + pitch * hs)
    cpitch = row["cpitch"] if row["cpitch"] != 0 else pitch
    luma = [bufs[b0][o0 + y * pitch + step - 1:o0 + y * pitch + step * ws:step] for y in range(hs)]
    chroma = [bufs[b1][o1 + y * cpitch + step - 1:o1 + y * cpitch + step * ws:step] for y in range(hs // 2)]
    return nv12_to_bgr(np.stack(luma + chroma))


def rectangle(row, r, layout, ch, cw, flags):
    """Rules 1 to 3 for one list entry -> (X1, Y1, X2, Y2, class) or None (skipped).  Python integers: nothing overflows."""
    score = np.float32(r[4]) * np.float32(r[5]) if layout == 0 else np.float32(r[4])
    cls_f = r[6] if layout == 0 else r[5]
    px = [_round_px(r[i], row["divisor"]) for i in range(4)]
    if any(p is None for p in px) or not score >= np.float32(row["min_score"]):
        return None
    if not (cls_f >= 0 and cls_f < 128):                             # (NaN fails both)
        return None
    cls = int(cls_f)
    if not (row["mask"][cls >> 5] >> (cls & 31)) & 1:
        return None
    x1, y1, x2, y2 = px[0], px[1], px[2] - 1, px[3] - 1
    if x2 < x1 or y2 < y1 or x2 < 0 or x1 >= row["ws"] or y2 < 0 or y1 >= row["hs"]:
        return None
    q = min(max(row["pad_q8"], 0), 256)
    w, h = x2 - x1 + 1, y2 - y1 + 1
    px_, py_ = (w * q + 128) >> 8, (h * q + 128) >> 8
    x1, x2, y1, y2 = x1 - px_, x2 + px_, y1 - py_, y2 + py_
    w, h = x2 - x1 + 1, y2 - y1 + 1
    if flags & KEEP:
        if w * ch < h * cw:
            w2 = -(-(h * cw) // ch)
            x1 -= (w2 - w) >> 1
            x2, w = x1 + w2 - 1, w2
        elif w * ch > h * cw:
            h2 = -(-(w * ch) // cw)
            y1 -= (h2 - h) >> 1
            y2, h = y1 + h2 - 1, h2
    if w > MAX_SIDE or h > MAX_SIDE:
        return None
    return x1, y1, x2, y2, cls


def axis(c, w):
    """Rule 4 on one axis: (first tap, second tap, weight) per output index, taps relative to the rectangle."""
    j = np.arange(c, dtype=np.int64)
    n, d = (2 * j + 1) * w - c, 2 * c
    x0 = n // d                                                      # (numpy's // floors)
    f = n - x0 * d
    return np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), (256 * f + c) // d


def taps(frame, fill, ys, xs):
    """Rule 5: (B, G, R) int64 [len(ys), len(xs), 3] of the frame's pixels at rows ys x columns xs, `fill` outside the frame."""
    hs, ws = frame.shape[:2]
    out = np.empty((len(ys), len(xs), 3), dtype=np.int64)
    out[:] = np.asarray(fill[:3], dtype=np.int64)
    inside = ((ys >= 0) & (ys < hs))[:, None] & ((xs >= 0) & (xs < ws))[None, :]
    got = frame[np.clip(ys, 0, hs - 1)][:, np.clip(xs, 0, ws - 1)].astype(np.int64)
    out[inside] = got[inside]
    return out


def sample(frame, fill, rect, ch, cw):
    """Rules 4 and 5 for one rectangle -> int64 [ch, cw, 3] in (B, G, R)."""
    x1, y1, x2, y2 = rect
    xa, xb, wx = axis(cw, x2 - x1 + 1)
    ya, yb, wy = axis(ch, y2 - y1 + 1)
    wx, wy = wx[None, :, None], wy[:, None, None]
    v00, v01 = taps(frame, fill, y1 + ya, x1 + xa), taps(frame, fill, y1 + ya, x1 + xb)
    v10, v11 = taps(frame, fill, y1 + yb, x1 + xa), taps(frame, fill, y1 + yb, x1 + xb)
    return ((256 - wx) * (256 - wy) * v00 + wx * (256 - wy) * v01 + (256 - wx) * wy * v10 + wx * wy * v11 + 32768) >> 16


def bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # round to nearest even (finite values)


def restate(rows, frames, boxes, layout, ids, cnt, max_list, flags, kind, mean, scale, out, out_index, out_rect, out_count):
    """The rule for one call, into numpy copies of the four output buffers (out [capacity, 3, ch, cw] in NP_DTYPE[kind])."""
    capacity, _, ch, cw = out.shape
    total = 0
    for b, row in enumerate(rows):
        if not possible(row):
            continue
        kept = 0
        for k in range(min(max(int(cnt[b]), 0), max_list, 256)):
            got = rectangle(row, boxes[b, k], layout, ch, cw, flags)
            if got is None or (row["max_crops"] > 0 and kept >= row["max_crops"]):
                continue
            kept += 1
            slot, total = total, total + 1
            if slot >= capacity:
                continue
            v = sample(frames[b], row["fill"], got[:4], ch, cw)      # [ch, cw, 3] (B, G, R)
            planes = np.moveaxis(v[:, :, ::-1] if flags & RGB_OUT else v, 2, 0)
            if kind == "u8":
                out[slot] = planes
            else:
                m = np.zeros(3, np.float32) if mean is None else mean
                s = np.ones(3, np.float32) if scale is None else scale
                f = (planes.astype(np.float32) - m[:, None, None]) * s[:, None, None]
                assert f.dtype == np.float32
                out[slot] = bf16_bits(f) if kind == "bf16" else f.astype(NP_DTYPE[kind])
            out_index[slot] = (b, k, -1 if ids is None else ids[b, k], got[4])
            out_rect[slot] = got[:4]
    out_count[:] = (min(total, capacity), total)


def assert_fair(rows, boxes, layout, cnt, max_list):
    """The condition on a case's OWN INPUTS under which fp32 must reproduce the rule exactly (float64)."""
    for b, row in enumerate(rows):
        for r in boxes[b, :min(max(int(cnt[b]), 0), max_list, 256)]:
            for c in r[:4]:
                if np.isfinite(c):
                    v = np.float64(np.float32(c)) / np.float64(np.float32(row["divisor"])) + 0.5
                    assert abs(v - np.round(v)) >= MARGIN, (b, c, v)
            sc = np.float64(np.float32(r[4])) * np.float64(np.float32(r[5])) if layout == 0 else np.float64(np.float32(r[4]))
            if np.isfinite(sc):
                assert abs(sc - np.float64(np.float32(row["min_score"]))) >= MARGIN, (b, sc)


# ---- surfaces and lists ----------------------------------------------------------------------------------------------
def surface(fmt, hs, ws, pitch, first, cpitch=0, detached=False, luma_rows=None, **kw):
    """A table row over backing buffers first, first + 1 -> (row, sizes): every allocation is the exact minimum."""
    step = {BGR: 3, RGB: 3, NV12: 1, P010: 2}[fmt]
    row = dict(fmt=fmt, hs=hs, ws=ws, pitch=pitch, cpitch=cpitch, p0=(first, 0), p1=None, divisor=1.0, min_score=MIN_SCORE,
               max_crops=0, pad_q8=0, fill=(114, 114, 114, 0), mask=ALL)
    row.update(kw)
    if fmt in (BGR, RGB):
        return row, [(hs - 1) * pitch + step * ws]
    cp = cpitch or pitch
    if detached:
        row["p1"] = (first + 1, 0)
        return row, [(hs - 1) * pitch + step * ws, (hs // 2 - 1) * cp + step * ws]
    lr = luma_rows or hs
    if lr != hs:
        row["p1"] = (first, lr * pitch)
    return row, [lr * pitch + (hs // 2 - 1) * cp + step * ws]


def make_rows():
    """The four surfaces of the issue in one launch, and a row without a surface.  -> (rows, buffer sizes)."""
    rows, sizes = [], []
    for fmt, hs, ws, pitch, kw in ((BGR, 48, 64, 192, dict(divisor=1.0, pad_q8=0, fill=(10, 200, 90, 0))),
                                   (RGB, 50, 70, 3 * 70 + 14, dict(divisor=0.5, pad_q8=26, fill=(1, 2, 3, 0))),
                                   (NV12, 48, 64, 72, dict(divisor=0.3, pad_q8=256, cpitch=80, detached=True)),
                                   (P010, 32, 48, 2 * 48 + 4, dict(divisor=1.0, pad_q8=26, fill=(255, 0, 128, 0)))):
        row, sz = surface(fmt, hs, ws, pitch, len(sizes), **kw)
        rows.append(row)
        sizes += sz
    rows.append(dict(rows[0], p0=None))
    # the NV12 luma plane has 56 rows allocated (the chroma plane is detached, with its own pitch)
    sizes[2] = 55 * 72 + 64
    return rows, sizes


def pixel_boxes(hs, ws, ch, cw):
    """Sixteen entries in SURFACE pixels, (x1, y1, x2, y2) covering [x1, x2) x [y1, y2).  -> list of (box, class, id)."""
    return [
        ((4, 6, 20, 30), 1, 3),                                      # 0 tall: grows in x under keep-aspect
        ((10, 8, 10 + cw, 8 + ch), 0, 17),                           # 1 exactly the crop's size
        ((-6, 10, 6, 22), 2, 5),                                     # 2 half outside on the left: the fill colour
        ((ws - 5, hs - 7, ws + 9, hs + 5), 127, 123456),             # 3 crosses the bottom right corner; the last class id
        ((ws + 3, 4, ws + 12, 12), 0, 6),                            # 4 wholly outside: skipped
        ((30, 8, 22, 20), 1, 7),                                     # 5 x2 < x1: skipped
        ((np.nan, 8, 28, 24), 1, 8),                                 # 6 a NaN coordinate: skipped
        ((7, 9, 8, 10), 3, 9),                                       # 7 one pixel
        ((2, 20, 41, 27), 0, 10),                                    # 8 wide, odd sides: grows in y under keep-aspect
        ((12, 12, 30, 30), 5, 11),                                   # 9 a class the row's mask may leave out
        ((8, 4, 40, 30), 0, 12),                                     # 10 plainly visible, but its score is below min_score
        ((3, 3, 12, 18), np.nan, 13),                                # 11 a NaN class: skipped
        ((5, 5, np.inf, 12), 1, 14),                                 # 12 an infinite coordinate: skipped
        ((5, 5, 16, 12), 128, 15),                                   # 13 a class past the mask's 128 bits: skipped
        ((5, 5, 16, 12), -1, 16),                                    # 14 a negative class: skipped
        ((ws - 9, 1, ws, 14), 4, -7),                                # 15 ends on the last column; a negative id
    ]


SCORES = [0.957 - 0.0331 * k for k in range(16)]
SCORES[10] = 0.2137


def make_lists(rows, layout, ch, cw, max_list=20):
    """boxes [B, max_list, 7 | 6] fp32, ids [B, max_list] int32, cnt [B] for the rows' own box sets (entries beyond: zeros)."""
    B = len(rows)
    boxes = np.zeros((B, max_list, 7 if layout == 0 else 6), dtype=np.float32)
    ids = np.zeros((B, max_list), dtype=np.int32)
    for b, row in enumerate(rows):
        for k, (px, cls, ident) in enumerate(pixel_boxes(row["hs"], row["ws"], ch, cw)):
            d = row["divisor"]
            if d in (1.0, 0.5):
                c = [p * d for p in px]                              # exact in fp32: c / d + 0.5 is p + 0.5
            else:                                                    # constructed: c / d + 0.5 lands a quarter pixel above p + 0.5
                c = [np.float32(d * (p + 0.25)) for p in px]
            boxes[b, k, :4] = c
            boxes[b, k, 4:] = (0.9, SCORES[k] / 0.9, cls) if layout == 0 else (SCORES[k], cls)
            ids[b, k] = ident
    return boxes, ids, np.full(B, 16, dtype=np.int32)


def table_of(rows, tensors):
    t = np.zeros(len(rows), dtype=_CROP_DTYPE)
    for b, r in enumerate(rows):
        p0 = 0 if r["p0"] is None else tensors[r["p0"][0]].data_ptr() + r["p0"][1]
        p1 = 0 if r["p1"] is None else tensors[r["p1"][0]].data_ptr() + r["p1"][1]
        t[b] = (p0, p1, r["hs"], r["ws"], r["pitch"], r["cpitch"], r["fmt"], r["divisor"], r["min_score"], r["max_crops"],
                r["pad_q8"], r["fill"], r["mask"])
    return t


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().ravel()


def run_case(dev, rows, sizes, boxes, layout, ids, cnt, size, flags=KEEP, kind="u8", capacity=24, mean=None, scale=None, seed=0):
    """Launch over pseudo-random surfaces into pseudo-random output buffers and compare every byte of the four outputs with the
    restatement.  The three per-slot buffers are allocated TWO SLOTS LONGER than the capacity the call is given: what lies past the
    capacity is compared too.  -> (count, out [capacity, 3, ch, cw] numpy in NP_DTYPE[kind], out_index, out_rect, the BGR frames)."""
    max_list = boxes.shape[1]
    assert_fair(rows, boxes, layout, cnt, max_list)
    rng = np.random.RandomState(seed)
    host = [rng.randint(0, 256, size=n).astype(np.uint8) for n in sizes]
    tensors = [torch.from_numpy(h.copy()).to(dev) for h in host]
    table = torch.from_numpy(table_of(rows, tensors).view(np.uint8).copy()).to(dev)
    ch, cw = size
    item = np.dtype(NP_DTYPE[kind]).itemsize
    room = capacity + 2
    fill = [rng.randint(0, 256, size=n).astype(np.uint8) for n in (room * 3 * ch * cw * item, room * 16, room * 16, 8)]
    out = torch.from_numpy(fill[0].copy()).view(DTYPES[kind]).view(room, 3, ch, cw).to(dev)
    index, rect = (torch.from_numpy(f.copy()).view(torch.int32).view(room, 4).to(dev) for f in fill[1:3])
    count = torch.from_numpy(fill[3].copy()).view(torch.int32).to(dev)
    t_ids = None if ids is None else torch.from_numpy(ids).to(dev)
    t_mean = None if mean is None else torch.from_numpy(mean).to(dev)
    t_scale = None if scale is None else torch.from_numpy(scale).to(dev)
    ops.crop_gather(table, len(rows), torch.from_numpy(boxes).to(dev), layout, t_ids, torch.from_numpy(cnt).to(dev), out[:capacity],
                    index[:capacity], rect[:capacity], count, flags=flags, mean=t_mean, scale=t_scale)
    frames = [frame_of(r, host) if possible(r) else None for r in rows]
    w_out = fill[0].copy().view(NP_DTYPE[kind]).reshape(room, 3, ch, cw)
    w_index, w_rect = (f.copy().view(np.int32).reshape(room, 4) for f in fill[1:3])
    w_count = fill[3].copy().view(np.int32)
    restate(rows, frames, boxes, layout, ids, cnt, max_list, flags, kind, mean, scale, w_out[:capacity], w_index[:capacity],
            w_rect[:capacity], w_count)
    assert np.array_equal(raw(count), w_count.view(np.uint8)), (raw(count).view(np.int32), w_count)
    assert np.array_equal(raw(index), w_index.view(np.uint8).ravel()), "out_index differs"
    assert np.array_equal(raw(rect), w_rect.view(np.uint8).ravel()), "out_rect differs"
    got = raw(out)
    assert np.array_equal(got, w_out.view(np.uint8).ravel()), "%d bytes of out differ" % int((got != w_out.view(np.uint8).ravel()).sum())
    for t, h in zip(tensors, host):                                  # the sources are only read
        assert np.array_equal(raw(t), h)
    return w_count.copy(), w_out[:capacity], w_index[:capacity], w_rect[:capacity], frames


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,with_ids", [(0, False), (1, True), (1, False)])
def test_four_formats_one_launch(backend, layout, with_ids):
    """B = 5 rows (dense BGR, RGB with a pitch, NV12 with a padded luma plane and a detached chroma plane, P010, no surface) of
    different sizes, divisors, paddings and fill colours; sixteen entries per row covering every branch of rules 1 to 3."""
    rows, sizes = make_rows()
    boxes, ids, cnt = make_lists(rows, layout, 16, 24)
    count, _, index, _, _ = run_case(backend, rows, sizes, boxes, layout, ids if with_ids else None, cnt, (16, 24), capacity=40)
    assert tuple(count) == (32, 32)                                  # entries 0-3, 7-9 and 15 of each of the four surfaces
    assert list(index[:8, 1]) == [0, 1, 2, 3, 7, 8, 9, 15] and list(index[::8, 0][:4]) == [0, 1, 2, 3]
    assert list(index[:4, 2]) == ([3, 17, 5, 123456] if with_ids else [-1] * 4)


@pytest.mark.parametrize("kind", ["u8", "f32", "f16", "bf16"])
@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_output_variants(backend, kind, order):
    """The four output types with a mean and a scale per plane (uint8 has none), both plane orders."""
    rows, sizes = make_rows()
    boxes, ids, cnt = make_lists(rows, 1, 8, 8)
    flags = KEEP | (RGB_OUT if order == "rgb" else 0)
    mean, scale = (None, None) if kind == "u8" else (MEAN, SCALE)
    count, out, _, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (8, 8), flags=flags, kind=kind, capacity=33, mean=mean,
                                   scale=scale, seed=1)
    assert tuple(count) == (32, 32)
    if kind == "f32":                                                # (the case does normalise: values around 0, not 0..255)
        assert -3.0 < out[:32].min() < 0.0 < out[:32].max() < 3.0


def test_float_output_without_mean_and_scale(backend):
    rows, sizes = make_rows()
    boxes, ids, cnt = make_lists(rows, 1, 8, 8)
    _, out, _, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (8, 8), kind="f16", capacity=32, seed=2)
    assert out.astype(np.float32).max() > 128.0


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("pad_q8", [0, 26, 256])
def test_aspect_and_padding(backend, size, keep, pad_q8):
    """Keep-aspect and stretch under the three paddings for the three crop shapes, on every format."""
    rows, sizes = make_rows()
    for r in rows:
        r["pad_q8"] = pad_q8
    boxes, ids, cnt = make_lists(rows, 1, *size)
    count, _, _, rect, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, size, flags=KEEP if keep else 0, capacity=32, seed=3)
    assert tuple(count) == (32, 32)
    if keep:                                                         # every sampled rectangle has the crop's aspect, to a pixel
        w, h = rect[:32, 2] - rect[:32, 0] + 1, rect[:32, 3] - rect[:32, 1] + 1
        assert np.all(np.abs(w * size[0] - h * size[1]) < np.maximum(size[0], size[1]))


def test_odd_growth_goes_right_and_down(backend):
    """Numbers worked by hand from rules 2 and 3, not from the restatement: 8 x 8 crops from a 64 x 48 BGR surface."""
    row, sizes = surface(BGR, 48, 64, 192, 0)
    boxes = np.zeros((1, 4, 6), dtype=np.float32)
    boxes[0, 0] = (20, 10, 25, 20, 0.9137, 0)                        # 5 x 10: W' = 10, grows by 5: 2 on the left, 3 on the right
    boxes[0, 1] = (10, 20, 20, 23, 0.9137, 0)                        # 10 x 3: H' = 10, grows by 7: 3 at the top, 4 at the bottom
    boxes[0, 2] = (30, 30, 37, 37, 0.9137, 0)                        # 7 x 7: already square
    boxes[0, 3] = (40, 8, 50, 28, 0.9137, 0)                         # 10 x 20 with pad 26 / 256: px = 1, py = 2 -> 12 x 24 -> 24 x 24
    cnt = np.array([3], dtype=np.int32)
    _, _, _, rect, _ = run_case(backend, [row], sizes, boxes, 1, None, cnt, (8, 8), capacity=4)
    assert rect[:3].tolist() == [[18, 10, 27, 19], [10, 17, 19, 26], [30, 30, 36, 36]]
    _, _, _, rect, _ = run_case(backend, [dict(row, pad_q8=26)], sizes, boxes[:, 3:].copy(), 1, None, np.array([1], dtype=np.int32), (8, 8), capacity=4)
    assert rect[0].tolist() == [33, 6, 56, 29]
    _, _, _, rect, _ = run_case(backend, [dict(row, pad_q8=26)], sizes, boxes[:, 3:].copy(), 1, None, np.array([1], dtype=np.int32), (8, 8), flags=0,
                                capacity=4)
    assert rect[0].tolist() == [39, 6, 50, 29]                       # stretch: the padded rectangle as it is


@pytest.mark.parametrize("size", SIZES)
def test_identity(backend, size):
    """A box of exactly Ch x Cw pixels with no padding: the crop is the slice cut from the (converted) source — compared with the
    slice itself, whatever the restatement says."""
    rows, sizes = make_rows()
    ch, cw = size
    boxes = np.zeros((5, 2, 6), dtype=np.float32)
    at = [(3, 5), (11, 2), (0, 0), (0, 0)]                           # (x, y); the P010 surface is 32 rows high: the 32 x 8 crop starts at row 0
    for b, (x, y) in enumerate(at):
        d = rows[b]["divisor"]
        c = [x, y, x + cw, y + ch]
        boxes[b, 0, :4] = [p * d for p in c] if d in (1.0, 0.5) else [np.float32(d * (p + 0.25)) for p in c]
        boxes[b, 0, 4:] = (0.9137, 1)
        rows[b]["pad_q8"] = 0
    cnt = np.array([1, 1, 1, 1, 1], dtype=np.int32)
    count, out, _, rect, frames = run_case(backend, rows, sizes, boxes, 1, None, cnt, size, capacity=5, seed=4)
    assert tuple(count) == (4, 4)
    for b, (x, y) in enumerate(at):
        assert rect[b].tolist() == [x, y, x + cw - 1, y + ch - 1]
        assert np.array_equal(out[b], np.moveaxis(frames[b][y:y + ch, x:x + cw], 2, 0))


def test_one_pixel_box(backend):
    """A 1 x 1 box, stretched: every tap is that pixel, the crop is constant."""
    rows, sizes = make_rows()
    boxes = np.zeros((5, 1, 6), dtype=np.float32)
    for b in range(4):
        d = rows[b]["divisor"]
        c = [9, 7, 10, 8]
        boxes[b, 0, :4] = [p * d for p in c] if d in (1.0, 0.5) else [np.float32(d * (p + 0.25)) for p in c]
        boxes[b, 0, 4:] = (0.9137, 1)
        rows[b]["pad_q8"] = 0
    count, out, _, _, frames = run_case(backend, rows, sizes, boxes, 1, None, np.ones(5, dtype=np.int32), (16, 24), flags=0, capacity=4,
                                        seed=5)
    assert tuple(count) == (4, 4)
    for b in range(4):
        assert np.array_equal(out[b], np.broadcast_to(frames[b][7, 9][:, None, None], (3, 16, 24)))


def test_boxes_outside_the_surface(backend):
    """Half outside: the outside half is the fill colour.  Fully outside (on each side, and touching the edge from outside): skipped."""
    row, sizes = surface(BGR, 48, 64, 192, 0, fill=(7, 99, 201, 0))
    boxes = np.zeros((1, 8, 6), dtype=np.float32)
    boxes[0, :, 4:] = (0.9137, 0)
    boxes[0, 0, :4] = (-8, 8, 8, 24)                                 # 16 x 16, its left half outside
    boxes[0, 1, :4] = (-20, 8, 0, 24)                                # X2 = -1: outside
    boxes[0, 2, :4] = (64, 8, 80, 24)                                # X1 = Ws: outside
    boxes[0, 3, :4] = (8, -30, 24, 0)                                # above
    boxes[0, 4, :4] = (8, 48, 24, 60)                                # below
    boxes[0, 5, :4] = (56, 40, 72, 56)                               # the bottom right corner: three quarters outside
    boxes[0, 6, :4] = (-5, -5, 1, 1)                                 # meets the surface in pixel (0, 0) alone
    count, out, index, _, frames = run_case(backend, [row], sizes, boxes, 1, None, np.array([7], dtype=np.int32), (16, 16), flags=0, capacity=8)
    assert tuple(count) == (3, 3) and index[:3, 1].tolist() == [0, 5, 6]
    fill = np.array([7, 99, 201], dtype=np.uint8)[:, None, None]
    assert np.array_equal(out[0][:, :, :8], np.broadcast_to(fill, (3, 16, 8)))       # 16 -> 16 pixels: the identity, half of it fill
    assert np.array_equal(out[0][:, :, 8:], np.moveaxis(frames[0][8:24, 0:8], 2, 0))
    assert np.array_equal(out[1][:, 8:, :], np.broadcast_to(fill, (3, 8, 16)))
    assert np.array_equal(out[1][:, :, 8:], np.broadcast_to(fill, (3, 16, 8)))


def test_oversize_rectangles_are_skipped(backend):
    """A padded (or aspect-grown) side above 16384 pixels is skipped; 16384 itself is sampled."""
    row, sizes = surface(BGR, 48, 64, 192, 0)
    boxes = np.zeros((1, 6, 6), dtype=np.float32)
    boxes[0, :, 4:] = (0.9137, 0)
    boxes[0, 0, :4] = (-100, 10, 16284, 20)                          # W = 16384: kept (stretch)
    boxes[0, 1, :4] = (-100, 10, 16285, 20)                          # W = 16385: skipped
    boxes[0, 2, :4] = (10, -9000, 20, 9000)                          # H = 18000: skipped
    boxes[0, 3, :4] = (-1e9, -1e9, 1e9, 1e9)                         # the whole plane and more
    boxes[0, 4, :4] = (-3e9, 4, 3e9, 8)                              # clamped to +-2^30 before it becomes an integer
    boxes[0, 5, :4] = (4, 4, 12, 12)
    cnt = np.array([6], dtype=np.int32)
    count, _, index, _, _ = run_case(backend, [row], sizes, boxes, 1, None, cnt, (8, 8), flags=0, capacity=4)
    assert tuple(count) == (2, 2) and index[:2, 1].tolist() == [0, 5]
    # padding takes a side over the limit: 6000 + 2 * 6000 = 18000; keep-aspect does: 9000 x 10 into 32 x 8 asks for H' = 36000
    boxes[0, 0, :4] = (-100, 10, 5900, 20)
    count, _, index, _, _ = run_case(backend, [dict(row, pad_q8=256)], sizes, boxes, 1, None, cnt, (8, 8), flags=0, capacity=4)
    assert tuple(count) == (1, 1) and index[0, 1] == 5
    boxes[0, 0, :4] = (-100, 10, 8900, 20)
    count, _, index, _, _ = run_case(backend, [row], sizes, boxes, 1, None, cnt, (32, 8), flags=0, capacity=4)
    assert tuple(count) == (2, 2)
    count, _, index, _, _ = run_case(backend, [row], sizes, boxes, 1, None, cnt, (32, 8), flags=KEEP, capacity=4)
    assert tuple(count) == (1, 1) and index[0, 1] == 5


def test_filters_caps_and_counts(backend):
    """The class mask, min_score, max_crops (it counts KEPT entries: skipped ones before them do not use it up), cnt = 0, cnt < 0
    and cnt above max_list."""
    rows, sizes = make_rows()
    boxes, ids, cnt = make_lists(rows, 1, 8, 8)
    rows[0].update(mask=(0b1011, 0, 0, 0))                           # classes 0, 1, 3: entries 0, 1, 7, 8 (2, 5, 127 and 4 are left out)
    rows[1].update(max_crops=5)                                      # kept entries 0, 1, 2, 3, 7: entries 4 to 6 were skipped, not counted
    rows[2].update(min_score=0.8)                                    # entries 0, 1, 2, 3
    rows[3].update(mask=(0, 0, 0, 1 << 31), max_crops=1)             # class 127 alone: entry 3
    count, _, index, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (8, 8), capacity=20, seed=6)
    assert tuple(count) == (14, 14)
    assert index[:14, :2].tolist() == [[0, 0], [0, 1], [0, 7], [0, 8], [1, 0], [1, 1], [1, 2], [1, 3], [1, 7], [2, 0], [2, 1], [2, 2],
                                       [2, 3], [3, 3]]
    rows, _ = make_rows()
    cnt[:] = (0, -3, 100, 16, 16)                                    # 100 > max_list 20: the empty entries behind the 16 are looked at
    boxes[:, 16:, 4] = 0.0137
    count, _, index, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (8, 8), capacity=20, seed=7)
    assert tuple(count) == (16, 16) and set(index[:16, 0].tolist()) == {2, 3}
    count, _, _, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, np.zeros(5, dtype=np.int32), (8, 8), capacity=20, seed=8)
    assert tuple(count) == (0, 0)                                    # nothing but out_count is written


def test_capacity_overflow(backend):
    """Twenty kept entries into eight slots: out_count = (8, 20), the slots are the first eight in order, nothing behind them."""
    rows, sizes = make_rows()
    rows = rows[:3]
    boxes = np.zeros((3, 10, 6), dtype=np.float32)
    for b, n in enumerate((6, 10, 6)):                               # row 1: entries 3 and 7 are skipped: 6 + 8 + 6 kept
        for k in range(n):
            c = [2 + 3 * k, 4 + k, 14 + 3 * k, 20 + 2 * k]
            d = rows[b]["divisor"]
            boxes[b, k, :4] = [p * d for p in c] if d in (1.0, 0.5) else [np.float32(d * (p + 0.25)) for p in c]
            boxes[b, k, 4:] = (0.9137 if not (b == 1 and k in (3, 7)) else 0.1137, k % 4)
    cnt = np.array([6, 10, 6], dtype=np.int32)
    count, _, index, _, _ = run_case(backend, rows, sizes[:4], boxes, 1, None, cnt, (16, 24), capacity=8, seed=9)
    assert tuple(count) == (8, 20)
    assert index[:, :2].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [0, 4], [0, 5], [1, 0], [1, 1]]


def test_full_list_of_256(backend):
    """cnt = 300 on one row: entries 0..255 are looked at — every thread of the plan resolves one, every wave numbers its own —
    entry 256 is not."""
    rng = np.random.RandomState(10)
    row, sizes = surface(BGR, 48, 64, 192, 0, pad_q8=26)
    boxes = np.zeros((1, 300, 6), dtype=np.float32)
    x1, y1 = rng.randint(-6, 60, size=300), rng.randint(-6, 44, size=300)
    boxes[0, :, 0], boxes[0, :, 1] = x1, y1
    boxes[0, :, 2], boxes[0, :, 3] = x1 + rng.randint(1, 24, size=300), y1 + rng.randint(1, 24, size=300)
    boxes[0, :, 4] = np.where(np.arange(300) % 7 == 3, 0.1234, 0.9137)
    boxes[0, :, 5] = rng.randint(0, 9, size=300)
    ids = rng.randint(0, 300000, size=(1, 300)).astype(np.int32)
    cnt = np.array([300], dtype=np.int32)
    count, _, index, _, _ = run_case(backend, [row], sizes, boxes, 1, ids, cnt, (8, 8), capacity=256, seed=11)
    assert 150 < count[0] == count[1] < 256 and index[count[0] - 1, 1] > 245
    lone = np.zeros_like(boxes)
    lone[0, :, 4] = 0.0137
    lone[0, 255] = (8, 24, 40, 40, 0.9137, 1)
    lone[0, 256] = (44, 4, 60, 20, 0.9137, 2)
    count, _, index, _, _ = run_case(backend, [row], sizes, lone, 1, ids, cnt, (8, 8), capacity=4, seed=12)
    assert tuple(count) == (1, 1) and index[0, 1] == 255


def test_descriptors_no_surface_can_have(backend):
    """An unknown format, odd NV12 / P010 sizes, a pitch below the row's bytes, a negative chroma pitch, no plane, Hs == 0: the row
    keeps nothing (and, the allocations being the exact minimum, reads nothing); the good row between them is served."""
    rows, sizes = make_rows()
    boxes, ids, cnt = make_lists(rows, 1, 8, 8)
    rows[4] = dict(rows[2], cpitch=63)                               # a chroma pitch below Ws
    rows[0].update(fmt=7)
    rows[1].update(pitch=3 * 70 - 1)
    rows[2].update(hs=47)
    count, _, index, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (8, 8), capacity=10, seed=13)
    assert tuple(count) == (8, 8) and set(index[:8, 0].tolist()) == {3}
    rows, _ = make_rows()
    rows[4] = dict(rows[0], hs=0)
    rows[0].update(fmt=-1)
    rows[1].update(ws=0)
    rows[2].update(ws=63)                                            # an odd width
    rows[3].update(pitch=2 * 48 - 2)                                 # a luma pitch below 2 Ws
    count, _, _, _, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (8, 8), capacity=10, seed=14)
    assert tuple(count) == (0, 0)
    rows, _ = make_rows()
    rows[2].update(cpitch=-80)
    rows[3].update(p1=(4, 0), cpitch=95)                             # a chroma pitch below 2 Ws
    count, _, index, _, _ = run_case(backend, rows[2:4], sizes, boxes[2:4].copy(), 1, ids[2:4].copy(), cnt[2:4].copy(), (8, 8), capacity=10,
                                     seed=15)
    assert tuple(count) == (0, 0)


def test_status_codes(backend):
    dev = backend
    rows, sizes = make_rows()
    boxes, ids, cnt = make_lists(rows, 1, 8, 8)
    tensors = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in sizes]
    table = torch.from_numpy(table_of(rows, tensors).view(np.uint8).copy()).to(dev)
    tb, ti, tc = torch.from_numpy(boxes).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(cnt).to(dev)
    out = torch.zeros((4, 3, 8, 8), dtype=torch.float32, device=dev)
    index, rect = torch.zeros((4, 4), dtype=torch.int32, device=dev), torch.zeros((4, 4), dtype=torch.int32, device=dev)
    count, ms = torch.zeros(2, dtype=torch.int32, device=dev), torch.ones(3, dtype=torch.float32, device=dev)
    good = dict(rows=table.data_ptr(), B=5, boxes=tb.data_ptr(), layout=1, max_list=20, ids=ti.data_ptr(), cnt=tc.data_ptr(), Ch=8, Cw=8,
                flags=3, out_dtype=_lib.DT_F32, mean3=ms.data_ptr(), scale3=ms.data_ptr(), out=out.data_ptr(), capacity=4,
                out_index=index.data_ptr(), out_rect=rect.data_ptr(), out_count=count.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return _lib.lib().sy_crop_gather(a["rows"], a["B"], a["boxes"], a["layout"], a["max_list"], a["ids"], a["cnt"], a["Ch"], a["Cw"],
                                         a["flags"], a["out_dtype"], a["mean3"], a["scale3"], a["out"], a["capacity"], a["out_index"],
                                         a["out_rect"], a["out_count"], ops.stream_of(table))
    assert call() == 0 and count.tolist() == [4, 32]
    assert call(ids=None) == 0 and call(mean3=None) == 0 and call(scale3=None) == 0 and call(flags=0) == 0
    for kw in (dict(rows=None), dict(boxes=None), dict(cnt=None), dict(out=None), dict(out_index=None), dict(out_rect=None),
               dict(out_count=None), dict(B=0), dict(B=-1), dict(max_list=0), dict(capacity=0), dict(capacity=-2), dict(layout=2),
               dict(layout=-1), dict(flags=4), dict(flags=-1), dict(out_dtype=4), dict(out_dtype=-1)):
        assert call(**kw) == 1, kw                                   # SY_ERR_ARG
    for kw in (dict(Cw=12), dict(Cw=4), dict(Ch=7), dict(Ch=0), dict(Ch=513), dict(Cw=520), dict(Cw=-8), dict(B=1025)):
        assert call(**kw) == _lib.SY_ERR_UNSUPPORTED, kw
    assert C.sizeof(_lib.CropRow) == _CROP_DTYPE.itemsize == 72

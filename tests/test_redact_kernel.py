"""sy_redact (csrc/redact.hip) on hand-made box lists, on the SIMT emulator and on the MI355X.

The yardstick is `restate` below: the nine points of the rule as include/streamyolo_hip.h states it, written in plain numpy over
whole frames — a coverage mask per surface, then cells — which knows nothing of tiles, chunks or threads.  It is computed from a
copy of the ORIGINAL bytes, so a kernel that read a pixel after somebody rewrote it would show as a mismatch.  The comparison is
np.array_equal on the ENTIRE backing allocation of every plane; the buffers are pre-filled with pseudo-random bytes and every
plane is backed by the exact minimum allocation — (rows - 1) * pitch + the row's bytes — so nothing behind a surface's last
payload byte can be touched unnoticed where the memory ends there.

No tolerance: the rule is integer arithmetic behind one float division and one floor.  To make that a fair demand of fp32 every
case asserts on ITS OWN INPUTS, in float64, that each c / divisor + 0.5 the launch looks at is at least 1e-3 away from an integer
and each score 1e-3 away from min_score.  Boxes are integers under the divisors 1 and 0.5; rows with the divisor 0.3 get
coordinates constructed to land a quarter pixel inside their cell.  Every positive case also requires that the restatement
itself changed at least one byte: no case passes by covering nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from streamyolo_amd import _lib, ops
from streamyolo_amd.redact import _REDACT_DTYPE
from test_overlay_kernel import _round_px

MARGIN = 1e-3
BGR, RGB, NV12, P010 = _lib.PIX_BGR, _lib.PIX_RGB, _lib.PIX_NV12, _lib.PIX_P010
PIXELATE, FILL = _lib.REDACT_PIXELATE, _lib.REDACT_FILL
RECT, ELLIPSE = _lib.REDACT_RECT, _lib.REDACT_ELLIPSE
MAX_SIDE = _lib.REDACT_MAX_SIDE
MIN_SCORE = 0.3
ALL = (0xFFFFFFFF,) * 4
FILL_BYTES = (10, 200, 90, 0, 77, 140, 33, 0)                        # B, G, R, 0, Y, U, V, 0 (the kernel converts nothing)


# ---- the rule, restated from the header --------------------------------------------------------------------------------
def possible(row):
    """Rule 9: a descriptor a surface can have."""
    hs, ws, fmt = row["hs"], row["ws"], row["fmt"]
    if row["p0"] is None or hs <= 0 or ws <= 0 or fmt not in (BGR, RGB, NV12, P010):
        return False
    if row["cell"] not in (4, 8, 16, 32) or row["mode"] not in (0, 1) or row["shape"] not in (0, 1):
        return False
    yuv = fmt in (NV12, P010)
    row_bytes = ws * (1 if fmt == NV12 else 2 if fmt == P010 else 3)
    cpitch = row["cpitch"] if row["cpitch"] != 0 else row["pitch"]
    return not (row["pitch"] < row_bytes or (yuv and (hs % 2 or ws % 2 or row["cpitch"] < 0 or cpitch < row_bytes)))


def rectangle(row, r, layout):
    """Rules 1 and 2 for one list entry -> the padded (X1, Y1, X2, Y2) or None (skipped).  Python integers: nothing overflows."""
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
    if x2 < x1 or y2 < y1:
        return None
    q = min(max(row["pad_q8"], 0), 256)
    w, h = x2 - x1 + 1, y2 - y1 + 1
    gx, gy = (w * q + 128) >> 8, (h * q + 128) >> 8
    return x1 - gx, y1 - gy, x2 + gx, y2 + gy


def coverage(row, boxes, layout, cnt, max_list):
    """Rules 1 to 4: the covered pixels of the row's surface, bool [hs, ws].  Every one of the min(cnt, max_list) entries counts."""
    hs, ws = row["hs"], row["ws"]
    cov = np.zeros((hs, ws), dtype=bool)
    for k in range(min(max(int(cnt), 0), max_list)):
        got = rectangle(row, boxes[k], layout)
        if got is None:
            continue
        x1, y1, x2, y2 = got
        w, h = x2 - x1 + 1, y2 - y1 + 1
        xa, xb, ya, yb = max(x1, 0), min(x2, ws - 1), max(y1, 0), min(y2, hs - 1)
        if xa > xb or ya > yb:
            continue
        if row["shape"] == ELLIPSE and w <= MAX_SIDE and h <= MAX_SIDE:
            dx = (2 * np.arange(xa, xb + 1, dtype=np.int64) + 1) - (2 * x1 + w)
            dy = (2 * np.arange(ya, yb + 1, dtype=np.int64) + 1) - (2 * y1 + h)
            cov[ya:yb + 1, xa:xb + 1] |= dx[None, :] ** 2 * (h * h) + dy[:, None] ** 2 * (w * w) <= w * w * h * h
        else:
            cov[ya:yb + 1, xa:xb + 1] = True
    return cov


def pixelate(plane, cov, cell):
    """Rule 6 on one plane [h, w, channels] (int64) with its coverage [h, w]: every covered sample takes its cell's rounded mean."""
    out = plane.copy()
    h, w = cov.shape
    for j in range(0, h, cell):
        for i in range(0, w, cell):
            c = cov[j:j + cell, i:i + cell]
            if c.any():
                block = plane[j:j + cell, i:i + cell]
                n = block.shape[0] * block.shape[1]
                out[j:j + cell, i:i + cell][c] = (block.reshape(n, -1).sum(axis=0) + (n >> 1)) // n
    return out


def restate(row, orig, out, boxes, layout, cnt, max_list):
    """The rule for one table row: reads the payload of `orig` (the backing buffers as they were), writes into `out` (copies of
    them).  -> the number of covered pixels."""
    if not possible(row):
        return 0
    hs, ws, fmt, pitch = row["hs"], row["ws"], row["fmt"], row["pitch"]
    cov = coverage(row, boxes, layout, cnt, max_list)
    if not cov.any():
        return 0
    fill, cell, b0, o0 = row["fill"], row["cell"], row["p0"][0], row["p0"][1]
    if fmt in (BGR, RGB):
        px = np.stack([orig[b0][o0 + y * pitch:o0 + y * pitch + 3 * ws] for y in range(hs)]).reshape(hs, ws, 3).astype(np.int64)
        if row["mode"] == FILL:
            new = np.empty_like(px)
            new[:] = fill[:3] if fmt == BGR else fill[2::-1]
        else:
            new = pixelate(px, cov, cell)
        for y in range(hs):
            line = out[b0][o0 + y * pitch:o0 + y * pitch + 3 * ws].reshape(ws, 3)
            line[cov[y]] = new[y][cov[y]]
        return int(cov.sum())
    step = 2 if fmt == P010 else 1                                   # P010: the high byte of every little-endian word
    b1, o1 = row["p1"] if row["p1"] is not None else (b0, o0 + pitch * hs)
    cpitch = row["cpitch"] if row["cpitch"] != 0 else pitch
    luma = np.stack([orig[b0][o0 + y * pitch + step - 1:o0 + y * pitch + step * ws:step] for y in range(hs)]).astype(np.int64)
    uv = np.stack([orig[b1][o1 + y * cpitch + step - 1:o1 + y * cpitch + step * ws:step] for y in range(hs // 2)]).astype(np.int64)
    uv = uv.reshape(hs // 2, ws // 2, 2)
    ccov = cov[0::2, 0::2] | cov[0::2, 1::2] | cov[1::2, 0::2] | cov[1::2, 1::2]      # rule 7: any of the four luma pixels
    if row["mode"] == FILL:
        new_y, new_uv = np.full_like(luma, fill[4]), np.empty_like(uv)
        new_uv[:] = fill[5:7]
    else:
        new_y = pixelate(luma[:, :, None], cov, cell)[:, :, 0]
        new_uv = pixelate(uv, ccov, cell // 2)
    for y in range(hs):
        line = out[b0][o0 + y * pitch:o0 + y * pitch + step * ws].reshape(ws, step)
        line[cov[y], step - 1] = new_y[y][cov[y]]
        if step == 2:
            line[cov[y], 0] = 0
    for y in range(hs // 2):
        line = out[b1][o1 + y * cpitch:o1 + y * cpitch + step * ws].reshape(ws // 2, 2, step)
        line[ccov[y], :, step - 1] = new_uv[y][ccov[y]]
        if step == 2:
            line[ccov[y], :, 0] = 0
    return int(cov.sum())


def assert_fair(rows, boxes, layout, cnt, max_list):
    """The condition on a case's OWN INPUTS under which fp32 must reproduce the rule exactly (float64)."""
    for b, row in enumerate(rows):
        for r in boxes[b, :min(max(int(cnt[b]), 0), max_list)]:
            for c in r[:4]:
                if np.isfinite(c):
                    v = np.float64(np.float32(c)) / np.float64(np.float32(row["divisor"])) + 0.5
                    assert abs(v - np.round(v)) >= MARGIN, (b, c, v)
            sc = np.float64(np.float32(r[4])) * np.float64(np.float32(r[5])) if layout == 0 else np.float64(np.float32(r[4]))
            if np.isfinite(sc):
                assert abs(sc - np.float64(np.float32(row["min_score"]))) >= MARGIN, (b, sc)


# ---- surfaces and lists ----------------------------------------------------------------------------------------------
def surface(fmt, hs, ws, pitch, first, cpitch=0, detached=False, **kw):
    """A table row over backing buffers first, first + 1 -> (row, sizes): every allocation is the exact minimum."""
    step = {BGR: 3, RGB: 3, NV12: 1, P010: 2}[fmt]
    row = dict(fmt=fmt, hs=hs, ws=ws, pitch=pitch, cpitch=cpitch, p0=(first, 0), p1=None, divisor=1.0, min_score=MIN_SCORE,
               pad_q8=0, mode=PIXELATE, cell=8, shape=RECT, fill=FILL_BYTES, mask=ALL)
    row.update(kw)
    if fmt in (BGR, RGB):
        return row, [(hs - 1) * pitch + step * ws]
    cp = cpitch or pitch
    if detached:
        row["p1"] = (first + 1, 0)
        return row, [(hs - 1) * pitch + step * ws, (hs // 2 - 1) * cp + step * ws]
    return row, [hs * pitch + (hs // 2 - 1) * cp + step * ws]


SURFACES = {
    "bgr": (BGR, 50, 150, 3 * 150 + 10, {}),                         # a padded pitch; 3 x 2 tiles, clipped cells on both edges
    "rgb": (RGB, 33, 70, 3 * 70, {}),
    "nv12": (NV12, 34, 66, 66, {}),                                  # contiguous: the chroma plane starts at row Hs
    "nv12_split": (NV12, 38, 70, 72, dict(cpitch=80, detached=True)),
    "p010": (P010, 36, 68, 2 * 68 + 4, {}),
}
MIXED = [("bgr", dict(divisor=1.0, pad_q8=0)), ("rgb", dict(divisor=0.5, pad_q8=26)),
         ("nv12_split", dict(divisor=0.3, pad_q8=256)), ("p010", dict(divisor=1.0, pad_q8=26))]


def make_rows(which, **common):
    """Table rows over consecutive backing buffers.  which: names of SURFACES or (name, per-row fields); the buffers are sized
    for the surface as SURFACES has it, the fields are written over the descriptor afterwards.  -> (rows, sizes)."""
    rows, sizes = [], []
    for w in which:
        name, own = (w, {}) if isinstance(w, str) else w
        fmt, hs, ws, pitch, kw = SURFACES[name]
        row, sz = surface(fmt, hs, ws, pitch, len(sizes), **kw)
        row.update(common)
        row.update(own)
        rows.append(row)
        sizes += sz
    return rows, sizes


def pixel_boxes(hs, ws):
    """Seventeen entries in SURFACE pixels, (x1, y1, x2, y2) covering [x1, x2) x [y1, y2).  -> list of (box, class, score)."""
    return [
        ((5, 3, 40, 28), 1, 0.957),                                  # 0 crosses cell borders of every size
        ((50, 20, 90, 45), 0, 0.921),                                # 1 crosses the tile borders x = 64 and y = 32
        ((58, 26, 75, 48), 2, 0.887),                                # 2 overlaps 1 (the union), crosses the same borders
        ((-6, 10, 7, 22), 2, 0.853),                                 # 3 partly off the left edge
        ((ws - 9, hs - 7, ws + 9, hs + 5), 127, 0.819),              # 4 crosses the bottom right corner; the last class id
        ((ws + 3, 4, ws + 12, 12), 0, 0.785),                        # 5 wholly off the surface (padding may bring it back in)
        ((30, 8, 22, 20), 1, 0.751),                                 # 6 x2 < x1: skipped
        ((np.nan, 8, 28, 24), 1, 0.717),                             # 7 a NaN coordinate: skipped
        ((44, 2, 45, 19), 3, 0.683),                                 # 8 one pixel wide: a 1-pixel-wide ellipse
        ((ws - 30, 1, ws - 21, 9), 5, 0.649),                        # 9 a class the row's mask may leave out
        ((8, 30, 40, hs - 1), 0, 0.2137),                            # 10 plainly visible, but its score is below min_score
        ((3, 3, 12, 18), np.nan, 0.615),                             # 11 a NaN class: skipped
        ((5, 5, np.inf, 12), 1, 0.581),                              # 12 an infinite coordinate: skipped
        ((5, 5, 16, 12), 128, 0.547),                                # 13 a class past the mask's 128 bits: skipped
        ((5, 5, 16, 12), -1, 0.513),                                 # 14 a negative class: skipped
        ((40, 30, 60, hs), 1, np.nan),                               # 15 a NaN score: skipped
        ((20, hs - 3, 29, hs + 40), 4, 0.479),                       # 16 hangs out of the bottom edge
    ]


def coords(px, d):
    """Box coordinates that the divisor d takes to the surface pixels px."""
    if d in (1.0, 0.5):
        return [p * d for p in px]                                   # exact in fp32: c / d + 0.5 is p + 0.5
    return [np.float32(d * (p + 0.25)) for p in px]                  # constructed: c / d + 0.5 lands a quarter pixel above p + 0.5


def make_lists(rows, layout, max_list=20):
    """boxes [B, max_list, 7 | 6] fp32 and cnt [B] for the rows' own box sets (entries beyond: zeros)."""
    boxes = np.zeros((len(rows), max_list, 7 if layout == 0 else 6), dtype=np.float32)
    for b, row in enumerate(rows):
        for k, (px, cls, score) in enumerate(pixel_boxes(row["hs"], row["ws"])):
            boxes[b, k, :4] = coords(px, row["divisor"])
            boxes[b, k, 4:] = (0.9, score / 0.9, cls) if layout == 0 else (score, cls)
    return boxes, np.full(len(rows), 17, dtype=np.int32)


def table_of(rows, tensors):
    t = np.zeros(len(rows), dtype=_REDACT_DTYPE)
    for b, r in enumerate(rows):
        p0 = 0 if r["p0"] is None else tensors[r["p0"][0]].data_ptr() + r["p0"][1]
        p1 = 0 if r["p1"] is None else tensors[r["p1"][0]].data_ptr() + r["p1"][1]
        t[b] = (p0, p1, r["hs"], r["ws"], r["pitch"], r["cpitch"], r["fmt"], r["divisor"], r["min_score"], r["pad_q8"], r["mode"],
                r["cell"], r["shape"], 0, r["fill"], r["mask"])
    return t


def run_case(dev, rows, sizes, boxes, layout, cnt, max_hw=None, seed=0):
    """Launch over pseudo-random backing buffers and compare every byte of them with the restatement of the ORIGINAL bytes.
    -> (covered pixels per row, the original buffers, the expected buffers)."""
    max_list = boxes.shape[1]
    assert_fair(rows, boxes, layout, cnt, max_list)
    if max_hw is None:
        max_hw = (max(max(r["hs"], 1) for r in rows), max(max(r["ws"], 1) for r in rows))
    rng = np.random.RandomState(seed)
    host = [rng.randint(0, 256, size=n).astype(np.uint8) for n in sizes]
    tensors = [torch.from_numpy(h.copy()).to(dev) for h in host]
    table = torch.from_numpy(table_of(rows, tensors).view(np.uint8).copy()).to(dev)
    ops.redact(table, len(rows), max_hw, torch.from_numpy(boxes).to(dev), layout, torch.from_numpy(cnt).to(dev))
    want = [h.copy() for h in host]
    covered = [restate(row, host, want, boxes[b], layout, cnt[b], max_list) for b, row in enumerate(rows)]
    for i, (w, t) in enumerate(zip(want, tensors)):
        got = t.cpu().numpy()
        assert np.array_equal(got, w), "buffer %d: %d bytes differ, first at %d" % (i, int((got != w).sum()), int(np.argmax(got != w)))
    return covered, host, want


def changed(host, want):
    return [int((h != w).sum()) for h, w in zip(host, want)]


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [RECT, ELLIPSE])
@pytest.mark.parametrize("mode", [PIXELATE, FILL])
@pytest.mark.parametrize("name", list(SURFACES))
def test_every_surface(backend, name, mode, shape):
    """Each of the five surfaces on its own, both modes and shapes: boxes across tile and cell borders, overlapping, partly and
    wholly off the surface, one pixel wide, filtered by score, class, NaN and inf."""
    rows, sizes = make_rows([name], mode=mode, shape=shape, pad_q8=26, cell=8)
    boxes, cnt = make_lists(rows, 1)
    covered, host, want = run_case(dev=backend, rows=rows, sizes=sizes, boxes=boxes, layout=1, cnt=cnt, seed=1)
    assert covered[0] > 0 and all(c > 0 for c in changed(host, want))


@pytest.mark.parametrize("shape", [RECT, ELLIPSE])
@pytest.mark.parametrize("mode", [PIXELATE, FILL])
@pytest.mark.parametrize("cell", [4, 8, 16, 32])
@pytest.mark.parametrize("layout", [0, 1])
def test_four_formats_one_launch(backend, layout, cell, mode, shape):
    """B = 4 rows of four formats, sizes, divisors (1, 0.5, 0.3, 1) and paddings (0, 26, 256, 26) in one launch whose Hmax x Wmax
    is larger than three of them; every cell size, both modes, both shapes, both list layouts."""
    rows, sizes = make_rows(MIXED, mode=mode, shape=shape, cell=cell)
    boxes, cnt = make_lists(rows, layout)
    covered, host, want = run_case(backend, rows, sizes, boxes, layout, cnt, max_hw=(50, 150), seed=2 + cell)
    assert all(c > 0 for c in covered) and all(c > 0 for c in changed(host, want))


@pytest.mark.parametrize("pad_q8", [0, 26, 256, -5, 999])
def test_padding(backend, pad_q8):
    """pad_q8 of 0, 26 and 256 on every row (and its clamping); with 256 entry 5, wholly off the surface, reaches back into it."""
    rows, sizes = make_rows(MIXED, shape=ELLIPSE, cell=4)
    for r in rows:
        r["pad_q8"] = pad_q8
    boxes, cnt = make_lists(rows, 1)
    lone = np.zeros_like(boxes)
    lone[:, :, 4] = 0.0137
    lone[:, 0] = boxes[:, 5]
    covered, _, _ = run_case(backend, rows, sizes, boxes, 1, cnt, seed=3)
    assert all(c > 0 for c in covered)
    rows = [dict(r, shape=RECT) for r in rows]
    covered, _, _ = run_case(backend, rows, sizes, lone, 1, cnt, seed=4)
    assert all((c > 0) == (pad_q8 >= 256) for c in covered)


def test_union_does_not_depend_on_the_order(backend):
    """The list reversed gives identical bytes."""
    rows, sizes = make_rows(MIXED, shape=ELLIPSE, cell=16, pad_q8=26)
    boxes, cnt = make_lists(rows, 1, max_list=17)
    covered, _, want = run_case(backend, rows, sizes, boxes, 1, cnt, seed=5)
    covered_r, _, want_r = run_case(backend, rows, sizes, boxes[:, ::-1].copy(), 1, cnt, seed=5)
    assert covered == covered_r and all(c > 0 for c in covered)
    assert all(np.array_equal(a, b) for a, b in zip(want, want_r))


def test_one_pixel_wide_ellipses(backend):
    """W = 1 or H = 1 under ELLIPSE: the whole line is inside (the centre column's dx is 0)."""
    rows, sizes = make_rows(["bgr", "nv12"], shape=ELLIPSE, mode=FILL, cell=4)
    boxes = np.zeros((2, 4, 6), dtype=np.float32)
    boxes[:, :, 4:] = (0.9137, 1)
    boxes[:, 0, :4] = (9, 2, 10, 31)                                 # a column
    boxes[:, 1, :4] = (20, 13, 66, 14)                               # a row across the tile border, to the NV12 surface's last column
    boxes[:, 2, :4] = (63, 20, 64, 21)                               # one pixel, the last of its tile
    boxes[:, 3, :4] = (30, 0, 33, 1)                                 # H = 1, W = 3
    covered, _, _ = run_case(backend, rows, sizes, boxes, 1, np.array([4, 4], dtype=np.int32), seed=6)
    assert covered == [29 + 46 + 1 + 3, 29 + 46 + 1 + 3]


def test_oversize_ellipse_is_its_rectangle(backend):
    """W > 16384 under ELLIPSE: covered as a rectangle — here the whole surface, corners included; W = 16384 is still an ellipse."""
    rows, sizes = make_rows(["bgr", "p010"], shape=ELLIPSE, mode=FILL, cell=32)
    boxes = np.zeros((2, 1, 6), dtype=np.float32)
    boxes[:, 0] = (-9000, -10, 9000, 60, 0.9137, 0)
    one = np.ones(2, dtype=np.int32)
    covered, host, want = run_case(backend, rows, sizes, boxes, 1, one, seed=7)
    assert covered == [50 * 150, 36 * 68]
    line = want[0][:450].reshape(150, 3)                             # (the first row of the BGR surface: all fill, in B, G, R)
    assert (line == np.array(FILL_BYTES[:3], dtype=np.uint8)).all()
    boxes[:, 0, :4] = (-16364, 10, 20, 40)                           # W = 16384: still an ellipse, of which the surface sees the right tip
    covered, host, want = run_case(backend, rows, sizes, boxes, 1, one, seed=8)
    assert 0 < covered[0] < 100 and 0 < covered[1] < 100
    boxes[:, 0, :4] = (-16365, 10, 20, 40)                           # W = 16385: the rectangle, 20 columns of the rows 10 to 39
    covered, host, want = run_case(backend, rows, sizes, boxes, 1, one, seed=8)
    assert covered == [20 * 30, 20 * 26]
    boxes[:, 0, :4] = (-3e9, -3e9, 3e9, 3e9)                         # clamped to +-2^30 before it becomes an integer
    covered, _, _ = run_case(backend, [dict(r, pad_q8=256) for r in rows], sizes, boxes, 1, one, seed=9)
    assert covered == [50 * 150, 36 * 68]


def test_filters_and_counts(backend):
    """The class mask, min_score; cnt = 0, cnt < 0 and cnt above max_list."""
    rows, sizes = make_rows(MIXED, cell=8)
    boxes, cnt = make_lists(rows, 1)
    base, _, _ = run_case(backend, rows, sizes, boxes, 1, cnt, seed=10)
    rows[0].update(mask=(0xFFFFFFFF & ~(1 << 5), 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))      # without class 5: entry 9 stays visible
    rows[1].update(min_score=0.8)                                    # entries 0 to 4
    rows[2].update(mask=(0, 0, 0, 1 << 31))                          # class 127 alone: entry 4
    rows[3].update(min_score=0.1)                                    # entry 10 too
    got, _, _ = run_case(backend, rows, sizes, boxes, 1, cnt, seed=10)
    assert 0 < got[0] < base[0] and 0 < got[1] < base[1] and 0 < got[2] < base[2] and got[3] > base[3]
    rows, _ = make_rows(MIXED, cell=8)
    late = boxes.copy()
    late[:, 17:, 4] = 0.0137
    late[:, 19] = boxes[:, 0]                                        # entry 19 is seen only by a count of 20 or more
    late[:, 0, 4] = 0.0137
    cnt = np.array([0, -3, 100, 19], dtype=np.int32)                 # 100 > max_list 20: all twenty entries are looked at
    got, host, want = run_case(backend, rows, sizes, late, 1, cnt, seed=11)
    assert got[0] == 0 and got[1] == 0 and got[2] > 0 and got[3] > 0
    assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1])
    full, _, _ = run_case(backend, rows, sizes, late, 1, np.full(4, 20, dtype=np.int32), seed=11)
    assert full[3] > got[3]


def test_no_cap_of_256(backend):
    """A list of 300 entries: entries 256 to 299 cover pixels nothing else covers, and they are covered."""
    rng = np.random.RandomState(12)
    rows, sizes = make_rows(["bgr", "nv12_split"], cell=4, shape=ELLIPSE, pad_q8=26)
    boxes = np.zeros((2, 300, 6), dtype=np.float32)
    for b, r in enumerate(rows):
        x1 = np.where(np.arange(300) < 256, rng.randint(-6, 30, size=300), rng.randint(44, r["ws"] - 4, size=300))
        y1 = rng.randint(-6, r["hs"] - 4, size=300)
        boxes[b, :, 0], boxes[b, :, 1] = x1, y1
        boxes[b, :, 2], boxes[b, :, 3] = x1 + rng.randint(1, 9, size=300), y1 + rng.randint(1, 9, size=300)
        boxes[b, :, 4] = np.where(np.arange(300) % 7 == 3, 0.1234, 0.9137)
        boxes[b, :, 5] = rng.randint(0, 9, size=300)
    assert boxes[:, :256, 2].max() * 1.1 + 2 < 44                    # (padded: entries 0..255 end left of column 44)
    cnt = np.array([300, 300], dtype=np.int32)
    covered, host, want = run_case(backend, rows, sizes, boxes, 1, cnt, seed=13)
    first, _, want_256 = run_case(backend, rows, sizes, boxes, 1, np.array([256, 256], dtype=np.int32), seed=13)
    assert all(c > f > 0 for c, f in zip(covered, first))
    for b, r in enumerate(rows):                                     # right of column 44: nothing under 256 entries, something under 300
        right = lambda buf: np.stack([buf[r["p0"][0]][y * r["pitch"]:][(3 if r["fmt"] == BGR else 1) * 44:(3 if r["fmt"] == BGR else 1) * r["ws"]]
                                      for y in range(r["hs"])])
        assert np.array_equal(right(want_256), right(host)) and not np.array_equal(right(want), right(host))
    covered_r, _, want_r = run_case(backend, rows, sizes, boxes[:, ::-1].copy(), 1, cnt, seed=13)
    assert covered_r == covered and all(np.array_equal(a, b) for a, b in zip(want, want_r))


def test_descriptors_no_surface_can_have(backend):
    """Every impossible descriptor of rule 9 leaves its buffers untouched (and, the allocations being the exact minimum, reads
    nothing); the good row between them is served."""
    bad = [("bgr", dict(fmt=7)), ("bgr", dict(fmt=-1)), ("rgb", dict(pitch=3 * 70 - 1)), ("nv12", dict(hs=33)), ("nv12_split", dict(ws=69)),
           ("p010", dict(pitch=2 * 68 - 2)), ("nv12_split", dict(cpitch=-80)), ("nv12_split", dict(cpitch=69)), ("bgr", dict(hs=0)),
           ("rgb", dict(ws=0)), ("bgr", dict(hs=-4)), ("bgr", dict(cell=0)), ("rgb", dict(cell=12)), ("nv12", dict(cell=64)),
           ("p010", dict(cell=2)), ("bgr", dict(cell=8, mode=2)), ("nv12", dict(mode=-1)), ("rgb", dict(shape=2)), ("p010", dict(shape=-1)),
           ("bgr", dict(mode=FILL, cell=5))]
    for at in range(0, len(bad), 5):
        which = bad[at:at + 5]
        rows, sizes = make_rows(which[:2] + ["p010"] + which[2:], pad_q8=26)
        for r, (name, _) in zip(rows, which[:2] + [("p010", {})] + which[2:]):      # the lists are made for the surface as allocated
            r["_hs"], r["_ws"] = SURFACES[name][1], SURFACES[name][2]
        boxes = np.zeros((len(rows), 20, 6), dtype=np.float32)
        for b, r in enumerate(rows):
            for k, (px, cls, score) in enumerate(pixel_boxes(r["_hs"], r["_ws"])):
                boxes[b, k] = coords(px, r["divisor"]) + [score, cls]
        cnt = np.full(len(rows), 17, dtype=np.int32)
        covered, host, want = run_case(backend, rows, sizes, boxes, 1, cnt, max_hw=(50, 150), seed=14 + at)
        assert [c > 0 for c in covered] == [b == 2 for b in range(len(rows))]
        assert sum(c > 0 for c in changed(host, want)) == 1
    rows, sizes = make_rows(MIXED)
    rows.append(dict(rows[0], p0=None))                              # no plane at all
    boxes, cnt = make_lists(rows, 1)
    covered, _, _ = run_case(backend, rows, sizes, boxes, 1, cnt, seed=15)
    assert covered[4] == 0 and all(c > 0 for c in covered[:4])


def test_status_codes(backend):
    dev = backend
    rows, sizes = make_rows(MIXED)
    boxes, cnt = make_lists(rows, 1)
    tensors = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in sizes]
    table = torch.from_numpy(table_of(rows, tensors).view(np.uint8).copy()).to(dev)
    tb, tc = torch.from_numpy(boxes).to(dev), torch.from_numpy(cnt).to(dev)
    good = dict(rows=table.data_ptr(), B=4, Hmax=50, Wmax=150, boxes=tb.data_ptr(), layout=1, max_list=20, cnt=tc.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return _lib.lib().sy_redact(a["rows"], a["B"], a["Hmax"], a["Wmax"], a["boxes"], a["layout"], a["max_list"], a["cnt"],
                                    ops.stream_of(table))
    assert call() == 0
    for kw in (dict(rows=None), dict(boxes=None), dict(cnt=None), dict(B=0), dict(B=-1), dict(max_list=0), dict(max_list=-2),
               dict(Hmax=0), dict(Wmax=0), dict(Hmax=-3), dict(Wmax=-1), dict(layout=2), dict(layout=-1)):
        assert call(**kw) == 1, kw                                   # SY_ERR_ARG
    for kw in (dict(B=65536), dict(Hmax=32 * 65535 + 1)):
        assert call(**kw) == _lib.SY_ERR_UNSUPPORTED, kw
    assert C.sizeof(_lib.RedactRow) == _REDACT_DTYPE.itemsize == 88

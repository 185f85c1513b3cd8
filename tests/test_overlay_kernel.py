"""sy_overlay_draw (csrc/overlay.hip) on hand-made box lists, on the SIMT emulator and on the MI355X.

The yardstick is `restate` below: the seven-point rendering rule as include/streamyolo_hip.h states it, written over whole images
with plain loops — a painter working from the LAST list entry to the first, so that the lowest index ends on top — and knowing
nothing of tiles, workgroups or lists in LDS.  The comparison is byte-for-byte equality of the ENTIRE backing allocations
(np.array_equal on the raw buffers), which are pre-filled with a pseudo-random pattern: uncovered pixels, pitch padding, padded
luma rows and the gap between the planes are proven unwritten.

No tolerance: the rule is integer arithmetic behind one float division and one floor.  To make that a fair demand of fp32 every
case asserts on ITS OWN INPUTS, in float64, that each c / divisor + 0.5 and each 100 * score the launch looks at is at least 1e-3
away from an integer (and each score 1e-3 away from min_score).  Boxes are integers under the divisors 1, 0.5 and 0.25; the row
with the divisor 0.3 gets coordinates constructed to land a quarter pixel inside their cell."""
import ctypes as C

import numpy as np
import pytest
import torch

from streamyolo_amd import _lib, ops
from streamyolo_amd.data import FrameSurfacesU8, Surface
from streamyolo_amd.overlay import _OVERLAY_DTYPE, font_glyphs, palette_rows

MARGIN = 1e-3
TILE_H, TILE_W = ops.OVERLAY_TILE
BGR, RGB, NV12, P010 = _lib.PIX_BGR, _lib.PIX_RGB, _lib.PIX_NV12, _lib.PIX_P010
NAMES = ["CAR", "PERSON", "TRUCK_AB", ""]                           # 3, 6, 8 and 0 glyphs
COLOURS = [(250, 40, 30), (20, 30, 60), (200, 255, 180), (90, 200, 10)]      # (B, G, R): dark and bright ones (white / black text)
K = len(NAMES)
PALETTE = palette_rows(COLOURS)
TEXT = np.full((K, 8), 0xFF, dtype=np.uint8)
for _k, _n in enumerate(NAMES):
    TEXT[_k, :len(_n)] = [ord(c) - 32 for c in _n]
GLYPHS = font_glyphs()
MIN_SCORE = 0.3


# ---- the rule, restated from the header --------------------------------------------------------------------------------
def _round_px(c, divisor):
    """floor(c / divisor + 0.5) in fp32 -> int, or None when c or the sum is not finite."""
    with np.errstate(all="ignore"):
        v = np.float32(c) / np.float32(divisor) + np.float32(0.5)
    if not np.isfinite(np.float32(c)) or not np.isfinite(v):
        return None
    return int(min(max(np.floor(np.float64(v)), -2.0 ** 30), 2.0 ** 30))


def _label(text, cls, score, ident, flags, have_ids):
    codes = []
    for code in (text[cls] if cls is not None else []):              # the name: up to 8 codes, 0xFF ends it
        if code == 0xFF:
            break
        codes.append(int(code))
    if (flags & 1) and have_ids:
        codes += [0] + [ord(ch) - 32 for ch in str(int(ident) % 100000)]
    elif flags & 2:
        with np.errstate(all="ignore"):
            v = min(max(int(np.float32(100.0) * np.float32(score)), 0), 99)
        codes += [0] + [ord(ch) - 32 for ch in "%02d%%" % v]
    return codes


def restate(row, bufs, boxes, layout, ids, cnt, max_list, tables=None):
    """Apply the rule for one table row to `bufs` (numpy copies of the backing allocations), in place.  row: the descriptor's
    fields as a dict — fmt, hs, ws, pitch, cpitch (0: the pitch), p0 = (buffer, offset) or None, p1 = (buffer, offset) or None
    (behind the luma rows), divisor, min_score, max_boxes, thickness, text_scale, flags.  tables: (palette [K, 8], class_text
    [K, 8]) of another style than this file's."""
    PALETTE, TEXT = tables if tables is not None else (globals()["PALETTE"], globals()["TEXT"])
    K = len(PALETTE)
    hs, ws, fmt = row["hs"], row["ws"], row["fmt"]
    if row["p0"] is None or hs <= 0 or ws <= 0 or fmt not in (BGR, RGB, NV12, P010):
        return
    yuv = fmt in (NV12, P010)
    row_bytes = ws * (1 if fmt == NV12 else 2 if fmt == P010 else 3)
    cpitch = row["cpitch"] if row["cpitch"] != 0 else row["pitch"]
    if row["pitch"] < row_bytes or (yuv and (hs % 2 or ws % 2 or row["cpitch"] < 0 or cpitch < row_bytes)):
        return                                                       # a descriptor no surface can have: skipped
    t, s = min(max(row["thickness"], 1), 16), min(max(row["text_scale"], 0), 4)
    n = min(max(int(cnt), 0), max_list, 256)
    if row["max_boxes"] > 0:
        n = min(n, row["max_boxes"])
    who = -np.ones((hs, ws), dtype=np.int64)                         # covering list index per pixel
    glyph = np.zeros((hs, ws), dtype=bool)
    cls_of = {}
    for k in range(n - 1, -1, -1):                                   # the painter: last entry first, entry 0 ends on top
        r = boxes[k]
        score = np.float32(r[4]) * np.float32(r[5]) if layout == 0 else np.float32(r[4])
        cls_f = r[6] if layout == 0 else r[5]
        px = [_round_px(r[i], row["divisor"]) for i in range(4)]
        if any(p is None for p in px) or not score >= np.float32(row["min_score"]):
            continue
        X1, Y1, X2, Y2 = px[0], px[1], px[2] - 1, px[3] - 1
        if X2 < X1 or Y2 < Y1:
            continue
        cls = int(cls_f) if 0 <= cls_f < K else None
        cls_of[k] = 0 if cls is None else cls
        ya, yb, xa, xb = max(Y1, 0), min(Y2, hs - 1), max(X1, 0), min(X2, ws - 1)
        if ya <= yb and xa <= xb:                                    # 2. outline: the rectangle's pixels outside the inner one
            yy, xx = np.mgrid[ya:yb + 1, xa:xb + 1]
            ring = ~((xx >= X1 + t) & (xx <= X2 - t) & (yy >= Y1 + t) & (yy <= Y2 - t))
            who[ya:yb + 1, xa:xb + 1][ring] = k
            glyph[ya:yb + 1, xa:xb + 1][ring] = False
        if s > 0:                                                    # 3. label tab: over this box's own outline
            codes = _label(TEXT, cls, score, None if ids is None else ids[k], row["flags"], ids is not None)
            top = Y1 if Y1 - 8 * s < 0 else Y1 - 8 * s
            for y in range(max(top, 0), min(top + 8 * s, hs)):
                for x in range(max(X1, 0), min(X1 + 8 * s * len(codes), ws)):
                    fx, fy = (x - X1) // s, (y - top) // s
                    code = codes[fx // 8]
                    bit = (GLYPHS[code, fy] >> (7 - fx % 8)) & 1 if code < 64 else 0
                    who[y, x], glyph[y, x] = k, bool(bit)
    b0, o0 = row["p0"]
    if fmt in (BGR, RGB):
        for y in range(hs):
            for x in range(ws):
                k = who[y, x]
                if k < 0:
                    continue
                pal = PALETTE[cls_of[k]]
                v = [pal[3]] * 3 if glyph[y, x] else ([pal[0], pal[1], pal[2]] if fmt == BGR else [pal[2], pal[1], pal[0]])
                at = o0 + y * row["pitch"] + 3 * x
                bufs[b0][at:at + 3] = v
        return
    step = 2 if fmt == P010 else 1
    b1, o1 = row["p1"] if row["p1"] is not None else (b0, o0 + row["pitch"] * hs)
    for y in range(hs):
        for x in range(ws):
            k = who[y, x]
            if k >= 0:
                pal = PALETTE[cls_of[k]]
                at = o0 + y * row["pitch"] + step * x
                bufs[b0][at:at + step] = [pal[7] if glyph[y, x] else pal[4]] if step == 1 else [0, pal[7] if glyph[y, x] else pal[4]]
    for y in range(0, hs, 2):                                        # 6. one (U, V) per 2 x 2 block: the first covered pixel's
        for x in range(0, ws, 2):
            for yy, xx in ((y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)):
                k = who[yy, xx]
                if k >= 0:
                    pal = PALETTE[cls_of[k]]
                    u, v = (128, 128) if glyph[yy, xx] else (pal[5], pal[6])
                    at = o1 + (y // 2) * cpitch + step * x
                    bufs[b1][at:at + 2 * step] = [u, v] if step == 1 else [0, u, 0, v]
                    break


def assert_fair(rows, boxes, layout, cnt, max_list):
    """The condition on a case's OWN INPUTS under which fp32 must reproduce the rule exactly (float64)."""
    for b, row in enumerate(rows):
        n = min(max(int(cnt[b]), 0), max_list, 256)
        for r in boxes[b, :n]:
            for c in r[:4]:
                if np.isfinite(c):
                    v = np.float64(np.float32(c)) / np.float64(np.float32(row["divisor"])) + 0.5
                    assert abs(v - np.round(v)) >= MARGIN, (b, c, v)
            sc = np.float64(np.float32(r[4])) * np.float64(np.float32(r[5])) if layout == 0 else np.float64(np.float32(r[4]))
            if np.isfinite(sc):
                assert abs(100.0 * sc - np.round(100.0 * sc)) >= MARGIN, (b, sc)
                assert abs(sc - np.float64(np.float32(row["min_score"]))) >= MARGIN, (b, sc)


# ---- surfaces and lists ----------------------------------------------------------------------------------------------
def make_rows(rng):
    """The four formats of one launch and a row without a surface.  -> (rows, buffer sizes)."""
    style = dict(min_score=MIN_SCORE, max_boxes=0)
    sizes = [70 * (3 * 134 + 10) + 7,                                # 0: BGR, pitch 3 Ws + 10 (and a tail behind the last row)
             46 * 3 * 90,                                            # 1: RGB, dense
             72 * 140, 35 * 160 + 5,                                 # 2, 3: NV12 luma padded to 72 rows (pitch 140); chroma on its own, pitch 160
             (38 + 19) * 136 + 3]                                    # 4: P010 in one allocation, pitch 2 Ws + 4, chroma at row Hs
    rows = [
        dict(fmt=BGR, hs=70, ws=134, pitch=3 * 134 + 10, cpitch=0, p0=(0, 0), p1=None, divisor=0.25, thickness=3, text_scale=1, flags=1, q=4, **style),
        dict(fmt=RGB, hs=46, ws=90, pitch=3 * 90, cpitch=0, p0=(1, 0), p1=None, divisor=0.5, thickness=1, text_scale=2, flags=2, q=2, **style),
        dict(fmt=NV12, hs=70, ws=134, pitch=140, cpitch=160, p0=(2, 0), p1=(3, 0), divisor=1.0, thickness=3, text_scale=2, flags=1, q=1, **style),
        dict(fmt=P010, hs=38, ws=66, pitch=136, cpitch=0, p0=(4, 0), p1=None, divisor=0.3, thickness=1, text_scale=1, flags=2, q=1, **style),
        dict(fmt=BGR, hs=70, ws=134, pitch=3 * 134, cpitch=0, p0=None, p1=None, divisor=1.0, thickness=2, text_scale=1, flags=0, q=1, **style),
    ]
    return rows, sizes


def pixel_boxes(hs, ws, q):
    """Twelve boxes in SURFACE pixels, (x1, y1, x2, y2) covering [x1, x2) x [y1, y2), all multiples of the row's quantum q (what an
    integer box gives under its divisor); rows with q = 1 move some corners to odd pixels.  -> list of (box, class, id)."""
    o = 1 if q == 1 else 0
    nar = max(q, 1)
    ws, hs = ws // q * q, hs // q * q                                # (the edges are crossed all the same)
    return [
        ((-8, 20, 12, 36), 9, 3),                                    # 0 crosses the left edge; a class id >= num_classes
        ((20, -4, 60, 12), 1, 17),                                   # 1 crosses the top edge: Y1 < 0, the tab goes inside, clipped
        ((ws - 8, 4, ws + 8, 28), 0, 5),                             # 2 crosses the right edge; Y1 < 8 s: tab inside, off the right edge
        ((16 + o, hs - 8 + o, 56, hs + 8), 2, 123456),               # 3 crosses the bottom edge; an id >= 100000; odd corner
        ((ws + 8, hs + 8, ws + 24, hs + 24), 0, 6),                  # 4 wholly outside
        ((40, 8, 32, 20), 1, 7),                                     # 5 x2 < x1
        ((np.nan, 8, 48, 24), 1, 8),                                 # 6 a NaN coordinate
        ((4 + o, 40 + o, 4 + o + nar, 64), 3, 9),                    # 7 narrower than 2 t (q = 1: one pixel wide, odd); a nameless class
        ((TILE_W, TILE_H, TILE_W + 36, TILE_H + 24), 0, 10),         # 8 starts on the FIRST column / row of a tile ...
        ((TILE_W + 8 + o, TILE_H + o, TILE_W + 48, TILE_H + 20), 2, 11),      # 9 ... and is overlapped, tab and all, by another class
        ((TILE_W - 24, 4, TILE_W, TILE_H), 1, 99999),                # 10 ends on the LAST column / row of a tile
        ((8, 40, 40, 60), 0, 12),                                    # 11 plainly visible, but its score is below min_score
    ]


SCORES = [0.957 - 0.0531 * k for k in range(11)] + [0.2137]


def make_lists(rows, layout, max_list=16):
    """boxes [B, max_list, 7 | 6] fp32, ids [B, max_list] int32, cnt [B] for the rows' own box sets (entries beyond: zeros)."""
    B = len(rows)
    boxes = np.zeros((B, max_list, 7 if layout == 0 else 6), dtype=np.float32)
    ids = np.zeros((B, max_list), dtype=np.int32)
    for b, row in enumerate(rows):
        for k, (px, cls, ident) in enumerate(pixel_boxes(row["hs"], row["ws"], row["q"])):
            d = row["divisor"]
            if d in (1.0, 0.5, 0.25):
                c = [p * d for p in px]                              # integer boxes
                assert all(np.isnan(v) or v == int(v) for v in c)
            else:                                                    # constructed: c / d + 0.5 lands a quarter pixel above p + 0.5
                c = [np.float32(d * (p + 0.25)) for p in px]
            boxes[b, k, :4] = c
            if layout == 0:
                boxes[b, k, 4:] = (0.9, SCORES[k] / 0.9, cls)
            else:
                boxes[b, k, 4:] = (SCORES[k], cls)
            ids[b, k] = ident
    return boxes, ids, np.full(B, 12, dtype=np.int32)


def table_of(rows, tensors):
    t = np.zeros(len(rows), dtype=_OVERLAY_DTYPE)
    for b, r in enumerate(rows):
        p0 = 0 if r["p0"] is None else tensors[r["p0"][0]].data_ptr() + r["p0"][1]
        p1 = 0 if r["p1"] is None else tensors[r["p1"][0]].data_ptr() + r["p1"][1]
        t[b] = (p0, p1, r["hs"], r["ws"], r["pitch"], r["cpitch"], r["fmt"], r["divisor"], r["min_score"], r["max_boxes"],
                r["thickness"], r["text_scale"], r["flags"], 0)
    return t


def dev_tables(dev):
    return tuple(torch.from_numpy(a.copy()).to(dev) for a in (PALETTE, TEXT, GLYPHS))


def run_case(dev, rows, sizes, boxes, layout, ids, cnt, max_hw, seed=0):
    """Launch over pseudo-random backing buffers and compare every byte of them with the restatement."""
    max_list = boxes.shape[1]
    assert_fair(rows, boxes, layout, cnt, max_list)
    rng = np.random.RandomState(seed)
    host = [rng.randint(0, 256, size=n).astype(np.uint8) for n in sizes]
    tensors = [torch.from_numpy(h.copy()).to(dev) for h in host]
    table = torch.from_numpy(table_of(rows, tensors).view(np.uint8).copy()).to(dev)
    pal, text, glyphs = dev_tables(dev)
    t_boxes, t_cnt = torch.from_numpy(boxes).to(dev), torch.from_numpy(cnt).to(dev)
    t_ids = None if ids is None else torch.from_numpy(ids).to(dev)
    ops.overlay_draw(table, len(rows), max_hw, t_boxes, layout, t_ids, t_cnt, pal, text, glyphs)
    want = [h.copy() for h in host]
    for b, row in enumerate(rows):
        restate(row, want, boxes[b], layout, None if ids is None else ids[b], cnt[b], max_list)
    drawn = 0
    for h, w, t in zip(host, want, tensors):
        got = t.cpu().numpy()
        assert np.array_equal(got, w), "%d bytes differ" % int((got != w).sum())
        drawn += int((w != h).sum())
    return drawn, tensors


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,with_ids", [(0, False), (1, True), (1, False)])
def test_four_formats_one_launch(backend, layout, with_ids):
    """B = 5 rows (BGR with a pitch, dense RGB, split-plane NV12 with a padded luma, single-buffer P010, no surface) of different
    sizes, styles and divisors; twelve boxes per row covering every branch of the rule.  ids = NULL with flags bit 0: no id."""
    rows, sizes = make_rows(None)
    boxes, ids, cnt = make_lists(rows, layout)
    drawn, _ = run_case(backend, rows, sizes, boxes, layout, ids if with_ids else None, cnt, (72, 136))
    assert drawn > 1000                                              # (the case does draw: four surfaces with outlines and tabs)


def test_counts_caps_and_styles(backend):
    """cnt = 0; cnt above max_boxes; cnt above max_list; text scale 0; the other thickness per format; clamped style fields."""
    rows, sizes = make_rows(None)
    boxes, ids, cnt = make_lists(rows, 1)
    rows[0].update(thickness=1, text_scale=0)                        # no tab at all
    rows[1].update(thickness=3, text_scale=1, max_boxes=5, flags=1)  # cnt 12 > max_boxes 5: boxes 5.. are not looked at
    rows[2].update(thickness=40, text_scale=9, flags=2)              # clamped to 16 and 4
    rows[3].update(thickness=3, text_scale=2, flags=3)               # both bits: the id wins
    cnt[:] = (12, 12, 100, 0, 12)                                    # 100 > max_list 16: the empty entries behind the 12 are looked at
    boxes[:, 12:, 4] = 0.0137
    rows[4].update(p0=(0, 0), hs=0)                                  # Hs == 0: nothing is drawn
    drawn, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (72, 136), seed=1)
    assert drawn > 1000
    rows2, _ = make_rows(None)
    drawn, _ = run_case(backend, rows2, sizes, boxes, 1, ids, np.array([0, -3, 0, 0, 0], dtype=np.int32), (72, 136), seed=2)
    assert drawn == 0


def test_descriptors_no_surface_can_have(backend):
    """An unknown format, odd NV12 / P010 sizes, a pitch below the row's bytes, a negative chroma pitch: skipped, nothing written."""
    rows, sizes = make_rows(None)
    boxes, ids, cnt = make_lists(rows, 1)
    rows[4] = dict(rows[2], cpitch=133)                              # a chroma pitch below Ws
    rows[0].update(fmt=7)
    rows[1].update(pitch=3 * 90 - 1)
    rows[2].update(hs=69)
    rows[3].update(p1=(4, 38 * 136), cpitch=-136)
    drawn, _ = run_case(backend, rows, sizes, boxes, 1, ids, cnt, (72, 136), seed=3)
    assert drawn == 0
    rows, _ = make_rows(None)
    rows[2].update(ws=133)                                           # an odd width; a luma pitch below 2 Ws
    rows[3].update(pitch=2 * 66 - 2)
    drawn, _ = run_case(backend, rows[2:4], sizes, boxes[2:4].copy(), 1, ids[2:4].copy(), cnt[2:4].copy(), (72, 136), seed=4)
    assert drawn == 0


def test_full_list_of_256(backend):
    """cnt = 256 on a 64 x 64 BGR frame fills the LDS list: every thread of a workgroup resolves a box, every wave compacts."""
    rng = np.random.RandomState(5)
    row = dict(fmt=BGR, hs=64, ws=64, pitch=192, cpitch=0, p0=(0, 0), p1=None, divisor=1.0, thickness=1, text_scale=1, flags=1,
               min_score=MIN_SCORE, max_boxes=0)
    boxes = np.zeros((1, 300, 6), dtype=np.float32)
    x1, y1 = rng.randint(-4, 60, size=300), rng.randint(-4, 60, size=300)
    boxes[0, :, 0], boxes[0, :, 1] = x1, y1
    boxes[0, :, 2], boxes[0, :, 3] = x1 + rng.randint(1, 24, size=300), y1 + rng.randint(1, 24, size=300)
    boxes[0, :, 4] = np.where(np.arange(300) % 7 == 3, 0.1234, (9137.5 - 11 * np.arange(300)) / 10000)      # 100 s = xx.xx5
    boxes[0, :, 5] = rng.randint(0, K + 1, size=300)
    ids = rng.randint(0, 300000, size=(1, 300)).astype(np.int32)
    cnt = np.array([300], dtype=np.int32)                            # the launch looks at 256
    drawn, _ = run_case(backend, [row], [64 * 192], boxes, 1, ids, cnt, (64, 64), seed=6)
    assert drawn > 3000
    # entry 255 is looked at, entry 256 is not: alone on a clean frame
    lone = np.zeros_like(boxes)
    lone[0, :, 4] = 0.0137
    lone[0, 255] = (8, 24, 40, 56, 0.9137, 1)
    lone[0, 256] = (44, 4, 60, 20, 0.9137, 2)
    drawn, tensors = run_case(backend, [row], [64 * 192], lone, 1, ids, cnt, (64, 64), seed=7)
    assert drawn > 0


def test_p010_round_trip(backend):
    """A P010 surface drawn on and read back through sy_frames_u8_pack_surfaces' high-byte rule is the NV12 surface of the high
    bytes drawn with the same lists."""
    dev = backend
    hs, ws = 38, 66
    rng = np.random.RandomState(11)
    words = rng.randint(0, 256, size=(hs + hs // 2, ws, 2)).astype(np.uint8)       # (low byte, high byte) per sample
    p010 = torch.from_numpy(words.reshape(hs + hs // 2, 2 * ws).copy()).to(dev)
    nv12 = torch.from_numpy(words[:, :, 1].copy()).to(dev)
    common = dict(hs=hs, ws=ws, divisor=1.0, thickness=2, text_scale=1, flags=1, min_score=MIN_SCORE, max_boxes=0, q=1)
    rows = [dict(common, fmt=P010, pitch=2 * ws, cpitch=2 * ws, p0=(0, 0), p1=(0, hs * 2 * ws)),
            dict(common, fmt=NV12, pitch=ws, cpitch=ws, p0=(1, 0), p1=(1, hs * ws))]
    boxes, ids, cnt = make_lists(rows, 1)
    table = torch.from_numpy(table_of(rows, [p010, nv12]).view(np.uint8).copy()).to(dev)
    pal, text, glyphs = dev_tables(dev)
    before = nv12.clone()
    ops.overlay_draw(table, 2, (hs, ws), torch.from_numpy(boxes).to(dev), 1, torch.from_numpy(ids).to(dev), torch.from_numpy(cnt).to(dev),
                     pal, text, glyphs)
    assert not torch.equal(before, nv12)
    src = FrameSurfacesU8(2, (hs, ws), (hs, ws), dev)
    src.set_row(0, Surface((p010[:hs], p010[hs:]), "p010"))
    src.set_row(1, Surface((nv12[:hs], nv12[hs:]), "nv12"))
    src.upload()
    out = src.to_nchw()
    assert torch.equal(out[0], out[1])
    assert torch.equal(p010.view(hs + hs // 2, ws, 2)[:, :, 1], nv12)


def test_status_codes(backend):
    dev = backend
    rows, sizes = make_rows(None)
    boxes, ids, cnt = make_lists(rows, 1)
    tensors = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in sizes]
    table = torch.from_numpy(table_of(rows, tensors).view(np.uint8).copy()).to(dev)
    pal, text, glyphs = dev_tables(dev)
    tb, ti, tc = torch.from_numpy(boxes).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(cnt).to(dev)
    good = dict(rows=table.data_ptr(), B=5, Hmax=72, Wmax=136, boxes=tb.data_ptr(), layout=1, max_list=16, ids=ti.data_ptr(),
                cnt=tc.data_ptr(), palette=pal.data_ptr(), class_text=text.data_ptr(), num_classes=K, glyphs=glyphs.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return _lib.lib().sy_overlay_draw(a["rows"], a["B"], a["Hmax"], a["Wmax"], a["boxes"], a["layout"], a["max_list"], a["ids"],
                                          a["cnt"], a["palette"], a["class_text"], a["num_classes"], a["glyphs"], ops.stream_of(table))
    assert call() == 0
    assert call(ids=None) == 0 and call(class_text=None) == 0
    for kw in (dict(rows=None), dict(boxes=None), dict(cnt=None), dict(palette=None), dict(glyphs=None), dict(B=0), dict(B=-1),
               dict(max_list=0), dict(num_classes=0), dict(layout=2), dict(layout=-1), dict(Hmax=0), dict(Wmax=0)):
        assert call(**kw) == 1, kw                                   # SY_ERR_ARG
    assert call(num_classes=129) == _lib.SY_ERR_UNSUPPORTED
    assert call(B=65536) == _lib.SY_ERR_UNSUPPORTED
    assert C.sizeof(_lib.OverlayRow) == _OVERLAY_DTYPE.itemsize == 64

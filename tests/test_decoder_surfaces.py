"""Decoder surfaces read in place: split-plane NV12 and P010 rows (sy_frames_u8_pack_surfaces, sy_frame_surf, data.Surface,
data.FrameSurfacesU8, MultiStreamDetector(surfaces=True); csrc/input_pipeline.hip).

The contract is bit equality with the existing path on the REPACKED frame (dense planes, one pitch, chroma at row Hs) — so the
yardstick throughout is torch.equal against FrameRowsU8 / sy_frames_u8_pack_rows, whose own bits tests/test_pixel_formats.py
pins; there is no tolerance to choose.  P010's definition (the 8-bit sample is the 16-bit word's high byte) is restated here in
numpy: words >> 8."""
import numpy as np
import pytest
import torch

from streamyolo_amd import _lib, ops
from streamyolo_amd import streaming as S
from streamyolo_amd.data import FramePairsU8, FrameRowsU8, FrameSurfacesU8, Surface
from streamyolo_amd.ops import View
from test_pixel_formats import GEOMS, _models, _nv12, _pack_all, _same_all, _t, nv12_to_bgr

CANVAS = (32, 64)
MAX_HW = (64, 128)
OUT_SIZES = [(32, 64), (16, 32)]
GEOM_IDS = ["%dx%d_d%d" % g[:3] for g in GEOMS]
assert GEOMS == [(32, 64, 1, 0), (64, 128, 2, 0), (40, 72, 0, 0), (50, 20, 0, 0), (34, 70, -1, 1), (64, 126, 2, 0), (32, 62, 1, 0)]


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _noise(seed, shape, backend):
    return _t(np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8), backend)


def _staged(frame, geom, out_size, backend, fmt="nv12"):
    """The yardstick: the dense frame through FrameRowsU8 (sy_frames_u8_pack_rows) -> NCHW fp32, Focus fp32 / fp16 / bf16."""
    _, _, dec, mir = geom
    rows = FrameRowsU8(1, MAX_HW, CANVAS, backend, out_size=out_size)
    rows.set_row(0, frame, mirror=bool(mir), decimate=dec, divisor=1.0, pixel_format=fmt)
    rows.upload()
    return _pack_all(rows, out_size)


def _in_place(surface, geom, out_size, backend):
    _, _, dec, mir = geom
    rows = FrameSurfacesU8(1, MAX_HW, CANVAS, backend, out_size=out_size)
    arena = rows.arena.clone()
    rows.set_row(0, surface, mirror=bool(mir), decimate=dec, divisor=1.0)
    rows.upload()
    res = _pack_all(rows, out_size)
    assert torch.equal(rows.arena, arena)
    return res


def _nv12_surface(nv, layout, backend, pad_seed=0, step=1):
    """The NV12 frame `nv` [Hs*3/2, row bytes] (P010: step = 2, row bytes = 2 Ws) laid out as a decoder might, every byte outside
    the planes' own rows and columns random (pad_seed):
      a  one buffer, pitch = row bytes + 6, chroma at row Hs + 8 (1080 -> 1088 in small)
      b  one buffer, pitch = row bytes rounded up to 256, chroma at row Hs + 16: both planes aligned (the fast path)
      c  chroma in an allocation of its own with another pitch
      d  luma 4-byte aligned with a pitch that is a multiple of 4, the chroma plane at an ODD address
    -> (Surface, the tensors it views)"""
    rows, rb = nv.shape
    hs, ws, fmt = rows // 3 * 2, rb // step, "nv12" if step == 1 else "p010"
    y, uv = _t(nv[:hs], backend), _t(nv[hs:], backend)
    if layout in ("a", "b"):
        pitch, c0 = (rb + 6, hs + 8) if layout == "a" else ((rb + 255) // 256 * 256, hs + 16)
        buf = _noise(pad_seed, (c0 + hs // 2 + 3, pitch), backend)
        buf[:hs, :rb].copy_(y)
        buf[c0:c0 + hs // 2, :rb].copy_(uv)
        s = Surface.from_buffer(buf, hs, ws, fmt, chroma_row=c0)
        assert s.pitch == s.chroma_pitch == pitch and s.planes[1].data_ptr() == buf.data_ptr() + c0 * pitch
        if layout == "b":
            assert all(p.data_ptr() % 4 == 0 for p in s.planes) and pitch % 4 == 0
        return s, (buf,)
    if layout == "c":
        lum, chr_ = _noise(pad_seed, (hs, rb + 6), backend), _noise(pad_seed + 1, (hs // 2, rb + 10), backend)
        lum[:, :rb].copy_(y)
        chr_[:, :rb].copy_(uv)
        s = Surface((lum[:, :rb], chr_[:, :rb]), fmt)
        assert (s.pitch, s.chroma_pitch) == (rb + 6, rb + 10)
        return s, (lum, chr_)
    assert layout == "d"
    pitch = (rb + 3) // 4 * 4 + 4
    lum, flat = _noise(pad_seed, (hs, pitch), backend), _noise(pad_seed + 1, (1 + (hs // 2) * pitch,), backend)
    lum[:, :rb].copy_(y)
    chroma = flat[1:].as_strided((hs // 2, rb), (pitch, 1))
    chroma.copy_(uv)
    s = Surface((lum[:, :rb], chroma), fmt)
    assert s.planes[0].data_ptr() % 4 == 0 and s.pitch % 4 == 0 and s.chroma_pitch % 4 == 0 and s.planes[1].data_ptr() % 2 == 1
    return s, (lum, flat)


def _p010_words(nv, seed):
    """NV12 bytes -> little-endian P010 words as bytes [rows, 2 Ws]: the sample in the HIGH byte, the low byte random (so the six
    unused bits and the two truncated bits are non-zero)."""
    low = np.random.RandomState(seed).randint(0, 256, nv.shape).astype(np.uint16)
    words = (nv.astype(np.uint16) << 8) | low
    assert (low & 0x3f).any() and (low & 0xc0).any() and np.array_equal((words >> 8).astype(np.uint8), nv)
    return words.astype("<u2").view(np.uint8).reshape(nv.shape[0], 2 * nv.shape[1])


# ---- 1: split-plane NV12 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", OUT_SIZES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_split_plane_nv12_equals_the_repacked_frame(backend, geom, out_size):
    """Layouts a - d of one random NV12 frame == sy_frames_u8_pack_rows on the frame repacked densely, in every output; layout b
    qualifies for the wide-load fast path, layout d would if the luma plane alone decided."""
    hs, ws = geom[:2]
    nv = _nv12(hs * 1000 + ws, hs, ws)
    want = _staged(nv, geom, out_size, backend)
    assert not torch.equal(want[0], torch.full_like(want[0], 114.0))
    for layout in "abcd":
        s, _ = _nv12_surface(nv, layout, backend, pad_seed=7)
        assert s.hw == (hs, ws) and s.pixel_format == "nv12"
        _same_all(_in_place(s, geom, out_size, backend), want, layout)


# ---- 2: padding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", OUT_SIZES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_padding_is_never_read(backend, geom, out_size):
    """Layouts a and c built twice with different random bytes everywhere outside the planes' Ws columns and between the planes:
    identical outputs (the planes themselves hold the same random bytes)."""
    hs, ws = geom[:2]
    nv = _nv12(hs * 1000 + ws + 1, hs, ws)
    for layout in "ac":
        (s1, keep1), (s2, keep2) = _nv12_surface(nv, layout, backend, pad_seed=11), _nv12_surface(nv, layout, backend, pad_seed=23)
        assert any(not torch.equal(a, b) for a, b in zip(keep1, keep2))
        assert all(torch.equal(a, b) for a, b in zip(s1.planes, s2.planes))
        _same_all(_in_place(s1, geom, out_size, backend), _in_place(s2, geom, out_size, backend), layout)


# ---- 3: P010 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", OUT_SIZES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_p010_equals_nv12_on_the_high_bytes(backend, geom, out_size):
    """P010 words with random low bytes, pitch 2 Ws + 10 with a padded luma height (byte views) and a detached chroma plane (16-bit
    tensors) == the NV12 path on words >> 8; other low bytes: the same output."""
    hs, ws = geom[:2]
    nv = _nv12(hs * 1000 + ws + 2, hs, ws)
    want = _staged(nv, geom, out_size, backend)
    w1, w2 = _p010_words(nv, 1), _p010_words(nv, 2)
    assert not np.array_equal(w1, w2)
    pitch = 2 * ws + 10
    for w in (w1, w2):
        buf = _noise(5, (hs + 4 + hs // 2, pitch), backend)
        buf[:hs, :2 * ws].copy_(_t(w[:hs], backend))
        buf[hs + 4:, :2 * ws].copy_(_t(w[hs:], backend))
        s = Surface.from_buffer(buf, hs, ws, "p010", chroma_row=hs + 4)
        assert s.hw == (hs, ws) and s.pitch == s.chroma_pitch == pitch and s.format == _lib.PIX_P010
        _same_all(_in_place(s, geom, out_size, backend), want, "pitch 2 Ws + 10")
    # 16-bit tensors, the chroma plane an allocation of its own with a pitch of its own
    lum = torch.from_numpy(np.ascontiguousarray(w1[:hs]).view("<i2").copy()).to(backend)
    chroma = torch.zeros((hs // 2, ws + 3), dtype=torch.int16, device=backend)
    chroma[:, :ws].copy_(torch.from_numpy(np.ascontiguousarray(w1[hs:]).view("<i2").copy()))
    s = Surface((lum, chroma[:, :ws]), "p010")
    assert lum.dtype == torch.int16 and s.hw == (hs, ws) and (s.pitch, s.chroma_pitch) == (2 * ws, 2 * ws + 6)
    assert s.planes[0].data_ptr() == lum.data_ptr() and s.planes[1].data_ptr() == chroma.data_ptr()
    _same_all(_in_place(s, geom, out_size, backend), want, "detached")
    for layout in "cd":
        s, _ = _nv12_surface(w2, layout, backend, pad_seed=9, step=2)
        _same_all(_in_place(s, geom, out_size, backend), want, layout)


def test_p010_lattice_is_the_published_fixed_point(backend):
    """The 256-luma x 7x7-chroma lattice of test_nv12_conversion_is_the_published_fixed_point in the high bytes of P010 words whose
    low bytes are random: exactly the int64 statement of the NV12 formula, and what the NV12 entry point writes."""
    lat = [0, 16, 64, 128, 192, 240, 255]
    pairs = [(u, v) for u in lat for v in lat]
    hs, ws = 2 * len(pairs), 256
    nv = np.zeros((hs * 3 // 2, ws), dtype=np.uint8)
    nv[:hs] = np.arange(256, dtype=np.uint8)[None, :]
    for r, (u, v) in enumerate(pairs):
        nv[hs + r, 0::2], nv[hs + r, 1::2] = u, v
    want = torch.from_numpy(nv12_to_bgr(nv)).permute(2, 0, 1).float().unsqueeze(0)
    assert torch.equal(FramePairsU8(_t(nv[None], backend), None, (hs, ws), 1, pixel_format="nv12").to_nchw().cpu(), want)
    words = _t(_p010_words(nv, 3), backend)
    rows = FrameSurfacesU8(1, (hs, ws), (hs, ws), backend)
    rows.set_row(0, Surface((words[:hs], words[hs:]), "p010"))
    rows.upload()
    assert torch.equal(rows.to_nchw().cpu(), want)


# ---- 4: BGR / RGB -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", OUT_SIZES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_bgr_and_rgb_surfaces_with_a_pitch(backend, geom, out_size):
    """Pitch 3 Ws + 5 (a byte buffer) and a column slice of a wider [Hs, Ws + 4, 3] tensor == the dense frame."""
    hs, ws = geom[:2]
    frame = np.random.RandomState(hs + ws).randint(0, 256, (hs, ws, 3)).astype(np.uint8)
    for fmt in ("bgr", "rgb"):
        want = _staged(frame, geom, out_size, backend, fmt)
        buf = _noise(3, (hs + 1, 3 * ws + 5), backend)
        buf[:hs, :3 * ws].copy_(_t(frame.reshape(hs, 3 * ws), backend))
        s = Surface.from_buffer(buf, hs, ws, fmt)
        assert s.pitch == 3 * ws + 5 and s.hw == (hs, ws) and tuple(s.planes[0].shape) == (hs, ws, 3)
        _same_all(_in_place(s, geom, out_size, backend), want, (fmt, "pitch"))
        wide = _noise(4, (hs, ws + 4, 3), backend)
        wide[:, 2:2 + ws].copy_(_t(frame, backend))
        s = Surface(wide[:, 2:2 + ws], fmt)
        assert s.pitch == 3 * (ws + 4) and s.planes[0].data_ptr() == wide.data_ptr() + 6
        _same_all(_in_place(s, geom, out_size, backend), want, (fmt, "slice"))
    assert not torch.equal(want[0], _staged(frame, geom, out_size, backend, "bgr")[0])           # (the order matters)


# ---- 5: one launch ----------------------------------------------------------------------------------------------------------------
# (kind, Hs, Ws, decimate, mirror) of the six rows
M_ROWS = [("nv12_surface", 64, 128, 2, 0),
          ("p010_surface", 40, 72, 0, 1),
          ("bgr_staged", 50, 20, 0, 0),
          ("rgb_surface", 34, 70, -1, 0),
          ("empty", 0, 0, 1, 0),
          ("nv12_staged", 32, 64, 1, 1)]


@pytest.mark.parametrize("out_size", OUT_SIZES)
def test_rows_of_every_kind_share_one_launch(backend, out_size):
    """Batch 6: an NV12 surface of layout a, a P010 surface, a staged BGR frame, an RGB surface, an empty row and a staged NV12
    frame in ONE sy_frames_u8_pack_surfaces launch, every row == its single-frame result; refilled in another order the launch has
    the identical C-ABI arguments (all but the freshly allocated output) and the rows follow."""
    rng = np.random.RandomState(5)
    dense, given = [], []
    for k, (kind, hs, ws, _, _) in enumerate(M_ROWS):
        if kind == "empty":
            dense.append(None); given.append(None)
        elif kind.startswith("nv12") or kind.startswith("p010"):
            nv = _nv12(80 + k, hs, ws)
            dense.append(nv)
            given.append(nv if kind == "nv12_staged" else
                         _nv12_surface(nv, "a", backend, pad_seed=k)[0] if kind == "nv12_surface" else
                         _nv12_surface(_p010_words(nv, k), "c", backend, pad_seed=k, step=2)[0])
        else:
            f = rng.randint(0, 256, (hs, ws, 3)).astype(np.uint8)
            dense.append(f)
            wide = _noise(k, (hs, ws + 2, 3), backend)
            wide[:, 1:1 + ws].copy_(_t(f, backend))
            given.append(f if kind == "bgr_staged" else Surface(wide[:, 1:1 + ws], "rgb"))
    B = len(M_ROWS)
    rows = FrameSurfacesU8(B, MAX_HW, CANVAS, backend, out_size=out_size)

    def fill(order):
        for b, k in enumerate(order):
            kind, _, _, dec, mir = M_ROWS[k]
            if given[k] is None:
                rows.set_row(b, None)
            else:
                rows.set_row(b, given[k], mirror=bool(mir), decimate=dec, divisor=1.0,
                             pixel_format=None if isinstance(given[k], Surface) else kind[:-7])
        rows.upload()

    def launch():
        with _lib.record() as calls:
            nchw = rows.to_nchw()
        res = [nchw]
        for dt in ("fp32", "fp16", "bf16"):
            v = View.alloc(B, out_size[0] // 2, out_size[1] // 2, 16, dt, backend)
            rows.pack_focus(v)
            res.append(v.buf.reshape(B, -1, 16).clone())
        return calls, res
    order = list(range(B))
    fill(order)
    assert [int(f) for f in rows._rows["format"]] == [2, 3, 0, 1, 0, 2]
    first_calls, got = launch()
    for k, (kind, hs, ws, dec, mir) in enumerate(M_ROWS):
        for lay in range(4):
            if dense[k] is None:
                want = torch.full_like(got[lay][k], 114.0)
                if lay:
                    want[..., 12:] = 0
            else:
                fmt = "nv12" if kind[:4] in ("nv12", "p010") else kind[:3]
                want = _staged(dense[k], (hs, ws, dec, mir), out_size, backend, fmt)[lay]
            assert torch.equal(got[lay][k].reshape(-1), want.reshape(-1)), (kind, lay)
    perm = [5, 3, 4, 0, 2, 1]
    fill(perm)
    second_calls, got2 = launch()
    (_, a1, name1), (_, a2, name2) = first_calls[0], second_calls[0]
    assert len(first_calls) == len(second_calls) == 1 and name1 == name2 == "sy_frames_u8_pack_surfaces"
    assert a1[:7] + a1[8:] == a2[:7] + a2[8:] and a1[0] == rows.table.data_ptr()
    for b2, k in enumerate(perm):
        for lay in range(4):
            assert torch.equal(got2[lay][b2], got[lay][k]), (b2, k, lay)


# ---- 6: nothing is copied -----------------------------------------------------------------------------------------------------------
def test_a_surface_row_is_pointers_only(backend):
    """set_row with a Surface and a tick: the arena keeps its bytes, the table row holds the planes' data_ptr()s and strides, the
    planes are referenced until the row is set again; a staged row is a descriptor with plane1 = NULL into the arena."""
    nv = _nv12(21, 32, 64)
    s, _ = _nv12_surface(nv, "a", backend)
    rows = FrameSurfacesU8(2, MAX_HW, CANVAS, backend)
    assert rows._rows.dtype.itemsize == 48 and rows.table.numel() == 96 and rows.pixel_format == "surfaces"
    assert rows.decimate == ("surfaces", rows.table.data_ptr())
    legacy = FrameRowsU8(2, MAX_HW, CANVAS, backend)
    assert legacy._rows.dtype.itemsize == 32 and legacy.table.numel() == 64 and legacy.decimate == ("rows", legacy.table.data_ptr())
    rows.arena.fill_(77)
    rows.set_row(0, s, mirror=True)
    rows.upload()
    out = rows.to_nchw()
    assert torch.equal(rows.arena, torch.full_like(rows.arena, 77))
    assert tuple(rows._rows[0]) == (s.planes[0].data_ptr(), s.planes[1].data_ptr(), 32, 64, 70, 70, 1, 1, _lib.PIX_NV12, 0)
    assert rows._held[0] is s.planes and rows._held[1] is None
    dev_table = rows.table.cpu().numpy().view(rows._rows.dtype)
    assert np.array_equal(dev_table, rows._rows)
    assert torch.equal(out[0], _staged(nv, (32, 64, 1, 1), CANVAS, backend)[0][0])
    assert torch.equal(out[1], torch.full_like(out[1], 114.0))
    rows.set_row(0, nv, pixel_format="nv12")
    assert rows._held[0] is None
    assert tuple(rows._rows[0]) == (rows.arena.data_ptr(), 0, 32, 64, 64, 0, 1, 0, _lib.PIX_NV12, 0)
    assert not torch.equal(rows.arena, torch.full_like(rows.arena, 77))
    rows.set_row(1, s)
    rows.set_row(1, None)
    assert rows._held[1] is None and tuple(rows._rows[1]) == (0, 0, 0, 0, 0, 0, 1, 0, 0, 0)


# ---- 7: impossible descriptors --------------------------------------------------------------------------------------------------------
def test_impossible_descriptors_are_the_plain_canvas(backend):
    """Table rows written by hand whose pointers aim at non-114 bytes: an unknown format, odd NV12 / P010 sizes, a luma or chroma
    pitch below the row's bytes and a negative chroma pitch are written as all-114, the good rows beside them are written.  Bad
    host arguments: sy_frames_u8_pack_rows' status codes."""
    rows = FrameSurfacesU8(10, (16, 16), (16, 16), backend)
    nv = _nv12(3, 16, 16)
    data = _t(np.concatenate([nv, nv, nv]), backend)             # 72 rows of 16 bytes, none of them all 114
    p, NV, P0 = data.data_ptr(), _lib.PIX_NV12, _lib.PIX_P010
    uv = p + 16 * 16
    rows._rows[0] = (p, uv, 16, 16, 16, 16, 1, 0, NV, 0)         # good: NV12
    rows._rows[1] = (p, uv, 16, 16, 48, 48, 1, 0, 4, 0)          # unknown format
    rows._rows[2] = (p, uv, 16, 15, 16, 16, 1, 0, NV, 0)         # odd NV12 width
    rows._rows[3] = (p, uv, 15, 16, 16, 16, 1, 0, NV, 0)         # odd NV12 height
    rows._rows[4] = (p, uv, 16, 7, 16, 16, 1, 0, P0, 0)          # odd P010 width
    rows._rows[5] = (p, uv, 16, 16, 15, 16, 1, 0, NV, 0)         # pitch below the row bytes
    rows._rows[6] = (p, uv, 16, 16, 16, 15, 1, 0, NV, 0)         # chroma pitch below the row bytes
    rows._rows[7] = (p, uv, 16, 16, 16, -16, 1, 0, NV, 0)        # negative chroma pitch
    rows._rows[8] = (p, uv, 16, 8, 16, 15, 1, 0, P0, 0)          # P010: 16 bytes a row, chroma pitch 15
    rows._rows[9] = (p, 0, 16, 8, 16, 0, 1, 0, P0, 0)            # good: P010 [16, 8] words, plane1 NULL and chroma_stride 0
    rows.upload()
    out = rows.to_nchw().cpu()
    assert torch.equal(out[0], torch.from_numpy(nv12_to_bgr(nv)).permute(2, 0, 1).float())
    assert torch.equal(out[1:9], torch.full((8, 3, 16, 16), 114.0))
    hi = nv[:, 1::2]                                             # the high bytes of the words the P010 row sees
    want9 = torch.full((3, 16, 16), 114.0)
    want9[:, :, :8] = torch.from_numpy(nv12_to_bgr(hi)).permute(2, 0, 1).float()
    assert torch.equal(out[9], want9)
    v = View.alloc(10, 8, 8, 16, "fp16", backend)
    rows.pack_focus(v)
    f = v.buf.reshape(10, 64, 16).cpu().float()
    assert torch.equal(f[1:9, :, :12], torch.full((8, 64, 12), 114.0)) and torch.equal(f[..., 12:], torch.zeros(10, 64, 4))
    assert not torch.equal(f[0, :, :12], torch.full((64, 12), 114.0))

    lib = _lib.lib()
    rows = FrameSurfacesU8(2, (8, 8), (8, 8), backend)
    out = torch.zeros((2, 3, 8, 8), dtype=torch.float32, device=backend)
    t, o, st = rows.table.data_ptr(), out.data_ptr(), ops.stream_of(out)
    fn = lib.sy_frames_u8_pack_surfaces
    assert fn(t, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 0
    assert fn(None, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 1
    assert fn(t, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, None, _lib.DT_F32, st) == 1
    assert fn(t, 0, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 1
    assert fn(t, 2, 8, 8, 7, 8, ops.FRAMES_FOCUS, o, _lib.DT_F32, st) == 1
    assert fn(t, 2, 8, 8, 8, 7, ops.FRAMES_FOCUS, o, _lib.DT_F32, st) == 1
    assert fn(t, 2, 8, 8, 8, 8, 2, o, _lib.DT_F32, st) == 1
    assert fn(t, 2, 8, 8, 8, 8, ops.FRAMES_FOCUS, o, 7, st) == 1
    assert fn(t, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F16, st) == 1
    assert fn(t, 65536, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 3
    assert torch.equal(out.cpu(), torch.full((2, 3, 8, 8), 114.0))               # (only the good call wrote)


# ---- 8: the Python layer ------------------------------------------------------------------------------------------------------------
HW, D_CANVAS, OTHER = (128, 192), (64, 96), (90, 150)            # tests/test_multistream_mixed.py's sizes


def test_python_layer_rejects_before_anything_is_stored(backend):
    """Surface / set_row / open / _check: ValueError with table, divisors, arena and the stream bookkeeping as they were."""
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=backend)        # noqa: E731
    bad = [(lambda: Surface((u8(16, 16).float(), u8(8, 16)), "nv12")),               # dtype
           (lambda: Surface((u8(16, 16), u8(8, 16).to(torch.int16)), "nv12")),
           (lambda: Surface((u8(16, 32)[:, ::2], u8(8, 16)), "nv12")),                # innermost stride 2
           (lambda: Surface(u8(16, 16, 6)[:, :, ::2], "bgr")),
           (lambda: Surface(u8(16, 32, 3)[:, ::2], "rgb")),                           # pixel stride 6
           (lambda: Surface((u8(16, 16), u8(8, 14)), "nv12")),                        # planes that do not agree
           (lambda: Surface((u8(16, 16), u8(16, 16)), "nv12")),
           (lambda: Surface((u8(16, 32), u8(8, 16)), "p010")),
           (lambda: Surface((u8(15, 16), u8(7, 16)), "nv12")),                        # odd sizes
           (lambda: Surface((u8(16, 14), u8(8, 14)), "p010")),                        # 7 words
           (lambda: Surface((u8(16, 15), u8(8, 15)), "p010")),                        # half a word
           (lambda: Surface((u8(16, 16),), "nv12")),                                  # one plane
           (lambda: Surface((u8(16, 16), u8(8, 16)), "bgr")),
           (lambda: Surface(u8(16, 16), "bgr")),                                      # dims
           (lambda: Surface(u8(16, 16, 4)[:, :, :3], "bgr")),                         # BGRA: pixel stride 4
           (lambda: Surface((u8(1, 16).expand(16, 16), u8(8, 16)), "nv12")),          # pitch 0 < Ws
           (lambda: Surface((np.zeros((16, 16), np.uint8), np.zeros((8, 16), np.uint8)), "nv12")),
           (lambda: Surface((u8(16, 16), u8(8, 16)), "i420")),
           (lambda: Surface.from_buffer(u8(24, 16), 16, 16, "nv12", chroma_row=17)),  # chroma rows past the buffer
           (lambda: Surface.from_buffer(u8(24, 16), 16, 16, "p010")),                 # 32 bytes a row do not fit
           (lambda: Surface.from_buffer(u8(24, 16), 16, 6, "bgr"))]
    for k, make in enumerate(bad):
        with pytest.raises(ValueError):
            make()
            pytest.fail("case %d was accepted" % k)
    good = Surface((u8(16, 16), u8(8, 16)), "nv12")
    p010 = Surface((u8(16, 32), u8(8, 32)), "p010")
    assert Surface((torch.zeros((16, 16), dtype=torch.int16, device=backend),) * 1 +
                   (torch.zeros((8, 16), dtype=torch.int16, device=backend),), "p010").hw == (16, 16)

    rows = FrameSurfacesU8(2, (16, 16), (16, 16), backend)
    rows.set_row(0, good)
    rows.set_row(1, np.full((16, 16, 3), 9, np.uint8), pixel_format="rgb")
    table, div, arena, held = rows._rows.copy(), rows._div.copy(), rows.arena.clone(), list(rows._held)
    elsewhere = torch.device("meta")                             # (a device that is never the object's)
    away = Surface((torch.zeros((16, 16), dtype=torch.uint8, device=elsewhere),
                    torch.zeros((8, 16), dtype=torch.uint8, device=elsewhere)), "nv12")
    for args, kw in (((0, away), {}),                                                 # the wrong device
                     ((0, good), {"pixel_format": "p010"}),                           # not the surface's format
                     ((2, good), {}),                                                 # no such row
                     ((0, good), {"decimate": 2}),                                    # 8 x 8 does not fill a 16 x 16 canvas
                     ((0, good), {"decimate": -1}),                                   # no divisor
                     ((0, Surface((u8(32, 32), u8(16, 32)), "nv12")), {"decimate": 1}),
                     ((0, np.zeros((16, 32), np.uint8)), {"pixel_format": "p010"}),   # P010 goes through Surface only
                     ((0, np.zeros((24, 15), np.uint8)), {"pixel_format": "nv12"})):
        with pytest.raises(ValueError):
            rows.set_row(*args, **kw)
    assert np.array_equal(rows._rows, table) and np.array_equal(rows._div, div) and torch.equal(rows.arena, arena)
    assert all(a is b for a, b in zip(rows._held, held))

    # "p010" outside surfaces is an unknown name
    with pytest.raises(ValueError):
        FramePairsU8(u8(1, 24, 32), None, (16, 16), pixel_format="p010")
    legacy = FrameRowsU8(1, (16, 16), (16, 16), backend)
    with pytest.raises(ValueError):
        legacy.set_row(0, np.zeros((24, 32), np.uint8), pixel_format="p010")
    with pytest.raises(ValueError):
        _lib.pixel_format_code("p010")
    assert _lib.pixel_format_code("p010", surfaces=True) == _lib.PIX_P010 == 3
    model = _models(backend)
    with pytest.raises(ValueError):
        S.StreamingDetector(model, HW, dtype="fp32", device=backend, pixel_format="p010")
    with pytest.raises(ValueError):
        S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend, pixel_format="p010")
    with pytest.raises(ValueError):
        S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend, max_frame_hw=HW, pixel_format="p010")
    mixed = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend, max_frame_hw=HW)
    assert type(mixed._in) is FrameRowsU8 and not mixed.surfaces
    with pytest.raises(ValueError):
        mixed.open(pixel_format="p010")
    m = mixed.open(pixel_format="nv12")
    with pytest.raises(ValueError):
        mixed._check([Surface((u8(*HW), u8(HW[0] // 2, HW[1])), "nv12")], [m])       # a Surface without surfaces=True

    det = S.MultiStreamDetector(model, HW, max_streams=3, batch=2, dtype="fp32", device=backend, surfaces=True)
    assert type(det._in) is FrameSurfacesU8 and det.max_frame_hw == HW and det._stage is None
    a, b = det.open(pixel_format="nv12"), det.open(frame_hw=OTHER, pixel_format="p010")
    state = (list(det._free), det._next_id, dict(det._slot_of), dict(det._first), dict(det._geom), dict(det._fmt))
    with pytest.raises(ValueError):
        det.open(frame_hw=(90, 149), pixel_format="p010")                             # odd width
    with pytest.raises(ValueError):
        det.open(frame_hw=(130, 192), pixel_format="p010")                            # above max_frame_hw
    with pytest.raises(ValueError):
        det.open(pixel_format="p016")
    assert state == (det._free, det._next_id, det._slot_of, det._first, det._geom, det._fmt)
    table, div, arena = det._in._rows.copy(), det._in._div.copy(), det._in.arena.clone()
    nv_hw = Surface((u8(*HW), u8(HW[0] // 2, HW[1])), "nv12")
    p_other = Surface((u8(OTHER[0], 2 * OTHER[1]), u8(OTHER[0] // 2, 2 * OTHER[1])), "p010")
    away_p = Surface((torch.zeros((OTHER[0], 2 * OTHER[1]), dtype=torch.uint8, device=elsewhere),
                      torch.zeros((OTHER[0] // 2, 2 * OTHER[1]), dtype=torch.uint8, device=elsewhere)), "p010")
    for frames, sids in (([p_other], [a]),                                            # not its stream's format
                         ([Surface((u8(*OTHER), u8(OTHER[0] // 2, OTHER[1])), "nv12")], [a]),      # not its stream's size
                         ([nv_hw], [b]),
                         ([np.zeros((OTHER[0] * 3 // 2, OTHER[1]), np.uint8)], [b]),  # a plain frame on the P010 stream
                         ([nv_hw, away_p], [a, b])):                                  # the wrong device, after a good frame
        with pytest.raises(ValueError):
            det(frames, sids)
    assert np.array_equal(det._in._rows, table) and np.array_equal(det._in._div, div) and torch.equal(det._in.arena, arena)
    assert det._first[a] and det._first[b]
    assert len(det._check([nv_hw, p_other], [a, b])) == 2
    assert len(det._check([np.zeros((HW[0] * 3 // 2, HW[1]), np.uint8)], [a])) == 1  # (a staged frame on the NV12 stream)


# ---- 9: the detector ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] is None


def test_detector_on_surfaces_end_to_end(backend):
    """MultiStreamDetector(batch=3, surfaces=True) with a padded NV12-surface stream (layout a), a P010-surface stream and a staged
    BGR stream over 3 ticks with a reset == a surfaces=False mixed detector fed the repacked frames (P010: its high-byte NV12
    frame), exactly; every tick replays the one tape, which holds one sy_frames_u8_pack_surfaces and no sy_frames_u8_pack_rows."""
    model = _models(backend)
    sizes, fmts, ref_fmts = [HW, OTHER, D_CANVAS], ["nv12", "p010", "bgr"], ["nv12", "nv12", "bgr"]
    det = S.MultiStreamDetector(model, HW, max_streams=3, batch=3, dtype="fp32", device=backend, surfaces=True)
    ref = S.MultiStreamDetector(model, HW, max_streams=3, batch=3, dtype="fp32", device=backend, max_frame_hw=HW)
    assert type(det._in) is FrameSurfacesU8 and type(ref._in) is FrameRowsU8
    det.warm_up(2); ref.warm_up(2)
    tape = det.plan._slots_tape[2]
    n_launch = tape.size()
    assert ref.plan._slots_tape[2].size() == n_launch
    sid = [det.open(frame_hw=hw, pixel_format=f) for hw, f in zip(sizes, fmts)]
    rid = [ref.open(frame_hw=hw, pixel_format=f) for hw, f in zip(sizes, ref_fmts)]
    seed = [500]

    def frame(i):
        """-> (what stream i delivers, the same picture repacked for the staged detector)"""
        seed[0] += 1
        if fmts[i] == "bgr":
            f = np.random.RandomState(seed[0]).randint(0, 256, sizes[i] + (3,)).astype(np.uint8)
            return f, f
        nv = _nv12(seed[0], *sizes[i])
        if fmts[i] == "nv12":
            return _nv12_surface(nv, "a", backend, pad_seed=seed[0])[0], nv
        return _nv12_surface(_p010_words(nv, seed[0]), "c", backend, pad_seed=seed[0], step=2)[0], nv

    def tick(order):
        fs = [frame(i) for i in order]
        arena = det._in.arena.clone()
        got = det([f[0] for f in fs], [sid[i] for i in order])
        want = ref([f[1] for f in fs], [rid[i] for i in order])
        for b in range(len(order)):
            assert _same(got[b], want[b]), (seed[0], order, b)
        assert det.plan._slots_tape[2] is tape and tape.size() == n_launch
        if 2 not in order:
            assert torch.equal(det._in.arena, arena)             # (surface rows only: nothing was staged)
        return got
    got = tick([0, 1, 2])
    assert sum(len(r[0]) for r in got) > 0
    tick([1, 0])                                                 # the staged stream absent, the surfaces in other rows
    det.reset(sid[0]); ref.reset(rid[0])
    tick([2, 0, 1])
    assert [int(f) for f in det._in._rows["format"]] == [_lib.PIX_BGR, _lib.PIX_NV12, _lib.PIX_P010]
    assert det._in._rows["plane1"][0] == 0 and det._in._rows["plane1"][1] != 0 and det._in._rows["chroma_stride"][2] == 2 * OTHER[1] + 10
    with _lib.record() as calls, torch.no_grad():
        det.plan.run_stream_slots(det._in, det.state)
    names = [c[2] for c in calls]
    assert names[0] == "sy_frames_u8_pack_surfaces" and names.count("sy_frames_u8_pack_surfaces") == 1
    assert "sy_frames_u8_pack_rows" not in names and "sy_frames_u8_pack" not in names and "sy_frames_u8_pack_fmt" not in names
    with _lib.record() as calls, torch.no_grad():
        ref.plan.run_stream_slots(ref._in, ref.state)
    names = [c[2] for c in calls]
    assert names[0] == "sy_frames_u8_pack_rows" and "sy_frames_u8_pack_surfaces" not in names

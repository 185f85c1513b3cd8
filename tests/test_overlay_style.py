"""The host side of the overlay (streamyolo_amd/overlay.py, data.Surface.clone): palette arithmetic, class text, the font table,
surface copies and every ValueError.  No GPU and no kernel library: CPU tensors only."""
import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import overlay as OV
from streamyolo_amd.data import Surface
from streamyolo_amd.utils.synth import bgr_to_nv12


def test_palette_yuv_matches_the_float_matrix():
    """The integer BT.601 form is within 1 LSB of utils/synth's float matrix (rounded) for 256 random colours."""
    rng = np.random.RandomState(0)
    bgr = rng.randint(0, 256, size=(256, 3)).astype(np.uint8)
    bgr[:4] = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255)]
    pal = OV.palette_rows(bgr)
    assert pal.dtype == np.uint8 and pal.shape == (256, 8) and np.array_equal(pal[:, :3], bgr)
    frame = np.repeat(np.repeat(bgr[None], 2, axis=0), 2, axis=1)    # one constant 2 x 2 block per colour: [2, 512, 3]
    nv12 = bgr_to_nv12(torch.from_numpy(frame)).numpy().astype(np.int64)
    y, uv = nv12[0, ::2], nv12[2].reshape(256, 2)
    assert np.abs(pal[:, 4].astype(np.int64) - y).max() <= 1
    assert np.abs(pal[:, 5:7].astype(np.int64) - uv).max() <= 1
    assert pal[:, 4].min() >= 16 and pal[:, 4].max() <= 235 and pal[:, 5:7].min() >= 16 and pal[:, 5:7].max() <= 240
    assert tuple(pal[0, 4:7]) == (16, 128, 128) and tuple(pal[1, 4:7]) == (235, 128, 128)


def test_text_value_selection():
    """White text (255, luma 235) on colours with Y < 128, black (0, luma 16) otherwise — decided on the integer Y."""
    rng = np.random.RandomState(1)
    bgr = rng.randint(0, 256, size=(200, 3))
    pal = OV.palette_rows(bgr).astype(np.int64)
    dark = pal[:, 4] < 128
    assert dark.any() and (~dark).any()
    assert np.array_equal(pal[:, 3], np.where(dark, 255, 0)) and np.array_equal(pal[:, 7], np.where(dark, 235, 16))
    grey = OV.palette_rows([(129, 129, 129), (130, 130, 130)])       # Y = 127 and 128: either side of the switch
    assert list(grey[:, 4]) == [127, 128] and list(grey[:, 3]) == [255, 0] and list(grey[:, 7]) == [235, 16]


def test_name_normalisation():
    code = lambda text: [ord(c) - 32 for c in text]
    assert OV.encode_name("car") == code("CAR")
    assert OV.encode_name("traffic_light") == code("TRAFFIC_")       # cut to 8 glyphs
    assert OV.encode_name("a{b}~é\n") == code("A B    ")         # outside ASCII 32..95 (after upper-casing): spaces
    assert OV.encode_name("") == []
    assert OV.encode_name("x-1:#%.") == code("X-1:#%.")
    st = sy.OverlayStyle(class_names=["bus", "stop_sign"])
    assert st.class_text.shape == (2, 8) and st.class_text.dtype == np.uint8
    assert list(st.class_text[0]) == code("BUS") + [0xFF] * 5 and list(st.class_text[1]) == code("STOP_SIG")
    assert OV.DEFAULT_CLASS_NAMES == ["person", "bicycle", "car", "motorcycle", "bus", "truck", "traffic_light", "stop_sign"]
    assert len(set(OV.DEFAULT_PALETTE)) == 8


def test_font_table():
    g = OV.font_glyphs()
    assert g.shape == (64, 8) and g.dtype == np.uint8
    need = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#%.-_:"
    rows = [bytes(g[ord(c) - 32]) for c in need]
    assert all(any(r) for r in rows)                                 # none blank
    assert len(set(rows)) == len(need)                               # all distinct
    assert not g[0].any()                                            # the space
    assert not (g & 0x81).any()                                      # a blank column on either side of every glyph: labels do not run together


def test_surface_clone_keeps_pitches_and_shares_nothing():
    rng = np.random.RandomState(2)
    wide = torch.from_numpy(rng.randint(0, 256, size=(10, 60)).astype(np.uint8))
    bgr = Surface.from_buffer(wide, 10, 14, "bgr")                   # pitch 60 > 3 * 14
    buf = torch.from_numpy(rng.randint(0, 256, size=(20, 24)).astype(np.uint8))
    nv12 = Surface.from_buffer(buf, 8, 20, "nv12", chroma_row=12)    # a padded luma, pitch 24 > 20
    luma = torch.from_numpy(rng.randint(0, 256, size=(6, 40)).astype(np.uint8))
    chroma = torch.from_numpy(rng.randint(0, 256, size=(3, 64)).astype(np.uint8))
    p010 = Surface((luma[:, :32], chroma[:, :32]), "p010")           # 6 x 16 samples; pitches 40 and 64
    for s in (bgr, nv12, p010):
        c = s.clone()
        assert isinstance(c, Surface) and c.pixel_format == s.pixel_format and c.format == s.format and c.hw == s.hw
        assert c.pitch == s.pitch and c.chroma_pitch == s.chroma_pitch and c.device == s.device
        assert len(c.planes) == len(s.planes)
        for a, b in zip(c.planes, s.planes):
            assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b)
            assert a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
        before = [p.clone() for p in s.planes]
        for a in c.planes:
            a.fill_(7)
        assert all(torch.equal(p, q) for p, q in zip(s.planes, before))


@pytest.mark.parametrize("kw", [
    dict(thickness=0), dict(thickness=17), dict(thickness=2.5), dict(thickness=True), dict(text_scale=-1), dict(text_scale=5),
    dict(text_scale="2"), dict(show="name"), dict(show=1), dict(min_score=float("nan")), dict(min_score=float("inf")),
    dict(min_score="high"), dict(max_boxes=0), dict(max_boxes=257), dict(max_boxes=1.5), dict(class_names=[]),
    dict(class_names=["a"] * 129), dict(class_names=["a", 3]), dict(palette=[(1, 2, 3)]), dict(palette=[(0, 0, 256)] * 8),
    dict(palette=[(0, 0)] * 8), dict(palette=[(0, 0, -1)] * 8), dict(palette=5), dict(class_names=["a", "b"], palette=[(1, 2, 3)] * 3),
])
def test_style_value_errors(kw):
    with pytest.raises(ValueError):
        sy.OverlayStyle(**kw)


def test_style_defaults_and_flags():
    st = sy.OverlayStyle()
    assert (st.thickness, st.text_scale, st.show, st.min_score, st.max_boxes) == (2, 2, "id", 0.3, 128)
    assert st.flags == 1 and sy.OverlayStyle(show="score").flags == 2 and sy.OverlayStyle(show=None).flags == 0
    assert st.palette.shape == (8, 8) and len({tuple(r[:3]) for r in st.palette}) == 8
    long = sy.OverlayStyle(class_names=["c%d" % k for k in range(20)])            # the default colours repeat
    assert long.palette.shape == (20, 8) and np.array_equal(long.palette[8], long.palette[0])
    pal, text, glyphs = st.tables("cpu")
    assert pal.dtype == text.dtype == glyphs.dtype == torch.uint8 and tuple(glyphs.shape) == (64, 8)
    assert st.tables("cpu")[0] is pal                                # built once per device


def test_target_value_errors():
    """What draw_detections and the detectors' draw() refuse before anything reaches the device."""
    frame = torch.zeros((12, 16, 3), dtype=torch.uint8)
    assert isinstance(OV.as_target(frame), Surface) and OV.as_target(frame).pixel_format == "bgr"
    for bad in (np.zeros((12, 16, 3), np.uint8), torch.zeros((12, 16, 3)), torch.zeros((12, 16), dtype=torch.uint8),
                torch.zeros((12, 16, 4), dtype=torch.uint8), "frame"):
        with pytest.raises(ValueError):
            OV.as_target(bad)
    with pytest.raises(ValueError):
        OV.as_target(frame, hw=(12, 18))
    with pytest.raises(ValueError):
        OV.as_target(frame, device="cuda:0")
    with pytest.raises(ValueError):
        sy.draw_detections(frame, np.zeros((2, 4)), np.zeros(3), np.zeros(2))      # 2 boxes, 3 scores
    with pytest.raises(ValueError):
        sy.draw_detections(frame, np.zeros((2, 4)), np.zeros(2), np.zeros(2), ids=np.zeros(1))
    with pytest.raises(ValueError):
        sy.draw_detections(frame, np.zeros((2, 4)), np.zeros(2), np.zeros(2), style="thick")
    assert sy.draw_detections(frame, np.zeros((0, 4)), [], []) is frame and not frame.any()      # nothing to draw: no launch

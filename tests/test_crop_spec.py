"""The host side of the crops (streamyolo_amd/crops.py): what CropSpec refuses, how its fields become the kernel's table values
(pad -> pad_q8, class list -> mask, mean / std -> the plane-order tables, flags, capacity) and what a source may be.  No library, no
device."""
import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import _lib
from streamyolo_amd import crops as CR
from streamyolo_amd.data import Surface


@pytest.mark.parametrize("kw", [
    dict(size=(64,)), dict(size=64), dict(size=(4, 64)), dict(size=(64, 4)), dict(size=(520, 64)), dict(size=(64, 520)),
    dict(size=(64, 60)), dict(size=(64.0, 64)), dict(size=(True, 64)), dict(size=("64", "64")),
    dict(pad=-0.1), dict(pad=1.01), dict(pad=float("nan")), dict(pad="wide"), dict(pad=True),
    dict(dtype=torch.float64), dict(dtype=torch.int8), dict(dtype="fp16"), dict(channel_order="gbr"), dict(channel_order=None),
    dict(mean=(1, 2)), dict(mean=(1, 2, float("inf"))), dict(mean=5), dict(std=(1, 0, 1)), dict(std=(1, 2, float("nan"))),
    dict(std="unit"), dict(dtype=torch.uint8, mean=(1, 2, 3)), dict(dtype=torch.uint8, std=(1, 2, 3)),
    dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_score="high"),
    dict(max_per_stream=-1), dict(max_per_stream=257), dict(max_per_stream=1.5), dict(max_per_stream=True),
    dict(classes=[128]), dict(classes=[-1]), dict(classes=[1.5]), dict(classes=3), dict(classes=[True]),
    dict(fill=(1, 2)), dict(fill=(0, 0, 256)), dict(fill=(0, -1, 0)), dict(fill=(1.5, 2, 3)), dict(fill=7),
    dict(capacity=0), dict(capacity=-4), dict(capacity=2.5), dict(capacity=2 ** 31),
])
def test_spec_value_errors(kw):
    with pytest.raises(ValueError):
        sy.CropSpec(**kw)


def test_spec_defaults():
    sp = sy.CropSpec()
    assert sp.size == (64, 64) and sp.pad == 0.0 and sp.pad_q8 == 0 and sp.keep_aspect and sp.dtype == torch.float16
    assert sp.channel_order == "bgr" and sp.flags == _lib.CROP_KEEP_ASPECT and sp.fill == (114, 114, 114)
    assert sp.min_score == 0.0 and sp.max_per_stream == 0 and sp.classes is None and sp.capacity is None
    assert sp.class_mask == (0xFFFFFFFF,) * 4                        # every class
    assert sp.mean is None and sp.scale is None and sp.tables("cpu") == (None, None)
    assert sp.slots(4) == 4 * CR.DEFAULT_PER_STREAM


def test_pad_becomes_pad_q8():
    for pad, q in ((0.0, 0), (0.1, 26), (0.25, 64), (0.5, 128), (1.0, 256), (1 / 512, 0), (3 / 512, 2), (0.998, 255), (0.9999, 256)):
        assert sy.CropSpec(pad=pad).pad_q8 == q == int(round(pad * 256)), pad


def test_class_list_becomes_the_mask():
    assert sy.CropSpec(classes=[]).class_mask == (0, 0, 0, 0)        # nothing is cropped
    assert sy.CropSpec(classes=[0]).class_mask == (1, 0, 0, 0)
    sp = sy.CropSpec(classes=[6, 7, 6, 31, 32, 95, 127])
    assert sp.classes == (6, 7, 31, 32, 95, 127)
    assert sp.class_mask == ((1 << 6) | (1 << 7) | (1 << 31), 1, 1 << 31, 1 << 31)
    assert sy.CropSpec(classes=np.array([2, 64])).class_mask == (4, 0, 1, 0)
    assert sy.CropSpec(classes=range(128)).class_mask == sy.CropSpec().class_mask


def test_mean_and_std_stay_in_plane_order():
    """mean / std are given per OUTPUT plane: whatever channel_order says, table entry c belongs to plane c, and the scale is the
    float32 reciprocal of the float32 std."""
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    for order in ("rgb", "bgr"):
        sp = sy.CropSpec(dtype=torch.float32, channel_order=order, mean=mean, std=std)
        assert sp.mean.dtype == sp.scale.dtype == np.float32
        assert np.array_equal(sp.mean, np.asarray(mean, dtype=np.float32))
        assert np.array_equal(sp.scale, np.float32(1.0) / np.asarray(std, dtype=np.float32))
        assert sp.flags == _lib.CROP_KEEP_ASPECT | (_lib.CROP_RGB_OUT if order == "rgb" else 0)
    only_mean = sy.CropSpec(mean=(1, 2, 3))
    assert np.array_equal(only_mean.scale, np.ones(3, dtype=np.float32)) and np.array_equal(only_mean.mean, [1, 2, 3])
    only_std = sy.CropSpec(std=(2, 4, 8), keep_aspect=False)
    assert np.array_equal(only_std.mean, np.zeros(3, dtype=np.float32)) and np.array_equal(only_std.scale, [0.5, 0.25, 0.125])
    assert only_std.flags == 0
    m, s = only_std.tables("cpu")
    assert m.dtype == s.dtype == torch.float32 and s.tolist() == [0.5, 0.25, 0.125]
    assert only_std.tables("cpu")[0] is m                            # built once per device


def test_capacity_and_row_cap():
    assert sy.CropSpec(max_per_stream=5).slots(4) == 20
    assert sy.CropSpec(max_per_stream=5, capacity=7).slots(4) == 7
    assert sy.CropSpec(capacity=100).slots(1) == 100


def test_specs_compare_by_value_and_share_a_detectors_buffers():
    """Two specs built from the same arguments are the same key of a detector's output cache (a spec written inline in a loop
    must not allocate a batch per tick), and the cache holds a few specs only."""
    kw = dict(size=(16, 24), pad=0.1, dtype=torch.float32, mean=(1, 2, 3), std=(2, 4, 8), classes=[3, 1], max_per_stream=5)
    a, b = sy.CropSpec(**kw), sy.CropSpec(**dict(kw, classes=(1, 3, 3), pad=0.1001))       # (the same mask, the same pad_q8)
    assert a is not b and a == b and hash(a) == hash(b) and a != "spec"
    for other in (dict(size=(16, 32)), dict(pad=0.2), dict(dtype=torch.float16), dict(mean=(1, 2, 4)), dict(std=None), dict(classes=[1]),
                  dict(max_per_stream=6), dict(keep_aspect=False), dict(channel_order="rgb"), dict(min_score=0.5), dict(fill=(1, 2, 3)),
                  dict(capacity=7)):
        assert sy.CropSpec(**dict(kw, **other)) != a, other
    cache = CR.CropCache()
    one = cache.get(a, 2, "cpu")
    assert tuple(one.images.shape) == (10, 3, 16, 24) and one.spec is a
    assert cache.get(b, 2, "cpu") is one and len(cache) == 1 and cache.peek(b) is one
    for k in range(10):
        cache.get(sy.CropSpec(capacity=1 + k), 2, "cpu")
        cache.get(a, 2, "cpu")                                       # (in use all along: never the one that goes)
    assert len(cache) == CR.CropCache.SIZE and cache.get(b, 2, "cpu") is one
    assert cache.peek(sy.CropSpec(capacity=1)) is None               # the least recently used ones went


def test_table_record_matches_the_header_struct():
    import ctypes as C
    assert CR._CROP_DTYPE.itemsize == C.sizeof(_lib.CropRow) == 72
    for name, _ in _lib.CropRow._fields_:
        assert CR._CROP_DTYPE.fields[name][1] == getattr(_lib.CropRow, name).offset, name
    rows = CR.CropRows(2, "cpu")
    sp = sy.CropSpec(pad=0.1, min_score=0.25, max_per_stream=9, classes=[1, 33], fill=(1, 2, 3))
    frame = torch.zeros((12, 16, 3), dtype=torch.uint8)
    rows.set_row(1, Surface(frame, "bgr"), 0.5, sp)
    r = rows._rows[1]
    assert (r["plane0"], r["plane1"], r["Hs"], r["Ws"], r["row_stride"], r["format"]) == (frame.data_ptr(), 0, 12, 16, 48, _lib.PIX_BGR)
    assert (r["divisor"], r["min_score"], r["max_crops"], r["pad_q8"]) == (0.5, 0.25, 9, 26)
    assert r["fill"].tolist() == [1, 2, 3, 0] and r["class_mask"].tolist() == [2, 2, 0, 0]
    assert not rows._rows[0]["plane0"] and tuple(rows.table.shape) == (144,)


def test_source_value_errors():
    """What crop_detections and the detectors' crops() refuse before anything reaches the device."""
    frame = torch.zeros((12, 16, 3), dtype=torch.uint8)
    assert isinstance(CR.as_source(frame), Surface) and CR.as_source(frame).pixel_format == "bgr"
    for bad in (np.zeros((12, 16, 3), np.uint8), torch.zeros((12, 16, 3)), torch.zeros((12, 16), dtype=torch.uint8),
                torch.zeros((12, 16, 4), dtype=torch.uint8), "frame"):
        with pytest.raises(ValueError):
            CR.as_source(bad)
    with pytest.raises(ValueError):
        CR.as_source(frame, hw=(12, 18))
    with pytest.raises(ValueError):
        CR.as_source(frame, device="cuda:0")
    with pytest.raises(ValueError):
        sy.crop_detections(frame, np.zeros((2, 4)), np.zeros(3), np.zeros(2))      # 2 boxes, 3 scores
    with pytest.raises(ValueError):
        sy.crop_detections(frame, np.zeros((2, 4)), np.zeros(2), np.zeros(2), ids=np.zeros(1))
    with pytest.raises(ValueError):
        sy.crop_detections(frame, np.zeros((2, 4)), np.zeros(2), np.zeros(2), spec="small")

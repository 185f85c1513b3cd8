"""RedactSpec (streamyolo_amd/redact.py) on the host: validation before anything reaches the device, value equality, the fill
colour's bytes in both colour spaces, and the descriptor record against the size include/streamyolo_hip.h states.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import streamyolo_amd as sy
from streamyolo_amd import _lib
from streamyolo_amd.overlay import palette_rows
from streamyolo_amd.redact import _REDACT_DTYPE, RedactSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "streamyolo_hip.h")


def test_defaults():
    s = RedactSpec()
    assert (s.mode, s.cell, s.shape, s.pad, s.classes, s.min_score, s.fill) == ("pixelate", 16, "rect", 0.1, None, 0.0, (0, 0, 0))
    assert (s.mode_code, s.shape_code, s.pad_q8) == (_lib.REDACT_PIXELATE, _lib.REDACT_RECT, 26)
    assert s.class_mask == (0xFFFFFFFF,) * 4
    assert sy.RedactSpec is RedactSpec and callable(sy.redact_detections)


@pytest.mark.parametrize("kw", [
    dict(mode="blur"), dict(mode=0), dict(mode=None),
    dict(cell=0), dict(cell=5), dict(cell=64), dict(cell=16.0), dict(cell="16"), dict(cell=True), dict(cell=None),
    dict(shape="circle"), dict(shape=1), dict(shape=None),
    dict(pad=-0.01), dict(pad=1.01), dict(pad=float("nan")), dict(pad="wide"), dict(pad=None), dict(pad=True),
    dict(classes=[128]), dict(classes=[-1]), dict(classes=[1.5]), dict(classes=3), dict(classes=[True]), dict(classes=["car"]),
    dict(min_score=float("nan")), dict(min_score=float("inf")), dict(min_score="high"), dict(min_score=None),
    dict(fill=(0, 0)), dict(fill=(0, 0, 256)), dict(fill=(-1, 0, 0)), dict(fill=(0.5, 0, 0)), dict(fill=7), dict(fill=None),
    dict(fill=(0, 0, 0, 0)),
])
def test_rejected_with_value_error(kw):
    with pytest.raises(ValueError):
        RedactSpec(**kw)


def test_accepted_values():
    for cell in (4, 8, 16, 32, np.int64(8)):
        assert RedactSpec(cell=cell).cell == int(cell)
    assert RedactSpec(mode="fill").mode_code == _lib.REDACT_FILL and RedactSpec(shape="ellipse").shape_code == _lib.REDACT_ELLIPSE
    assert [RedactSpec(pad=p).pad_q8 for p in (0, 0.1, 0.5, 1, 1.0)] == [0, 26, 128, 256, 256]
    s = RedactSpec(classes=[2, 0, 0, 127, 33])
    assert s.classes == (0, 2, 33, 127) and s.class_mask == (0b101, 0b10, 0, 1 << 31)
    assert RedactSpec(classes=[]).class_mask == (0, 0, 0, 0)
    assert RedactSpec(classes=range(8)).class_mask == (0xFF, 0, 0, 0)
    assert RedactSpec(min_score=0.25).min_score == 0.25


def test_value_equality():
    a, b = RedactSpec(mode="fill", cell=8, pad=0.1, classes=[1, 0]), RedactSpec(mode="fill", cell=8, pad=0.1, classes=(0, 1, 1))
    assert a == b and hash(a) == hash(b) and a is not b and len({a, b}) == 1
    for kw in (dict(mode="pixelate"), dict(cell=16), dict(shape="ellipse"), dict(pad=0.2), dict(classes=None), dict(min_score=0.1),
               dict(fill=(0, 0, 1))):
        other = RedactSpec(**dict(dict(mode="fill", cell=8, pad=0.1, classes=[0, 1]), **kw))
        assert other != a, kw
    assert RedactSpec(pad=0.1) == RedactSpec(pad=0.1001)             # the same pad_q8: the same launch
    assert a != "fill" and not (a == None)                           # noqa: E711


@pytest.mark.parametrize("fill", [(0, 0, 0), (255, 255, 255), (10, 200, 90), (255, 0, 0), (0, 0, 255), (114, 114, 114)])
def test_fill_bytes_in_both_colour_spaces(fill):
    """B, G, R, 0, Y, U, V, 0 — the Y, U, V of overlay.palette_rows (BT.601 limited range in its integer form)."""
    s = RedactSpec(mode="fill", fill=fill)
    p = palette_rows([fill])[0]
    assert s.fill_bytes == (fill[0], fill[1], fill[2], 0, int(p[4]), int(p[5]), int(p[6]), 0)
    b, g, r = fill
    assert s.fill_bytes[4] == ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    assert all(0 <= v <= 255 for v in s.fill_bytes)


def test_record_size_is_the_headers():
    """The size the header STATES for sy_redact_row, the size a C compiler gives it, the numpy record and the ctypes mirror."""
    src = open(HEADER).read()
    stated = re.search(r"typedef struct sy_redact_row \{\s*/\* (\d+) bytes", src)
    assert stated is not None and int(stated.group(1)) == _REDACT_DTYPE.itemsize == C.sizeof(_lib.RedactRow) == 88
    for name, (kind, _) in _REDACT_DTYPE.fields.items():
        assert getattr(_lib.RedactRow, name).offset == _REDACT_DTYPE.fields[name][1], name
    assert re.search(r"#define SY_REDACT_MAX_SIDE (\d+)", src).group(1) == str(_lib.REDACT_MAX_SIDE)
    tile = tuple(int(re.search(r"#define SY_REDACT_TILE_%s (\d+)" % a, src).group(1)) for a in "HW")
    assert tile == _lib.REDACT_TILE and tile[0] % 32 == 0 and tile[1] % 32 == 0


def test_record_size_as_a_c_compiler_sees_it(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu\\n", sizeof(sy_redact_row), '
                   'offsetof(sy_redact_row, fill), offsetof(sy_redact_row, class_mask));return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    size, fill, mask = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (size, fill, mask) == (_REDACT_DTYPE.itemsize, _REDACT_DTYPE.fields["fill"][1], _REDACT_DTYPE.fields["class_mask"][1])


def test_rows_table_holds_what_the_spec_says():
    """RedactRows on the CPU: the record of a row as the kernel will read it."""
    import torch
    from streamyolo_amd.data import Surface
    from streamyolo_amd.redact import RedactRows
    frame = torch.zeros((40, 64, 3), dtype=torch.uint8)
    spec = RedactSpec(mode="fill", cell=8, shape="ellipse", pad=0.5, classes=[3], min_score=0.25, fill=(1, 2, 3))
    rows = RedactRows(2, "cpu")
    rows.set_row(1, Surface(frame, "bgr"), 0.5, spec)
    rows.upload()
    rec = rows.table.numpy().view(_REDACT_DTYPE)
    assert rec[0]["plane0"] == 0 and rec[0]["Hs"] == 0               # a row nobody set redacts nothing
    r = rec[1]
    assert r["plane0"] == frame.data_ptr() and (r["Hs"], r["Ws"], r["row_stride"], r["format"]) == (40, 64, 192, _lib.PIX_BGR)
    assert (r["divisor"], r["min_score"], r["pad_q8"], r["mode"], r["cell"], r["shape"], r["reserved"]) == (0.5, 0.25, 128, 1, 8, 1, 0)
    assert tuple(r["fill"]) == spec.fill_bytes and tuple(r["class_mask"]) == (8, 0, 0, 0)

"""MultiStreamDetector.crops / StreamingDetector.crops / sy.crop_detections (streamyolo_amd/crops.py over csrc/crop.hip) on the
MI355X with the nano model, 128x192 cameras and batch 4 (the setting of tests/test_multistream_overlay.py).

The expected batches come from the restatement of tests/test_crop_kernel.py (the rule of include/streamyolo_hip.h in plain numpy)
applied to the tick's OWN device tensors — the det / cnt of detect_device, or the tracker's out / out_id / out_cnt — and are
compared byte for byte over the whole images, index, rect and count tensors: what lies behind count[0] must be what it was."""
import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import _lib
from streamyolo_amd import streaming as S
from streamyolo_amd.data import Surface
from test_crop_kernel import NP_DTYPE, frame_of, raw, restate

pytestmark = pytest.mark.gpu

HW, BATCH, T = (128, 192), 4, 32
OTHER, CANVAS = (100, 150), (64, 96)
KIND = {torch.uint8: "u8", torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.use_library(_lib.DEFAULT_PATH)
    return torch.device("cuda:0")


def _model():
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    sd = synth_state_dict(O.param_shapes(O.OracleConfig.named("nano")), seed=0, bn_stats=load_bn_stats("nano"))
    model = sy.build_model("nano")
    model.load_state_dict(sd, strict=True)
    return model


def _clip(hw, seed, n, step=(1, 2)):
    base = np.random.RandomState(seed).randint(0, 256, tuple(hw) + (3,)).astype(np.uint8)
    return [np.roll(base, (step[0] * t, step[1] * t), axis=(0, 1)) for t in range(n)]


@pytest.fixture(scope="module")
def pair(dev):
    """A tracked and an untracked detector over the same weights, warmed up."""
    tracked = S.MultiStreamDetector(_model(), HW, max_streams=6, batch=BATCH, device=dev, track=S.TrackConfig(max_tracks=T))
    plain = S.MultiStreamDetector(_model(), HW, max_streams=6, batch=BATCH, device=dev)
    tracked.warm_up(2)
    plain.warm_up(2)
    return tracked, plain


def _specs():
    """Fresh spec OBJECTS of the same four values: a detector keeps one set of output tensors per spec value, so what one test
    left in them is what the next one starts from.  The synthetic weights give low scores: min_score stays low so that the
    ticks' boxes are cropped."""
    return {"f16": sy.CropSpec(size=(16, 24), pad=0.1, dtype=torch.float16, mean=(103.53, 116.28, 123.675), std=(57.375, 57.12, 58.395),
                               max_per_stream=6, fill=(3, 200, 77)),
            "u8": sy.CropSpec(size=(8, 8), keep_aspect=False, dtype=torch.uint8, channel_order="rgb", min_score=0.02, capacity=9),
            "bf16": sy.CropSpec(size=(32, 8), pad=1.0, dtype=torch.bfloat16, channel_order="rgb", std=(255, 255, 255), max_per_stream=3),
            "f32": sy.CropSpec(size=(8, 16), dtype=torch.float32, classes=range(8), max_per_stream=4)}


class Source:
    """A crop source over a pseudo-random backing buffer: what crops() is given, and what the restatement needs of it."""

    def __init__(self, kind, hw, dev, seed):
        h, w = hw
        rng = np.random.RandomState(seed)
        if kind == "tensor":                                         # a plain uint8 [H, W, 3] tensor: BGR
            self.backing = torch.from_numpy(rng.randint(0, 256, size=(h, w * 3)).astype(np.uint8)).to(dev)
            self.source = self.backing.view(h, w, 3)
            self.surface = Surface(self.source, "bgr")
        elif kind == "rgb":                                          # a Surface with a pitch
            self.backing = torch.from_numpy(rng.randint(0, 256, size=(h, w * 3 + 12)).astype(np.uint8)).to(dev)
            self.source = self.surface = Surface.from_buffer(self.backing, h, w, "rgb")
        else:                                                        # "nv12" / "p010": one buffer, the luma plane padded by 8 rows
            step = 2 if kind == "p010" else 1
            self.backing = torch.from_numpy(rng.randint(0, 256, size=(h + 8 + h // 2, w * step + 6)).astype(np.uint8)).to(dev)
            self.source = self.surface = Surface.from_buffer(self.backing, h, w, kind, chroma_row=h + 8)
        self.host = self.backing.cpu().numpy().ravel().copy()

    def row(self, divisor, spec):
        s, base = self.surface, self.backing.data_ptr()
        return dict(fmt=s.format, hs=s.hw[0], ws=s.hw[1], pitch=s.pitch, cpitch=s.chroma_pitch, p0=(0, s.planes[0].data_ptr() - base),
                    p1=(0, s.planes[1].data_ptr() - base) if len(s.planes) == 2 else None, divisor=divisor, min_score=spec.min_score,
                    max_crops=spec.max_per_stream, pad_q8=spec.pad_q8, fill=spec.fill + (0,), mask=spec.class_mask)


NO_ROW = dict(p0=None, hs=0, ws=0, fmt=0)


def _host(crops):
    return [raw(t).copy() for t in (crops.images, crops.index, crops.rect, crops.count)]


def _expect(before, rows, sources, lists, layout, ids, cnt, spec, shape):
    """The four output buffers (bytes) the rule asks for, starting from what they held (`before`)."""
    kind = KIND[spec.dtype]
    out = before[0].copy().view(NP_DTYPE[kind]).reshape(shape)
    index, rect = (b.copy().view(np.int32).reshape(shape[0], 4) for b in before[1:3])
    count = before[3].copy().view(np.int32)
    frames = [None if s is None else frame_of(r, [s.host]) for r, s in zip(rows, sources)]
    restate(rows, frames, lists, layout, ids, cnt, lists.shape[1], spec.flags, kind, spec.mean, spec.scale, out, index, rect, count)
    return [a.view(np.uint8).ravel() for a in (out, index, rect, count)]


def _check_crops(det, res, tick_sids, crop_sids, sources, spec, tag):
    """crops() out of `sources` for `crop_sids` after the tick `res` over `tick_sids`, against the restatement.  -> crops kept"""
    held = det._crop_out.peek(spec) if det._crop_out is not None else None
    before = _host(held) if held is not None else None               # (a spec's first call allocates its tensors, zeroed)
    got = det.crops([s.source for s in sources], crop_sids, spec)
    shape = tuple(got.images.shape)
    if before is None:
        before = [np.zeros(t.numel() * t.element_size(), np.uint8) for t in (got.images, got.index, got.rect, got.count)]
    assert shape == (spec.slots(det.batch), 3) + spec.size and got.images.dtype == spec.dtype and got.count.is_cuda
    rows, per_row = [dict(NO_ROW) for _ in range(det.batch)], [None] * det.batch
    for s, sid in zip(sources, crop_sids):
        b = tick_sids.index(sid)
        rows[b], per_row[b] = s.row(1.0 if det.tracks is not None else det._geom[sid][2], spec), s
        assert got.row_sids[b] == sid
    assert [x for x in got.row_sids if x is not None] == [sid for sid in tick_sids if sid in crop_sids]
    if det.tracks is not None:
        lists, ids, cnt = (t.cpu().numpy() for t in res[-3:])
        want = _expect(before, rows, per_row, lists, 1, ids, cnt, spec, shape)
    else:
        want = _expect(before, rows, per_row, res[0].cpu().numpy(), 0, None, res[1].cpu().numpy(), spec, shape)
    for name, g, w in zip(("images", "index", "rect", "count"), _host(got), want):
        assert np.array_equal(g, w), (tag, name, int((g != w).sum()))
    return int(got.count[0])


@pytest.mark.parametrize("which", ["plain", "tracked"])
def test_crops_equal_the_rule_on_the_ticks_own_tensors(pair, dev, which):
    det = pair[0] if which == "tracked" else pair[1]
    specs = _specs()
    sids = [det.open() for _ in range(3)]
    clips = [_clip(HW, 20 + k, 2) for k in range(3)]
    kept = 0
    for t, (mix, order, kinds, names) in enumerate((([0, 1, 2], [2, 0, 1], ["tensor", "nv12", "rgb"], ["f16", "u8"]),
                                                    ([2, 0], [0], ["p010"], ["f16", "bf16", "f32"]))):
        tick = [sids[k] for k in mix]
        res = det.detect_device([clips[k][t] for k in mix], tick)
        sources = [Source(kind, HW, dev, 30 + i) for i, kind in enumerate(kinds)]
        for name in names:                                           # ("f16" twice: its tensors are reused, stale slots stay as they were)
            kept += _check_crops(det, res, tick, [sids[k] for k in order], sources, specs[name], (which, t, name))
    assert kept > 0                                                  # (the ticks did report boxes, and they were cropped)
    if which == "tracked":
        assert int(det._crop_out.peek(specs["f16"]).index[0, 2]) >= 0     # a track id, not the -1 of plain detections
    for sid in sids:
        det.close(sid)


def test_mixed_mode_two_camera_sizes(dev):
    det = S.MultiStreamDetector(_model(), HW, max_streams=4, batch=3, device=dev, max_frame_hw=HW)
    det.warm_up(2)
    a, b, c = det.open(frame_hw=OTHER), det.open(), det.open(frame_hw=CANVAS)
    frames = [_clip(OTHER, 40, 1)[0], _clip(HW, 41, 1)[0], _clip(CANVAS, 42, 1)[0]]
    res = det.detect_device(frames, [a, b, c])
    assert len(res) == 4 and det._geom[a][2] != det._geom[b][2] != det._geom[c][2]     # three box divisors: 0.64, 0.5, 1
    sources = [Source("nv12", OTHER, dev, 50), Source("tensor", HW, dev, 51), Source("rgb", CANVAS, dev, 52)]
    assert _check_crops(det, res, [a, b, c], [a, b, c], sources, _specs()["f16"], "mixed") > 0
    with pytest.raises(ValueError):                                  # a's camera is 100 x 150
        det.crops([Source("tensor", HW, dev, 53).source], [a])


def test_two_launches_no_host_read_no_allocation_and_the_tick_is_untouched(pair, dev):
    _, det = pair
    a, b = det.open(), det.open()
    clip = _clip(HW, 60, 3)
    tape = det.plan._slots_tape[2]
    size = tape.size()
    source = Source("nv12", HW, dev, 70)
    seen, first = [], None
    for t in range(3):                                               # stream a: a crops() behind every tick
        res = det.detect_device([clip[t]], [a])
        seen.append((res[0][0].clone(), res[1][0].clone()))
        if t == 0:
            first = det.crops([source.source], [a], _specs()["f16"])     # (allocates the outputs, builds the spec's device tables)
            continue
        torch.cuda.synchronize(dev)
        allocated = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        with _lib.NativeTape() as rec:                               # what crops() launches, counted where launches are made
            torch.cuda.set_sync_debug_mode("error")                  # and any synchronising call is an error
            try:
                got = det.crops([source.source], [a], _specs()["f16"])   # a spec built inline, as a caller's loop would: equal by value
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert rec.size()[1] == 2                                    # the plan and the gather
        assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == allocated
        assert got is first and got.count.is_cuda and got.images.is_cuda
        assert int(got.count[0]) > 0
    # the detector keeps the tensors of its few most recently used specs only: specs that vary do not pile up device memory
    for k in range(12):
        det.crops([source.source], [a], sy.CropSpec(size=(8, 8), capacity=1 + k))
    assert len(det._crop_out) <= 4
    for t in range(3):                                               # stream b: the same frames, never cropped
        res = det.detect_device([clip[t]], [b])
        assert torch.equal(res[1][0], seen[t][1]) and int(res[1][0]) > 0
        assert torch.equal(res[0][0, :int(res[1][0])], seen[t][0][:int(res[1][0])])
    assert det.plan._slots_tape[2] is tape and tape.size() == size   # the tick's tape: the same object, the same entries and launches
    det.close(a)
    det.close(b)


def test_value_errors(pair, dev):
    _, det = pair
    a, b, c = det.open(), det.open(), det.open()
    clip = _clip(HW, 80, 2)
    det.detect_device([clip[0], clip[0]], [a, b])
    det.detect_device([clip[1]], [a])                                # the latest tick: a alone
    good = Source("tensor", HW, dev, 81)
    spec = _specs()["u8"]
    got = det.crops([good.source], [a], spec)
    assert int(got.count[0]) > 0
    before = _host(got)
    for sources, sids in (([good.source], [b]),                      # b had no frame in the latest tick
                          ([good.source], [c]),                      # c never had one
                          ([good.source], [12345]),                  # not open
                          ([good.source, good.source], [a, a]),      # a stream named twice
                          ([good.source], [a, b]),                   # one source for two streams
                          ([good.source.cpu()], [a]),                # on another device
                          ([Source("tensor", (64, 96), dev, 82).source], [a]),      # another size
                          ([Source("nv12", (128, 160), dev, 83).source], [a]),
                          ([good.source.float()], [a])):             # not a uint8 tensor
        with pytest.raises(ValueError):
            det.crops(sources, sids, spec)
    with pytest.raises(ValueError):
        det.crops([good.source], [a], spec="small")
    assert all(np.array_equal(x, y) for x, y in zip(_host(got), before))     # nothing was written by the refused calls
    empty = det.crops([], [], spec)                                  # nothing asked for: nothing kept, no launch
    assert empty is got and empty.count.tolist() == [0, 0] and empty.row_sids == (None,) * BATCH
    for sid in (a, b, c):
        det.close(sid)


def test_crop_detections_equals_crops(pair, dev):
    _, det = pair
    a = det.open()
    res = det.detect_device([_clip(HW, 90, 1)[0]], [a])
    source = Source("nv12", HW, dev, 91)
    for name in ("f16", "u8"):
        spec = _specs()[name]
        one = det.crops([source.source], [a], spec)
        n = int(res[1][0])
        rows = res[0][0, :n]
        two = sy.crop_detections(source.source, rows[:, :4] / det._geom[a][2], rows[:, 4] * rows[:, 5], rows[:, 6], spec=spec)
        k = int(one.count[0])
        assert n > 0 and k > 0 and two.count.tolist() == one.count.tolist() and two.row_sids == (None,)
        assert torch.equal(one.images[:k], two.images[:k]) and torch.equal(one.rect[:k], two.rect[:k])
        assert torch.equal(one.index[:k, 1:], two.index[:k, 1:]) and not two.index[:k, 0].any()
    # host arrays and ids, against the restatement
    spec = _specs()["bf16"]
    boxes = (rows[:, :4] / det._geom[a][2]).cpu().numpy()
    scores, labels, ids = (rows[:, 4] * rows[:, 5]).cpu().numpy(), rows[:, 6].cpu().numpy(), (np.arange(n) * 7919).astype(np.int32)
    got = sy.crop_detections(source.source, boxes, scores, labels, ids=ids, spec=spec)
    lists = np.concatenate([boxes, scores[:, None], labels[:, None]], axis=1).astype(np.float32)[None]
    shape = tuple(got.images.shape)
    assert shape[0] == min(n, 3)                                     # capacity=None: room for what the row cap lets through
    zeros = [np.zeros(t.numel() * t.element_size(), np.uint8) for t in (got.images, got.index, got.rect, got.count)]
    want = _expect(zeros, [source.row(1.0, spec)], [source], lists, 1, ids[None], np.array([n]), spec, shape)
    assert all(np.array_equal(g, w) for g, w in zip(_host(got), want)) and int(got.count[0]) > 0
    none = sy.crop_detections(source.source, np.zeros((0, 4)), [], [], spec=spec)
    assert none.count.tolist() == [0, 0]
    det.close(a)


def test_streaming_detector_crops(dev):
    det = S.StreamingDetector(_model(), HW, device=dev)
    source = Source("nv12", HW, dev, 95)
    spec = _specs()["f16"]
    with pytest.raises(ValueError):                                  # no frame yet
        det.crops(source.source, spec)
    before = None
    for t, frame in enumerate(_clip(HW, 96, 2)):                     # the first frame (wrappers) and a taped one
        det(frame)
        source = Source("nv12" if t else "tensor", HW, dev, 97 + t)
        got = det.crops(source.source, spec)
        shape = tuple(got.images.shape)
        if before is None:
            before = [np.zeros(x.numel() * x.element_size(), np.uint8) for x in (got.images, got.index, got.rect, got.count)]
        d, cnt = det._last
        want = _expect(before, [source.row(det.in_scale, spec)], [source], d[:1].cpu().numpy(), 0, None, cnt[:1].cpu().numpy(), spec, shape)
        before = _host(got)
        assert all(np.array_equal(g, w) for g, w in zip(before, want)) and int(got.count[0]) > 0 and got.row_sids == (0,)
    with pytest.raises(ValueError):
        det.crops(Source("tensor", CANVAS, dev, 99).source, spec)

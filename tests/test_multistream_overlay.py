"""MultiStreamDetector.draw / StreamingDetector.draw / sy.draw_detections (streamyolo_amd/overlay.py over csrc/overlay.hip) on the
MI355X with the nano model, 128x192 cameras and batch 4.

The expected pictures come from the restatement of tests/test_overlay_kernel.py (the rendering rule of include/streamyolo_hip.h in
plain numpy) applied to the tick's OWN device tensors — the det / cnt of detect_device, or the tracker's out / out_id / out_cnt —
and are compared byte for byte over the targets' whole backing allocations, which start as pseudo-random bytes."""
import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import _lib
from streamyolo_amd import streaming as S
from streamyolo_amd.data import Surface
from test_overlay_kernel import restate

pytestmark = pytest.mark.gpu

HW, BATCH, T = (128, 192), 4, 32
OTHER, CANVAS = (100, 150), (64, 96)


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


# every box the tick reports is drawn (the synthetic weights give low scores), at most 40 per frame
STYLES = {"id": sy.OverlayStyle(min_score=0.0, max_boxes=40, thickness=1, text_scale=1, show="id"),
          "score": sy.OverlayStyle(min_score=0.02, max_boxes=40, thickness=2, text_scale=1, show="score")}


class Target:
    """A drawing target over a pseudo-random backing buffer: what draw() is given, and what the restatement needs of it."""

    def __init__(self, kind, hw, dev, seed):
        h, w = hw
        rng = np.random.RandomState(seed)
        if kind == "tensor":                                         # a plain uint8 [H, W, 3] tensor: BGR
            self.backing = torch.from_numpy(rng.randint(0, 256, size=(h, w * 3)).astype(np.uint8)).to(dev)
            self.target = self.backing.view(h, w, 3)
            self.surface = Surface(self.target, "bgr")
        elif kind == "rgb":                                          # a Surface with a pitch
            self.backing = torch.from_numpy(rng.randint(0, 256, size=(h, w * 3 + 12)).astype(np.uint8)).to(dev)
            self.target = self.surface = Surface.from_buffer(self.backing, h, w, "rgb")
        else:                                                        # "nv12" / "p010": one buffer, the luma plane padded by 8 rows
            step = 2 if kind == "p010" else 1
            self.backing = torch.from_numpy(rng.randint(0, 256, size=(h + 8 + h // 2, w * step + 6)).astype(np.uint8)).to(dev)
            self.target = self.surface = Surface.from_buffer(self.backing, h, w, kind, chroma_row=h + 8)
        self.before = self.backing.cpu().numpy().ravel().copy()

    def row(self, divisor, style):
        s, base = self.surface, self.backing.data_ptr()
        return dict(fmt=s.format, hs=s.hw[0], ws=s.hw[1], pitch=s.pitch, cpitch=s.chroma_pitch, p0=(0, s.planes[0].data_ptr() - base),
                    p1=(0, s.planes[1].data_ptr() - base) if len(s.planes) == 2 else None, divisor=divisor, min_score=style.min_score,
                    max_boxes=style.max_boxes, thickness=style.thickness, text_scale=style.text_scale, flags=style.flags)

    def check(self, divisor, style, boxes, layout, ids, cnt, tag):
        """The backing buffer now == the restatement over what it was.  -> bytes drawn."""
        want = [self.before.copy()]
        restate(self.row(divisor, style), want, boxes, layout, ids, cnt, boxes.shape[0], (style.palette, style.class_text))
        got = self.backing.cpu().numpy().ravel()
        assert np.array_equal(got, want[0]), (tag, int((got != want[0]).sum()))
        return int((want[0] != self.before).sum())


def _check_draw(det, res, tick_sids, draw_sids, targets, style, tag):
    """draw() into `targets` for `draw_sids` after the tick `res` over `tick_sids`, against the restatement."""
    returned = det.draw([t.target for t in targets], draw_sids, style)
    assert all(a is b.target for a, b in zip(returned, targets))
    if det.tracks is not None:
        out, out_id, out_cnt = (t.cpu().numpy() for t in res[-3:])
    else:
        dets, cnt = res[0].cpu().numpy(), res[1].cpu().numpy()
    drawn = 0
    for t, sid in zip(targets, draw_sids):
        b = tick_sids.index(sid)
        if det.tracks is not None:
            drawn += t.check(1.0, style, out[b], 1, out_id[b], out_cnt[b], (tag, sid))
        else:
            drawn += t.check(det._geom[sid][2], style, dets[b], 0, None, cnt[b], (tag, sid))
    return drawn


@pytest.mark.parametrize("which", ["plain", "tracked"])
def test_draw_equals_the_rule_on_the_ticks_own_tensors(pair, dev, which):
    det = pair[0] if which == "tracked" else pair[1]
    sids = [det.open() for _ in range(3)]
    clips = [_clip(HW, 20 + k, 2) for k in range(3)]
    drawn = 0
    for t, (mix, order, kinds) in enumerate((([0, 1, 2], [2, 0, 1], ["tensor", "nv12", "rgb"]), ([2, 0], [0], ["p010"]))):
        tick = [sids[k] for k in mix]
        res = det.detect_device([clips[k][t] for k in mix], tick)
        targets = [Target(kind, HW, dev, 30 + i) for i, kind in enumerate(kinds)]
        drawn += _check_draw(det, res, tick, [sids[k] for k in order], targets, STYLES["id" if t == 0 else "score"], (which, t))
    assert drawn > 0                                                 # (the ticks did report boxes, and they were drawn)
    for sid in sids:
        det.close(sid)


def test_mixed_mode_two_camera_sizes(dev):
    det = S.MultiStreamDetector(_model(), HW, max_streams=4, batch=3, device=dev, max_frame_hw=HW)
    det.warm_up(2)
    a, b, c = det.open(frame_hw=OTHER), det.open(), det.open(frame_hw=CANVAS)
    frames = [_clip(OTHER, 40, 1)[0], _clip(HW, 41, 1)[0], _clip(CANVAS, 42, 1)[0]]
    res = det.detect_device(frames, [a, b, c])
    assert len(res) == 4 and det._geom[a][2] != det._geom[b][2] != det._geom[c][2]     # three box divisors: 0.64, 0.5, 1
    targets = [Target("nv12", OTHER, dev, 50), Target("tensor", HW, dev, 51), Target("rgb", CANVAS, dev, 52)]
    assert _check_draw(det, res, [a, b, c], [a, b, c], targets, STYLES["score"], "mixed") > 0
    with pytest.raises(ValueError):                                  # a's camera is 100 x 150
        det.draw([Target("tensor", HW, dev, 53).target], [a])


def test_one_launch_no_host_read_and_the_tick_is_untouched(pair, dev):
    _, det = pair
    a, b = det.open(), det.open()
    clip = _clip(HW, 60, 3)
    tape = det.plan._slots_tape[2]
    size = tape.size()
    style = STYLES["score"]
    seen = []
    for t in range(3):                                               # stream a: a draw() behind every tick
        res = det.detect_device([clip[t]], [a])
        seen.append((res[0][0].clone(), res[1][0].clone()))
        target = Target("nv12", HW, dev, 70 + t)
        if t == 0:
            det.draw([target.target], [a], style)                    # (builds the style's device tables: copies from pageable memory)
            continue
        with _lib.NativeTape() as rec:                               # what draw() launches, counted where launches are made
            torch.cuda.set_sync_debug_mode("error")                  # and any synchronising call is an error
            try:
                det.draw([target.target], [a], style)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert rec.size()[1] == 1
        assert target.check(det._geom[a][2], style, res[0][0].cpu().numpy(), 0, None, int(res[1][0]), t) > 0
    for t in range(3):                                               # stream b: the same frames, never drawn
        res = det.detect_device([clip[t]], [b])
        assert torch.equal(res[1][0], seen[t][1]) and int(res[1][0]) > 0
        assert torch.equal(res[0][0, :int(res[1][0])], seen[t][0][:int(res[1][0])])
    assert det.plan._slots_tape[2] is tape and tape.size() == size   # the tick's tape: the same object, the same launches
    det.close(a)
    det.close(b)


def test_value_errors(pair, dev):
    _, det = pair
    a, b, c = det.open(), det.open(), det.open()
    clip = _clip(HW, 80, 2)
    det.detect_device([clip[0], clip[0]], [a, b])
    det.detect_device([clip[1]], [a])                                # the latest tick: a alone
    good = Target("tensor", HW, dev, 81)
    before = good.backing.clone()
    for targets, sids in (([good.target], [b]),                      # b had no frame in the latest tick
                          ([good.target], [c]),                      # c never had one
                          ([good.target], [12345]),                  # not open
                          ([good.target, good.target], [a, a]),      # a stream named twice
                          ([good.target], [a, b]),                   # one target for two streams
                          ([good.target.cpu()], [a]),                # on another device
                          ([Target("tensor", (64, 96), dev, 82).target], [a]),      # another size
                          ([Target("nv12", (128, 160), dev, 83).target], [a]),
                          ([good.target.float()], [a])):             # not a uint8 tensor
        with pytest.raises(ValueError):
            det.draw(targets, sids)
    with pytest.raises(ValueError):
        det.draw([good.target], [a], style="thick")
    assert torch.equal(good.backing, before)                         # nothing was written by the refused calls
    det.draw([good.target], [a], STYLES["id"])
    assert not torch.equal(good.backing, before)
    for sid in (a, b, c):
        det.close(sid)


def test_draw_detections_equals_draw(pair, dev):
    _, det = pair
    a = det.open()
    res = det.detect_device([_clip(HW, 90, 1)[0]], [a])
    style = STYLES["score"]
    one, two = Target("tensor", HW, dev, 91), Target("tensor", HW, dev, 91)
    det.draw([one.target], [a], style)
    n = int(res[1][0])
    rows = res[0][0, :n]
    back = sy.draw_detections(two.target, rows[:, :4] / det._geom[a][2], rows[:, 4] * rows[:, 5], rows[:, 6], style=style)
    assert back is two.target and n > 0
    assert torch.equal(one.backing, two.backing) and not torch.equal(one.backing, torch.from_numpy(one.before).to(dev).view_as(one.backing))
    # host arrays and ids: the same picture as the restatement's
    three = Target("p010", HW, dev, 92)
    boxes = (rows[:, :4] / det._geom[a][2]).cpu().numpy()
    scores, labels, ids = (rows[:, 4] * rows[:, 5]).cpu().numpy(), rows[:, 6].cpu().numpy(), np.arange(n) * 7919
    sy.draw_detections(three.target, boxes, scores, labels, ids=ids, style=STYLES["id"])
    lists = np.concatenate([boxes, scores[:, None], labels[:, None]], axis=1).astype(np.float32)
    assert three.check(1.0, STYLES["id"], lists, 1, ids.astype(np.int32), n, "host arrays") > 0
    det.close(a)


def test_streaming_detector_draw(dev):
    det = S.StreamingDetector(_model(), HW, device=dev)
    target = Target("nv12", HW, dev, 95)
    with pytest.raises(ValueError):                                  # no frame yet
        det.draw(target.target)
    style = STYLES["score"]
    for t, frame in enumerate(_clip(HW, 96, 2)):                     # the first frame (wrappers) and a taped one
        det(frame)
        target = Target("nv12" if t else "tensor", HW, dev, 97 + t)
        assert det.draw(target.target, style) is target.target
        d, cnt = det._last
        assert target.check(det.in_scale, style, d[0].cpu().numpy(), 0, None, int(cnt[0]), t) > 0
    with pytest.raises(ValueError):
        det.draw(Target("tensor", CANVAS, dev, 99).target, style)

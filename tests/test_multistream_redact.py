"""MultiStreamDetector.redact / StreamingDetector.redact / sy.redact_detections (streamyolo_amd/redact.py over csrc/redact.hip) on
the MI355X with the nano model, 128x192 cameras and batch 4.

The expected frames come from the restatement of tests/test_redact_kernel.py (the rule of include/streamyolo_hip.h in plain numpy,
computed from the ORIGINAL bytes) applied to the tick's OWN device tensors — the det / cnt of detect_device, or the tracker's out
/ out_cnt — and are compared byte for byte over the targets' whole backing allocations, which start as pseudo-random bytes.  The
synthetic weights give low scores and few boxes: the specs use min_score = 0.0, and every detector's run must have covered
pixels in at least one target — it FAILS otherwise, it does not skip."""
import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import _lib
from streamyolo_amd import streaming as S
from streamyolo_amd.data import Surface
from test_overlay_kernel import restate as restate_draw
from test_redact_kernel import restate

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


# every box the tick reports is redacted (the synthetic weights give low scores)
SPECS = {"pixelate": sy.RedactSpec(mode="pixelate", cell=8, shape="ellipse", pad=0.1, min_score=0.0),
         "fill": sy.RedactSpec(mode="fill", cell=16, shape="rect", pad=0.25, min_score=0.0, fill=(10, 200, 90)),
         "coarse": sy.RedactSpec(mode="pixelate", cell=32, shape="rect", pad=0.0, min_score=0.0)}
STYLE = sy.OverlayStyle(min_score=0.0, max_boxes=40, thickness=1, text_scale=1, show="score")


class Target:
    """A redaction target over a pseudo-random backing buffer: what redact() is given, and what the restatement needs of it."""

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

    def _geometry(self, divisor):
        s, base = self.surface, self.backing.data_ptr()
        return dict(fmt=s.format, hs=s.hw[0], ws=s.hw[1], pitch=s.pitch, cpitch=s.chroma_pitch, p0=(0, s.planes[0].data_ptr() - base),
                    p1=(0, s.planes[1].data_ptr() - base) if len(s.planes) == 2 else None, divisor=divisor)

    def row(self, divisor, spec):
        return dict(self._geometry(divisor), min_score=spec.min_score, pad_q8=spec.pad_q8, mode=spec.mode_code, cell=spec.cell,
                    shape=spec.shape_code, fill=spec.fill_bytes, mask=spec.class_mask)

    def draw_row(self, divisor, style):
        return dict(self._geometry(divisor), min_score=style.min_score, max_boxes=style.max_boxes, thickness=style.thickness,
                    text_scale=style.text_scale, flags=style.flags)

    def expect(self, divisor, spec, boxes, layout, cnt):
        """The restatement over what the backing buffer was.  -> (the expected bytes, covered pixels)."""
        want = [self.before.copy()]
        covered = restate(self.row(divisor, spec), [self.before], want, boxes, layout, cnt, boxes.shape[0])
        return want[0], covered

    def check(self, divisor, spec, boxes, layout, cnt, tag):
        """The backing buffer now == the restatement over what it was.  -> covered pixels."""
        want, covered = self.expect(divisor, spec, boxes, layout, cnt)
        got = self.backing.cpu().numpy().ravel()
        assert np.array_equal(got, want), (tag, int((got != want).sum()))
        assert (covered > 0) == bool((want != self.before).any()), tag
        return covered


def _lists(det, res):
    """The tick's own device tensors as numpy: (boxes [B, L, 6 | 7], layout, cnt [B])."""
    if det.tracks is not None:
        return res[-3].cpu().numpy(), 1, res[-1].cpu().numpy()
    return res[0].cpu().numpy(), 0, res[1].cpu().numpy()


def _check_redact(det, res, tick_sids, redact_sids, targets, spec, tag):
    """redact() of `targets` for `redact_sids` after the tick `res` over `tick_sids`, against the restatement."""
    returned = det.redact([t.target for t in targets], redact_sids, spec)
    assert all(a is b.target for a, b in zip(returned, targets))
    boxes, layout, cnt = _lists(det, res)
    covered = 0
    for t, sid in zip(targets, redact_sids):
        b = tick_sids.index(sid)
        covered += t.check(1.0 if det.tracks is not None else det._geom[sid][2], spec, boxes[b], layout, cnt[b], (tag, sid))
    return covered


@pytest.mark.parametrize("which", ["plain", "tracked"])
def test_redact_equals_the_rule_on_the_ticks_own_tensors(pair, dev, which):
    det = pair[0] if which == "tracked" else pair[1]
    sids = [det.open() for _ in range(3)]
    clips = [_clip(HW, 20 + k, 2) for k in range(3)]
    covered = 0
    for t, (mix, order, kinds) in enumerate((([0, 1, 2], [2, 0, 1], ["tensor", "nv12", "rgb"]), ([2, 0], [0], ["p010"]))):
        tick = [sids[k] for k in mix]
        res = det.detect_device([clips[k][t] for k in mix], tick)
        targets = [Target(kind, HW, dev, 30 + i) for i, kind in enumerate(kinds)]
        covered += _check_redact(det, res, tick, [sids[k] for k in order], targets, SPECS["pixelate" if t == 0 else "fill"], (which, t))
    assert covered > 0                                               # (the ticks did report boxes, and they were redacted)
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
    assert _check_redact(det, res, [a, b, c], [a, b, c], targets, SPECS["coarse"], "mixed") > 0
    with pytest.raises(ValueError):                                  # a's camera is 100 x 150
        det.redact([Target("tensor", HW, dev, 53).target], [a])


def test_one_launch_no_host_read_and_the_tick_is_untouched(pair, dev):
    _, det = pair
    a, b = det.open(), det.open()
    clip = _clip(HW, 60, 3)
    tape = det.plan._slots_tape[2]
    size = tape.size()
    spec = SPECS["pixelate"]
    seen = []
    for t in range(3):                                               # stream a: a redact() behind every tick
        res = det.detect_device([clip[t]], [a])
        seen.append((res[0][0].clone(), res[1][0].clone()))
        target = Target("nv12", HW, dev, 70 + t)
        if t == 0:
            det.redact([target.target], [a], spec)                   # (allocates the table and its pinned mirrors)
            continue
        with _lib.NativeTape() as rec:                               # what redact() launches, counted where launches are made
            torch.cuda.set_sync_debug_mode("error")                  # and any synchronising call is an error
            try:
                det.redact([target.target], [a], spec)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert rec.size()[1] == 1
        assert target.check(det._geom[a][2], spec, res[0][0].cpu().numpy(), 0, int(res[1][0]), t) > 0
    for t in range(3):                                               # stream b: the same frames, never redacted
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
            det.redact(targets, sids)
    for spec in ("pixelate", STYLE, sy.CropSpec()):                  # not a RedactSpec
        with pytest.raises(ValueError):
            det.redact([good.target], [a], spec=spec)
    assert torch.equal(good.backing, before)                         # nothing was written by the refused calls
    assert det.redact([], []) == []
    det.redact([good.target], [a], SPECS["fill"])
    assert not torch.equal(good.backing, before)
    for sid in (a, b, c):
        det.close(sid)


def test_redact_detections_equals_redact(pair, dev):
    _, det = pair
    a = det.open()
    res = det.detect_device([_clip(HW, 90, 1)[0]], [a])
    spec = SPECS["pixelate"]
    one, two = Target("tensor", HW, dev, 91), Target("tensor", HW, dev, 91)
    det.redact([one.target], [a], spec)
    n = int(res[1][0])
    rows = res[0][0, :n]
    back = sy.redact_detections(two.target, rows[:, :4] / det._geom[a][2], rows[:, 4] * rows[:, 5], rows[:, 6], spec=spec)
    assert back is two.target and n > 0
    assert torch.equal(one.backing, two.backing) and not torch.equal(one.backing, torch.from_numpy(one.before).to(dev).view_as(one.backing))
    # host arrays, every surface kind: the same frame as the restatement's
    boxes = (rows[:, :4] / det._geom[a][2]).cpu().numpy()
    scores, labels = (rows[:, 4] * rows[:, 5]).cpu().numpy(), rows[:, 6].cpu().numpy()
    lists = np.concatenate([boxes, scores[:, None], labels[:, None]], axis=1).astype(np.float32)
    for i, (kind, name) in enumerate((("p010", "fill"), ("nv12", "coarse"), ("rgb", "pixelate"))):
        t = Target(kind, HW, dev, 92 + i)
        sy.redact_detections(t.target, boxes, scores, labels, spec=SPECS[name])
        assert t.check(1.0, SPECS[name], lists, 1, n, ("host arrays", kind)) > 0
    with pytest.raises(ValueError):
        sy.redact_detections(one.target, boxes, scores[:-1], labels)
    with pytest.raises(ValueError):
        sy.redact_detections(one.target, boxes, scores, labels, spec=STYLE)
    assert sy.redact_detections(one.target, np.zeros((0, 4)), [], []) is one.target
    det.close(a)


def test_redact_then_draw(pair, dev):
    """redact() and then draw() on the same clone == the restated redaction followed by the restated drawing."""
    for det in pair:
        sids = [det.open() for _ in range(3)]
        clips = [_clip(HW, 20 + k, 2) for k in range(3)]
        total, drawn = 0, 0
        for tick in range(2):
            res = det.detect_device([c[tick] for c in clips], sids)
            boxes, layout, cnt = _lists(det, res)
            ids = res[-2].cpu().numpy() if det.tracks is not None else None
            targets = [Target(kind, HW, dev, 100 + i) for i, kind in enumerate(("nv12", "tensor", "p010"))]
            det.redact([t.target for t in targets], sids, SPECS["coarse"])
            det.draw([t.target for t in targets], sids, STYLE)
            for b, (t, sid) in enumerate(zip(targets, sids)):
                divisor = 1.0 if det.tracks is not None else det._geom[sid][2]
                want, covered = t.expect(divisor, SPECS["coarse"], boxes[b], layout, cnt[b])
                redacted = want.copy()
                want = [want]
                restate_draw(t.draw_row(divisor, STYLE), want, boxes[b], layout, None if ids is None else ids[b], cnt[b], boxes.shape[1],
                             (STYLE.palette, STYLE.class_text))
                assert np.array_equal(t.backing.cpu().numpy().ravel(), want[0]), (det.tracks is not None, tick, b)
                total += covered
                drawn += int((want[0] != redacted).sum())
        assert total > 0 and drawn > 0
        for sid in sids:
            det.close(sid)


def test_streaming_detector_redact(dev):
    det = S.StreamingDetector(_model(), HW, device=dev)
    target = Target("nv12", HW, dev, 95)
    with pytest.raises(ValueError):                                  # no frame yet
        det.redact(target.target)
    spec = SPECS["fill"]
    for t, frame in enumerate(_clip(HW, 96, 2)):                     # the first frame (wrappers) and a taped one
        det(frame)
        target = Target("nv12" if t else "tensor", HW, dev, 97 + t)
        assert det.redact(target.target, spec) is target.target
        d, cnt = det._last
        assert target.check(det.in_scale, spec, d[0].cpu().numpy(), 0, int(cnt[0]), t) > 0
    with pytest.raises(ValueError):
        det.redact(Target("tensor", CANVAS, dev, 99).target, spec)
    with pytest.raises(ValueError):
        det.redact(target.target, spec="fill")

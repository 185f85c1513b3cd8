"""Per-stream detection policies of MultiStreamDetector (policy=, open(policy=), set_policy) and StreamingDetector(policy=): the
tape holds sy_postprocess_rows, each tick's rows carry their streams' sy_det_policy records (engine.PolicyTable).  The set-up is
tests/test_multistream.py's: nano model, 128x192 frames, fp32.  Expected values come from plain detectors (the existing
sy_postprocess path) built with the same thresholds, bit for bit, and from ops.postprocess_rows on the plan's own output."""
import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import ops
from streamyolo_amd import streaming as S

HW = (128, 192)


def _model(seed=0):
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    cfg = O.OracleConfig.named("nano")
    model = sy.build_model("nano")
    model.load_state_dict(synth_state_dict(O.param_shapes(cfg), seed=seed, bn_stats=load_bn_stats("nano")), strict=True)
    return model


def _frames(seed, n):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, HW + (3,)).astype(np.uint8) for _ in range(n)]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] is None


def _detector(backend, **kw):
    det = S.MultiStreamDetector(_model(), HW, max_streams=3, batch=3, dtype="fp32", device=backend, **kw)
    det.warm_up(2)
    return det


# ---- 10 (a) + (c) --------------------------------------------------------------------------------------------------------------
def test_two_streams_two_policies_one_tick(backend):
    """Two streams with different thresholds in the same ticks == two plain detectors built with those thresholds; a detector
    built with policy=True whose streams never get a policy == the detector built without."""
    frames = [_frames(10 + t, 2) for t in range(2)]
    plain = _detector(backend)
    ids = [plain.open(), plain.open()]
    base = [plain(f, ids) for f in frames]                                       # conf 0.01 / nms 0.65: the existing path
    scores = np.concatenate([r[1] for tick in base for r in tick])
    assert scores.size > 4
    conf2 = float(np.median(scores))                                             # a threshold that really cuts
    strict = _detector(backend, conf_thre=conf2, nms_thresh=0.45)
    ids = [strict.open(), strict.open()]
    high = [strict(f, ids) for f in frames]

    det = _detector(backend, policy=True)
    a, b = det.open(), det.open(policy=sy.DetectionPolicy(conf_thre=conf2, nms_thresh=0.45))
    tape = det.plan._slots_tape[2]
    got = [det(f, [a, b]) for f in frames]
    assert det.plan._slots_tape[2] is tape
    for t in range(2):
        assert _same(got[t][0], base[t][0]) and _same(got[t][1], high[t][1]), t
    assert sum(len(r[0][0]) for r in got) > 0 and sum(len(r[1][0]) for r in got) > 0
    assert any(not _same(base[t][1], high[t][1]) for t in range(2))              # the two policies differ in effect
    # (c) policy=True and no per-stream policy anywhere
    quiet = _detector(backend, policy=True)
    ids = [quiet.open(), quiet.open()]
    for t, f in enumerate(frames):
        res = quiet(f, ids)
        assert _same(res[0], base[t][0]) and _same(res[1], base[t][1]), t
    # rows without a frame report nothing: one stream in a tick of batch 3
    d, c, n = quiet.detect_device(frames[0][:1], ids[:1])
    assert n == 1 and c[1:].cpu().tolist() == [0, 0]


# ---- 10 (b) + 9 ----------------------------------------------------------------------------------------------------------------
def test_set_policy_between_ticks_keeps_the_tape(backend):
    det = _detector(backend, policy=sy.DetectionPolicy())
    tape = det.plan._slots_tape[2]
    n_launch = tape.size()
    sid = det.open()
    frames = _frames(30, 4)
    first = det([frames[0]], [sid])[0]
    assert len(first[0]) > 2
    # stream state matters, so the expectations come from the rows call on what the plan itself produced in that tick
    def expect(policy):
        rec = policy.record(8, 0.01, 0.65)
        d, _, c = ops.postprocess_rows(det.plan.out[:1].clone(), 8, ops.det_policy_table([rec], backend))
        return S._parse(d, c, 0.5)
    cls = int(np.bincount(first[2]).argmax())
    for t, pol in enumerate([sy.DetectionPolicy(classes=[cls]), sy.DetectionPolicy(max_det=2, class_agnostic=True),
                             sy.DetectionPolicy(conf_thre=float(np.median(first[1])))]):
        det.set_policy(sid, pol)
        got = det([frames[1 + t]], [sid])[0]
        assert det.plan._slots_tape[2] is tape and tape.size() == n_launch
        assert _same(got, expect(pol)), t
        assert not _same(got, expect(sy.DetectionPolicy())), t
    assert set(det([frames[0]], [sid])[0][2].tolist()) != {cls}                  # (the last policy, not the first, is in force)
    det.set_policy(sid, sy.DetectionPolicy(classes=[cls]))
    assert set(det([frames[0]], [sid])[0][2].tolist()) == {cls}
    # a rejected policy changes nothing: table bytes, host records, tape
    before, rec = det.policies.table.clone(), det._pol[sid]
    for bad in (lambda: det.set_policy(sid, sy.DetectionPolicy(classes=[8])), lambda: det.set_policy(sid, "strict"),
                lambda: det.set_policy(12345, sy.DetectionPolicy()), lambda: det.open(policy=sy.DetectionPolicy(classes=[99])),
                lambda: det.set_policy(sid, sy.DetectionPolicy(conf_thre=float("nan")))):
        with pytest.raises(ValueError):
            bad()
    assert torch.equal(det.policies.table, before) and det._pol[sid] is rec and len(det._slot_of) == 1
    assert det.plan._slots_tape[2] is tape
    det.set_policy(sid, None)                                                    # back to the detector's own
    assert det._pol[sid] == sy.DetectionPolicy().record(8, 0.01, 0.65)
    with pytest.raises(ValueError):
        S.MultiStreamDetector(_model(), HW, batch=1, dtype="fp32", device=backend, policy=sy.DetectionPolicy(classes=[8]))


# ---- 10 (d) --------------------------------------------------------------------------------------------------------------------
def test_tracker_consumes_the_policy_rows(backend):
    pol = sy.DetectionPolicy(class_agnostic=True, max_det=6)
    det = _detector(backend, policy=True, track=True)
    sid = det.open(policy=pol)
    for t, f in enumerate(_frames(50, 3)):
        d, c, n, out, out_id, out_cnt = det.detect_device([f], [sid], frame_idx=[t])
        want = ops.postprocess_rows(det.plan.out.clone(), 8, ops.det_policy_table([pol.record(8, 0.01, 0.65)] + [ops.det_policy_record(0, 0, [])] * 2, backend))
        k = int(c[0])
        assert n == 1 and 0 < k <= 6 and c.cpu().tolist() == want[2].cpu().tolist()
        assert torch.equal(d[0, :k], want[0][0, :k])
        if t == 0:
            assert int(out_cnt[0]) <= k                                          # the tracker saw those rows and no others


# ---- 10 (e) --------------------------------------------------------------------------------------------------------------------
def test_policies_need_a_detector_built_for_them(backend):
    det = _detector(backend)
    with pytest.raises(ValueError):
        det.open(policy=sy.DetectionPolicy(max_det=5))
    assert not det._slot_of and len(det._free) == 3                              # no slot was taken
    sid = det.open()
    with pytest.raises(ValueError):
        det.set_policy(sid, sy.DetectionPolicy(max_det=5))
    with pytest.raises(ValueError):
        det.set_policy(sid, None)
    assert det.policies is None and not det._pol


# ---- StreamingDetector ---------------------------------------------------------------------------------------------------------
def test_streaming_detector_with_a_policy(backend):
    """The single-camera detector with a policy: the first frame (through the wrappers) and the taped frames give what the rows
    call gives on the plan's output of that frame, and the plain detector's detections of that class lead the list."""
    frames = _frames(70, 3)
    plain = S.StreamingDetector(_model(), HW, dtype="fp32", device=backend)
    base = [plain(f) for f in frames]
    cls = int(np.bincount(np.concatenate([r[2] for r in base])).argmax())
    pol = sy.DetectionPolicy(classes=[cls], max_det=3)
    det = S.StreamingDetector(_model(), HW, dtype="fp32", device=backend, policy=pol)
    table = ops.det_policy_table([pol.record(8, 0.01, 0.65)], backend)
    total = 0
    for f, want in zip(frames, base):
        got = det(f)
        d, _, c = ops.postprocess_rows(det.plan.out.clone(), 8, table)
        assert _same(got, S._parse(d, c, 0.5))
        assert len(got[2]) <= 3 and set(got[2].tolist()) <= {cls}
        assert len(got[2]) == min(3, int((want[2] == cls).sum()))
        assert np.array_equal(got[1][:1], want[1][want[2] == cls][:1])           # the best box of the class is the same box
        total += len(got[2])
    assert total > 0

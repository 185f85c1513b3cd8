"""MultiStreamDetector(track=...): the tracker launch (csrc/track.hip) behind the NMS on the tick's tape, on the MI355X with the
nano model, 128x192 cameras and batch 4.

The expected tracks come from the restatement of tests/test_track_kernel.py fed with the detector's OWN detections (the det / cnt
device tensors of the tick), under the same bounds.  Real detections may come too close to call in fp32 (the input condition of
that file): such a tick's comparison is skipped and the stream restarted, and at most 1 tick in 10 may be skipped."""
import numpy as np
import pytest
import torch

from streamyolo_amd import _lib
from streamyolo_amd import streaming as S
from test_track_kernel import MARGIN, NP64, TH32, Restatement, f32

pytestmark = pytest.mark.gpu

HW, BATCH, T = (128, 192), 4, 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.use_library(_lib.DEFAULT_PATH)
    return torch.device("cuda:0")


def _model():
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    sd = synth_state_dict(O.param_shapes(O.OracleConfig.named("nano")), seed=0, bn_stats=load_bn_stats("nano"))
    model = sy.build_model("nano")
    model.load_state_dict(sd, strict=True)
    return model


def _clip(hw, seed, n, step=(1, 2)):
    """n frames of one camera: a random image drifting by `step` pixels per frame, so that detections persist and move."""
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


class Mirror:
    """Both restatements beside a tracked detector: compare() checks one tick of detect_device against them."""

    def __init__(self):
        self.ref, self.r32 = Restatement(NP64, T), Restatement(TH32, T)
        self.ticks = self.skipped = 0
        self.err_k = self.err_32 = 0.0

    def compare(self, det, res, sids, firsts, dts, horizon, tag=None):
        """-> the streams whose tick was too close to call (their comparison is skipped; the caller restarts them)."""
        dets, cnt, n = res[0].cpu().numpy(), res[1].cpu().numpy(), res[2]
        out, out_id, out_cnt = (t.cpu().numpy() for t in res[-3:])
        close = []
        for b, sid in enumerate(sids):
            (h, w), _, div = det._geom[sid]
            args = (sid, firsts[b], dets[b, :cnt[b]], dts[b], f32(horizon), f32(w), f32(h), f32(div))
            self.ref.iou_margin, self.ref.clean_ok = np.inf, True
            want, w32 = self.ref.update(*args), self.r32.update(*args)
            self.ticks += 1
            if not (self.ref.iou_margin > MARGIN and self.ref.clean_ok):
                self.skipped += 1
                close.append(sid)
                continue
            k = len(want["id"])
            assert out_cnt[b] == k, (tag, b)
            assert out_id[b, :k].tolist() == want["id"] == w32["id"], (tag, b)
            assert out[b, :k, 5].tolist() == want["label"] and out[b, :k, 4].tolist() == [float(v) for v in want["score"]]
            ek, e32 = np.abs(out[b, :k, :4] - want["box"]).max(initial=0.0), np.abs(w32["box"] - want["box"]).max(initial=0.0)
            assert ek <= max(4.0 * e32, 1e-3), (tag, b, ek, e32)
            assert (out[b, :k, 0] >= 0).all() and (out[b, :k, 2] <= w).all() and (out[b, :k, 1] >= 0).all() and (out[b, :k, 3] <= h).all()
            self.err_k, self.err_32 = max(self.err_k, ek), max(self.err_32, e32)
        return close

    def restart(self, sid):
        self.ref.slots.pop(sid, None)
        self.r32.slots.pop(sid, None)


def test_tracking_changes_no_detection_and_adds_one_launch(pair):
    tracked, plain = pair
    ta, pa = [tracked.open() for _ in range(3)], [plain.open() for _ in range(3)]
    clips = [_clip(HW, 10 + k, 3) for k in range(3)]
    tape_t, tape_p = tracked.plan._slots_tape[2], plain.plan._slots_tape[2]
    assert tape_t.size()[1] == tape_p.size()[1] + 1              # the tracker: exactly one more launch
    for t, mix in enumerate(([0, 1, 2], [2, 0], [1])):           # another mix of streams (and of first frames) every tick
        frames = [clips[k][t] for k in mix]
        rt = tracked.detect_device(frames, [ta[k] for k in mix])
        rp = plain.detect_device(frames, [pa[k] for k in mix])
        assert len(rt) == len(rp) + 3 and rt[2] == rp[2] == len(mix)
        cnt_t, cnt_p = rt[1].cpu(), rp[1].cpu()
        assert torch.equal(cnt_t[:len(mix)], cnt_p[:len(mix)]) and int(cnt_t[:len(mix)].min()) > 0
        for b in range(len(mix)):
            assert torch.equal(rt[0][b, :cnt_t[b]].cpu(), rp[0][b, :cnt_p[b]].cpu())
    assert tracked.plan._slots_tape[2] is tape_t and plain.plan._slots_tape[2] is tape_p        # nothing was re-recorded
    for sid in ta:
        tracked.close(sid)
    for sid in pa:
        plain.close(sid)


def test_tracks_equal_the_restatement_on_the_detectors_own_detections(pair):
    from conftest import record_parity
    det, _ = pair
    sids = [det.open() for _ in range(3)]
    clips = {sid: _clip(HW, 20 + k, 12, step=(1 + k, 2)) for k, sid in enumerate(sids)}
    m, prev, fresh, matched = Mirror(), {}, set(sids), 0
    # 12 frame times; stream 1 skips every third frame (dt = 2 afterwards), stream 2 joins late; rows change with the mix
    for t in range(12):
        mix = [s for k, s in enumerate(sids) if not (k == 1 and t % 3 == 1) and not (k == 2 and t < 2)]
        if t % 2:
            mix = mix[::-1]
        firsts = [s in fresh for s in mix]
        dts = [0 if s in fresh else t - prev[s] for s in mix]
        res = det.detect_device([clips[s][t] for s in mix], mix, frame_idx=[t] * len(mix), horizon=1.0)
        close = m.compare(det, res, mix, firsts, dts, 1.0, tag=t)
        fresh -= set(mix)
        for s in mix:
            prev[s] = t
        for s in close:                                          # too close to call: this stream starts over on both sides
            det.reset(s)
            m.restart(s)
            fresh.add(s)
        matched += sum(m.ref.slot(s)["n_matched"] for s in mix)
    print("tracked ticks %d, skipped %d, kernel err %.3g px, float32 restatement err %.3g px" % (m.ticks, m.skipped, m.err_k, m.err_32))
    assert 10 * m.skipped <= m.ticks
    assert matched > 0                                           # the clips do produce persisting tracks
    record_parity("track_kf_multistream", kernel_err_px=m.err_k, float32_restatement_err_px=m.err_32, ticks=m.ticks, skipped=m.skipped)
    for s in sids:
        det.close(s)


def test_validation_and_reset(pair):
    det, _ = pair
    a, b = det.open(), det.open()
    clip = _clip(HW, 30, 4)
    det([clip[0], clip[0]], [a, b], frame_idx=[5, 5])
    r = det([clip[1]], [a])                                      # default index: the previous one + 1
    assert det._fidx[a] == 6 and len(r) == 1 and len(r[0]) == 5 and r[0][3] is None
    assert r[0][0].shape == (len(r[0][4]), 4) and r[0][2].dtype == np.int32
    before = [t.clone() for t in det.tracks.state.tensors()]
    marks = (dict(det._fidx), dict(det._first))
    for bad in ([6, 6], [7, 4]):                                 # a repeated index, an index going backwards (second frame)
        with pytest.raises(ValueError, match="does not follow"):
            det([clip[2], clip[2]], [a, b], frame_idx=bad)
    with pytest.raises(ValueError):
        det([clip[2]], [a], horizon=[1.0, 2.0])
    assert all(torch.equal(x, y) for x, y in zip(before, det.tracks.state.tensors())) and marks == (det._fidx, det._first)
    # forecast: horizon 0 repeats the last output of the stream; a closed id is refused
    last = det([clip[2]], [a], frame_idx=[8])[0]
    again = det.forecast([a], 0.0)[0]
    assert all(np.array_equal(x, y) for x, y in zip(last[:3] + last[4:], again[:3] + again[4:]))
    moved = det.forecast([a, b], [3.0, 0.0])
    assert len(moved) == 2 and len(moved[0]) == 5
    hdr = det.tracks.state.hdr.cpu().numpy()[det._slot_of[a]]
    assert hdr[2] > 0
    det.reset(a)                                                 # a new sequence: ids restart, whatever the index
    det([clip[3]], [a], frame_idx=[0])
    hdr = det.tracks.state.hdr.cpu().numpy()[det._slot_of[a]]
    assert hdr[1] == 0 and hdr[2] == hdr[0] > 0
    det.close(b)
    with pytest.raises(ValueError, match="not open"):
        det.forecast([b], 1.0)
    det.close(a)


def test_mixed_cameras_are_clipped_to_their_own_size(dev):
    """Two camera sizes in one tick: every row's boxes are in its own camera's coordinates and clipped to its own size."""
    small = (96, 128)
    det = S.MultiStreamDetector(_model(), HW, max_streams=3, batch=2, device=dev, max_frame_hw=(160, 256),
                                track=S.TrackConfig(max_tracks=T))
    det.warm_up(2)
    a, b = det.open(), det.open(frame_hw=small)
    ca, cb = _clip(HW, 40, 3), _clip(small, 41, 3)
    m, fresh = Mirror(), {a, b}
    for t in range(3):
        res = det.detect_device([cb[t], ca[t]], [b, a], horizon=2.0)
        assert len(res) == 7                                     # det, cnt, rows, div, out, out_id, out_cnt
        close = m.compare(det, res, [b, a], [s in fresh for s in (b, a)], [0 if s in fresh else 1 for s in (b, a)], 2.0, tag=t)
        fresh = set(close)                                       # (compare asserts each row's own bounds)
        for s in close:
            det.reset(s)
            m.restart(s)
        tick = det.tracks.ticks.cpu().numpy().view(np.dtype(_lib.TrackTick))
        assert (tick["img_w"][0], tick["img_h"][0]) == (128.0, 96.0) and (tick["img_w"][1], tick["img_h"][1]) == (192.0, 128.0)
        assert tick["divisor"][0] == np.float32(det._geom[b][2]) and tick["divisor"][1] == np.float32(0.5)
    assert m.skipped <= 1 and m.ticks == 6
    out, cnt = det.tracks.out.cpu().numpy(), det.tracks.out_cnt.cpu().numpy()
    assert cnt[0] > 0 and cnt[1] > 0 and out[0, :cnt[0], 2].max() <= 128.0 and out[0, :cnt[0], 3].max() <= 96.0


def test_without_track_nothing_changes(pair):
    _, plain = pair
    s = plain.open()
    clip = _clip(HW, 50, 1)
    r = plain([clip[0]], [s])
    assert len(r) == 1 and len(r[0]) == 4 and r[0][3] is None
    assert len(plain.detect_device([clip[0]], [s])) == 3
    with pytest.raises(ValueError, match="track"):
        plain([clip[0]], [s], frame_idx=[3])
    with pytest.raises(ValueError, match="track"):
        plain.forecast([s], 1.0)
    plain.close(s)

"""sy_track_update / sy_track_forecast (csrc/track.hip) on hand-made detections, on the SIMT emulator and on the MI355X.

The yardstick is `Restatement` below: the tick as include/streamyolo_hip.h and DESIGN.md describe it (reset, predict, truncate,
greedy IoU association, rebuild, forecast, clean-up), written once over a tiny array adapter and run twice — in float64 numpy
(the truth) and in float32 torch on the CPU (what honest fp32 arithmetic in another summation order gives).

* Association, ids, labels, scores, counts and the kept set must be IDENTICAL to the float64 run.  To make that a fair demand of
  fp32 every tick first asserts a condition on ITS OWN INPUTS, computed in float64: apart from exact ties (equal to the last
  bit, constructed from integer boxes) the IoU of every candidate pair is more than 1e-3 away from the threshold and the
  winner more than 1e-3 above its runner-up; and every box that reaches the clean-up either consists of float32-exact numbers
  only (then fp32 computes the very same w, h) or has w, h more than 1e-3 away from 0 and a clipped w, h whose int(w) * int(h)
  stays on its side of min_size when both move by 1e-3 either way (then the decision cannot come out differently).
* Box values (the forecast output and the stored state x): max |kernel - float64| <= max(4 x max |float32 run - float64|, 1e-3
  px) per tick; the factor covers another, equally valid summation order in F P F' and S^-1."""
import numpy as np
import pytest
import torch

from conftest import record_parity
from streamyolo_amd import _lib, ops

TH, R, Q, P_INIT, MIN_SIZE = 0.3, 10.0, 1.0, 100.0, 75
MARGIN = 1e-3
TICK = np.dtype([("dt", "<i4"), ("horizon", "<f4"), ("img_w", "<f4"), ("img_h", "<f4"), ("divisor", "<f4"), ("pad", "<i4", (3,))])
QUERY = np.dtype([("slot", "<i4"), ("horizon", "<f4"), ("img_w", "<f4"), ("img_h", "<f4")])
assert TICK.itemsize == 32 and QUERY.itemsize == 16


def f32(v):
    """The float32 value the kernel receives for a Python float, as an exact Python float."""
    return float(np.float32(v))


class NP64:
    arr = staticmethod(lambda v: np.array(v, dtype=np.float64))
    eye = staticmethod(lambda n: np.eye(n, dtype=np.float64))
    inv = staticmethod(np.linalg.inv)
    num = staticmethod(np.float64)


class TH32:
    arr = staticmethod(lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float32))
    eye = staticmethod(lambda n: torch.eye(n, dtype=torch.float32))
    inv = staticmethod(torch.linalg.inv)
    num = staticmethod(lambda v: torch.tensor(float(v), dtype=torch.float32))


def _lo(a, b):
    return a if a < b else b


def _hi(a, b):
    return a if a > b else b


class Restatement:
    """The tracker in plain Python over the adapter A (NP64 or TH32).  All inputs are float32-exact numbers."""

    def __init__(self, A, T):
        self.A, self.T = A, T
        self.slots = {}
        self.iou_margin, self.ties, self.clean_ok = np.inf, 0, True

    def slot(self, s):
        return self.slots.setdefault(s, dict(x=[], P=[], label=[], score=[], id=[], n_matched=0, next_id=0))

    def _iou(self, a, b):
        iw = _hi(_lo(a[0] + a[2], b[0] + b[2]) - _hi(a[0], b[0]), self.A.num(0.0))
        ih = _hi(_lo(a[1] + a[3], b[1] + b[3]) - _hi(a[1], b[1]), self.A.num(0.0))
        inter = iw * ih
        return inter / (a[2] * a[3] + b[2] * b[3] - inter)

    def update(self, s, first, det, dt, horizon, img_w, img_h, divisor):
        A, st = self.A, self.slot(s)
        if first:
            st.update(x=[], P=[], label=[], score=[], id=[], n_matched=0, next_id=0)
        n = len(st["x"])
        if n:                                                    # predict
            F, Qm = A.eye(8), A.eye(8) * A.num(dt) * A.num(dt) * A.num(Q)
            for k in range(4):
                F[k, k + 4] = dt
            st["x"] = [F @ x for x in st["x"]]
            st["P"] = [F @ P @ F.T + Qm for P in st["P"]]
        det = np.asarray(det, dtype=np.float32).reshape(-1, 7)[:self.T]      # truncate: detections beyond T are dropped
        m = len(det)
        if m:
            d = A.arr(det[:, :4].astype(np.float64)) / A.num(divisor)
            z = [A.arr([0.0] * 4) for _ in range(m)]
            for j in range(m):
                z[j][0], z[j][1], z[j][2], z[j][3] = d[j, 0], d[j, 1], d[j, 2] - d[j, 0], d[j, 3] - d[j, 1]
            score = [np.float32(det[j, 4]) * np.float32(det[j, 5]) for j in range(m)]
            label = [int(det[j, 6]) for j in range(m)]
            taken, match = set(), [None] * m
            th = A.num(f32(TH))
            for j in range(m):                                   # associate: greedy in detection order
                best, best_iou, seen = None, None, []
                for i in range(n):
                    if i in taken or st["label"][i] != label[j]:
                        continue
                    iou = self._iou(st["x"][i], z[j])
                    seen.append(float(iou))
                    if iou >= th and (best is None or iou >= best_iou):      # replaced on >=: the highest index wins a tie
                        best, best_iou = i, iou
                for v in seen:
                    self.iou_margin = min(self.iou_margin, abs(v - f32(TH)))
                if best is not None:
                    rest = sorted(seen, reverse=True)
                    if len(rest) > 1:
                        if rest[0] == rest[1]:
                            self.ties += 1
                        else:
                            self.iou_margin = min(self.iou_margin, rest[0] - rest[1])
                    taken.add(best)
                    match[j] = best
            matched = [j for j in range(m) if match[j] is not None]
            fresh = [j for j in range(m) if match[j] is None]
            xs, Ps, ids = [], [], []
            for j in matched:                                    # matched pairs first, each updated with its detection
                x, P = st["x"][match[j]], st["P"][match[j]]
                y = z[j] - x[:4]
                S = P[:4, :4] + A.eye(4) * A.num(R)
                K = P[:, :4] @ A.inv(S)
                xs.append(x + K @ y)
                Ps.append(P - K @ P[:4, :])
                ids.append(st["id"][match[j]])
            for j in fresh:                                      # then the unmatched detections as fresh tracks
                x = A.arr([0.0] * 8)
                x[0], x[1], x[2], x[3] = z[j][0], z[j][1], z[j][2], z[j][3]
                xs.append(x)
                Ps.append(A.eye(8) * A.num(P_INIT))
                ids.append(st["next_id"])
                st["next_id"] += 1
            order = matched + fresh
            st.update(x=xs, P=Ps, id=ids, label=[label[j] for j in order], score=[score[j] for j in order],
                      n_matched=len(matched))
        return self.forecast(s, horizon, img_w, img_h)

    def forecast(self, s, horizon, img_w, img_h):
        A, st = self.A, self.slot(s)
        boxes, keep = [], []
        for k, x in enumerate(st["x"]):
            b = [x[0], x[1], x[2], x[3]]
            if k < st["n_matched"]:
                b = [x[i] + A.num(horizon) * x[i + 4] for i in range(4)]
            w, h = b[2], b[3]
            ok = bool(w > 0) and bool(h > 0)
            ltrb = [_lo(_hi(b[0], A.num(0.0)), A.num(img_w)), _lo(_hi(b[1], A.num(0.0)), A.num(img_h)),
                    _lo(_hi(b[0] + b[2], A.num(0.0)), A.num(img_w)), _lo(_hi(b[1] + b[3], A.num(0.0)), A.num(img_h))]
            cw, ch = ltrb[2] - ltrb[0], ltrb[3] - ltrb[1]
            if A is NP64:                                        # the condition on the inputs (see the module docstring)
                vals = [float(v) for v in (w, h, cw, ch) + tuple(ltrb)]
                exact = all(f32(v) == v for v in vals)
                lo = int(max(float(cw) - MARGIN, 0.0)) * int(max(float(ch) - MARGIN, 0.0))
                up = int(float(cw) + MARGIN) * int(float(ch) + MARGIN)
                away = abs(float(w)) > MARGIN and abs(float(h)) > MARGIN and (not ok or (lo >= MIN_SIZE) == (up >= MIN_SIZE))
                self.clean_ok = self.clean_ok and (exact or away)
            ok = ok and int(float(cw)) * int(float(ch)) >= MIN_SIZE
            if ok:
                boxes.append([float(v) for v in ltrb])
                keep.append(k)
        return dict(box=np.array(boxes, dtype=np.float64).reshape(-1, 4), id=[st["id"][k] for k in keep],
                    label=[st["label"][k] for k in keep], score=[st["score"][k] for k in keep])


def dets(boxes, scores=None, labels=None):
    """[k, 7] float32 rows as sy_postprocess writes them (x1, y1, x2, y2, obj, class_conf, class), descending score."""
    k = len(boxes)
    scores = list(np.linspace(0.9, 0.5, k)) if scores is None else scores
    labels = [0] * k if labels is None else labels
    assert all(scores[i] >= scores[i + 1] for i in range(k - 1))
    d = np.zeros((k, 7), dtype=np.float32)
    d[:, :4] = np.asarray(boxes, dtype=np.float32).reshape(k, 4)
    d[:, 4], d[:, 5], d[:, 6] = scores, 0.75, labels
    return d


def row(slot, det, first=False, dt=1, horizon=0.0, img=(192.0, 128.0), divisor=1.0):
    return dict(slot=slot, det=det, first=first, dt=dt, horizon=horizon, img_w=img[0], img_h=img[1], divisor=divisor)


class Harness:
    """The kernel and both restatements side by side; tick() asserts everything the module docstring promises."""

    def __init__(self, backend, B, S, T, max_det=None):
        self.dev, self.B, self.S, self.T = backend, B, S, T
        self.max_det = max_det or T + 5
        self.state = ops.TrackState(S, T, backend)
        self.prm = ops.track_params(TH, R, Q, P_INIT, MIN_SIZE)
        self.out = torch.zeros((B, T, 6), dtype=torch.float32, device=backend)
        self.out_id = torch.zeros((B, T), dtype=torch.int32, device=backend)
        self.out_cnt = torch.zeros(B, dtype=torch.int32, device=backend)
        self.ref, self.r32 = Restatement(NP64, T), Restatement(TH32, T)
        self.err_k = self.err_32 = 0.0
        self.last = None

    def launch(self, rows):
        B = self.B
        det = np.zeros((B, self.max_det, 7), dtype=np.float32)
        cnt, slot, first, tick = np.zeros(B, np.int32), np.full(B, -1, np.int32), np.zeros(B, np.uint8), np.zeros(B, TICK)
        for b, r in enumerate(rows):
            if r is None:
                continue
            k = len(r["det"])
            det[b, :k] = r["det"]
            cnt[b], slot[b], first[b] = k, r["slot"], 1 if r["first"] else 0
            tick[b] = (r["dt"], r["horizon"], r["img_w"], r["img_h"], r["divisor"], (0, 0, 0))
        to = lambda a: torch.from_numpy(a).to(self.dev)
        self.out.fill_(-7.0); self.out_id.fill_(-7); self.out_cnt.fill_(-7)
        ops.track_update(to(det), to(cnt), to(slot), to(first), to(tick.view(np.uint8)), self.state, self.prm, self.out,
                         self.out_id, self.out_cnt)
        return self.out.cpu().numpy(), self.out_id.cpu().numpy(), self.out_cnt.cpu().numpy()

    def tick(self, rows, ties=0):
        rows = list(rows) + [None] * (self.B - len(rows))
        before = [t.clone() for t in self.state.tensors()]
        out, out_id, out_cnt = self.launch(rows)
        after = [t.cpu().numpy() for t in self.state.tensors()]
        live = {r["slot"] for r in rows if r is not None and 0 <= r["slot"] < self.S}
        for s in range(self.S):                                  # slots without a row this tick: bit for bit as they were
            if s not in live:
                assert all(np.array_equal(b[s].cpu().numpy(), a[s]) for b, a in zip(before, after)), s
        res = []
        for b, r in enumerate(rows):
            if r is None or not 0 <= r["slot"] < self.S:
                assert out_cnt[b] == 0 and (out[b] == -7.0).all() and (out_id[b] == -7).all()
                res.append(None)
                continue
            args = (r["slot"], r["first"], r["det"], r["dt"], f32(r["horizon"]), f32(r["img_w"]), f32(r["img_h"]), f32(r["divisor"]))
            ties0 = self.ref.ties
            want, w32 = self.ref.update(*args), self.r32.update(*args)
            assert self.ref.iou_margin > MARGIN and self.ref.clean_ok, "the test's inputs are too close to call in fp32"
            assert self.ref.ties - ties0 == ties
            n = len(want["id"])
            assert out_cnt[b] == n and (out[b, n:] == -7.0).all()
            assert out_id[b, :n].tolist() == want["id"] == w32["id"]
            assert out[b, :n, 5].tolist() == want["label"] and out[b, :n, 4].tolist() == [float(v) for v in want["score"]]
            st, s = self.ref.slot(r["slot"]), r["slot"]
            x, P, score, label, tid, hdr = after
            nn = len(st["x"])
            assert hdr[s].tolist() == [nn, st["n_matched"], st["next_id"], 0]
            assert tid[s, :nn].tolist() == st["id"] and label[s, :nn].tolist() == st["label"]
            assert score[s, :nn].tolist() == [float(v) for v in st["score"]]
            xs = np.array([np.asarray(v) for v in st["x"]]).reshape(nn, 8)
            x32 = np.array([v.numpy() for v in self.r32.slot(s)["x"]], dtype=np.float64).reshape(nn, 8)
            ek = max(np.abs(out[b, :n, :4] - want["box"]).max(initial=0.0), np.abs(x[s, :, :nn].T - xs).max(initial=0.0))
            e32 = max(np.abs(w32["box"] - want["box"]).max(initial=0.0), np.abs(x32 - xs).max(initial=0.0))
            print("track tick: kernel err %.3g, float32 restatement err %.3g" % (ek, e32))
            assert ek <= max(4.0 * e32, 1e-3), (ek, e32)
            self.err_k, self.err_32 = max(self.err_k, ek), max(self.err_32, e32)
            res.append(dict(want, n_matched=st["n_matched"], next_id=st["next_id"]))
        self.last = (out, out_id, out_cnt)
        return res

    def record(self, key):
        record_parity("track_kf_" + key, kernel_err_px=self.err_k, float32_restatement_err_px=self.err_32)


def grid_boxes(n, cols=10, size=12, pitch=16, shift=(0, 0)):
    return [[(i % cols) * pitch + shift[0], (i // cols) * pitch + shift[1], (i % cols) * pitch + shift[0] + size,
             (i // cols) * pitch + shift[1] + size] for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------
def test_overflow_detections_are_dropped(backend):
    """T = 8, 11 detections: the first 8 (the highest scores) become tracks, and again on the next tick."""
    h = Harness(backend, 1, 2, 8, max_det=11)
    r = h.tick([row(1, dets(grid_boxes(11)), first=True)])[0]
    assert r["id"] == list(range(8)) and r["next_id"] == 8
    r = h.tick([row(1, dets(grid_boxes(11, shift=(2, 1))))])[0]
    assert r["id"] == list(range(8)) and r["n_matched"] == 8 and r["next_id"] == 8
    h.record("overflow")


@pytest.mark.parametrize("dt", [1, 3])
def test_no_detections_keep_the_predicted_state(backend, dt):
    """cnt = 0 on a slot with moving tracks: x and P are predicted by dt and kept, n_matched / ids / labels stay."""
    h = Harness(backend, 1, 1, 8)
    h.tick([row(0, dets(grid_boxes(3)), first=True)])
    a = h.tick([row(0, dets(grid_boxes(2, shift=(3, 2))), dt=dt)])[0]
    assert a["n_matched"] == 2 and a["id"] == [0, 1]
    P0 = h.state.P.clone()
    b = h.tick([row(0, dets([]), dt=dt, horizon=1.0)])[0]
    assert b["n_matched"] == 2 and b["id"] == [0, 1] and b["next_id"] == 3
    assert not torch.equal(h.state.P, P0)                        # (the covariance grew)
    c = h.tick([row(0, dets(grid_boxes(2, shift=(3 + 3 * dt, 2 + 2 * dt))), dt=dt)])[0]
    assert c["id"] == [0, 1]
    h.record("predict_dt%d" % dt)


def test_row_first_restarts_a_slot(backend):
    h = Harness(backend, 1, 1, 8)
    assert h.tick([row(0, dets(grid_boxes(4)), first=True)])[0]["id"] == [0, 1, 2, 3]
    r = h.tick([row(0, dets(grid_boxes(3, shift=(1, 1))), first=True, dt=0)])[0]
    assert r["id"] == [0, 1, 2] and r["n_matched"] == 0 and r["next_id"] == 3
    r = h.tick([row(0, dets([]), first=True)])[0]                # a first frame without detections: an empty slot
    assert r["id"] == [] and r["next_id"] == 0


def test_rows_without_a_slot_write_nothing(backend):
    """Slot -1 and a slot >= S: count 0, no pool and no output row touched (Harness.tick checks both), beside a live row."""
    h = Harness(backend, 3, 2, 8)
    h.tick([row(0, dets(grid_boxes(2)), first=True), row(1, dets(grid_boxes(3)), first=True)])
    res = h.tick([row(-1, dets(grid_boxes(2))), row(1, dets(grid_boxes(3, shift=(1, 0)))), row(2, dets(grid_boxes(2)), first=True)])
    assert res[0] is None and res[2] is None and res[1]["id"] == [0, 1, 2]
    res = h.tick([row(7, dets(grid_boxes(2))), None, row(-3, dets(grid_boxes(2)))])
    assert res == [None, None, None]


def test_label_mismatch_blocks_a_perfect_overlap(backend):
    h = Harness(backend, 1, 1, 8)
    h.tick([row(0, dets(grid_boxes(2), labels=[1, 2]), first=True)])
    r = h.tick([row(0, dets(grid_boxes(2), labels=[2, 2]))])[0]
    assert r["id"] == [1, 2] and r["n_matched"] == 1             # the box of track 0 came back as class 2: a fresh track


def test_exact_iou_tie_goes_to_the_higher_track(backend):
    """Tracks (0, 0, 10, 10) and (10, 0, 20, 10), a detection (5, 0, 15, 10): IoU 50 / 150 with both, to the last bit."""
    h = Harness(backend, 1, 1, 8)
    h.tick([row(0, dets([[0, 0, 10, 10], [10, 0, 20, 10]]), first=True)])
    r = h.tick([row(0, dets([[5, 0, 15, 10]]))], ties=1)[0]
    assert r["id"] == [1] and r["n_matched"] == 1


def test_best_track_taken_by_an_earlier_detection(backend):
    """Both detections overlap track 0 best; the second one has to settle for track 1."""
    h = Harness(backend, 1, 1, 8)
    h.tick([row(0, dets([[0, 0, 20, 20], [12, 0, 32, 20]]), first=True)])
    r = h.tick([row(0, dets([[1, 0, 21, 20], [4, 0, 24, 20]]))])[0]
    assert r["id"] == [0, 1] and r["n_matched"] == 2


def test_nothing_matches_starts_from_scratch(backend):
    h = Harness(backend, 1, 1, 8)
    h.tick([row(0, dets(grid_boxes(3)), first=True)])
    r = h.tick([row(0, dets(grid_boxes(2, shift=(0, 64))))])[0]
    assert r["id"] == [3, 4] and r["n_matched"] == 0 and r["next_id"] == 5      # ids without gaps


def test_winner_beyond_lane_63(backend):
    """70 live tracks, T = 256: the first detection of the next tick belongs to track 69 (a lane's second track), and the
    detections arrive in the reverse order of the tracks."""
    h = Harness(backend, 1, 1, 256, max_det=80)
    h.tick([row(0, dets(grid_boxes(70), scores=list(np.linspace(0.9, 0.2, 70))), first=True, img=(256.0, 256.0))])
    back = grid_boxes(70, shift=(1, 1))[::-1]
    r = h.tick([row(0, dets(back, scores=list(np.linspace(0.9, 0.2, 70))), img=(256.0, 256.0))])[0]
    assert r["id"] == list(range(69, -1, -1)) and r["n_matched"] == 70
    h.record("wave_boundary")


def test_clean_up(backend):
    """extrap_clean_up: a box that left the image, a width forecast below zero, 15 x 5 kept and 14.9 x 5 dropped, and the
    horizon moving matched tracks only."""
    h = Harness(backend, 1, 1, 8)
    first = [[150, 10, 180, 40], [20, 60, 60, 100], [10, 10, 25, 15], [40, 10, 54.9, 15], [100, 60, 130, 90]]
    r = h.tick([row(0, dets(first), first=True)])[0]
    assert r["id"] == [0, 1, 2, 4]                               # 14.9 x 5 -> int 14 * 5 = 70 < 75
    # track 0 runs right, track 1 shrinks, track 4 stands still; one fresh detection
    second = [[160, 10, 190, 40], [22, 60, 50, 100], [100, 60, 130, 90], [60, 10, 90, 40]]
    r0 = h.tick([row(0, dets(second))])[0]
    assert r0["id"] == [0, 1, 4, 5] and r0["n_matched"] == 3
    r = h.tick([row(0, dets([]), horizon=20.0)])[0]              # far ahead: 0 is out of the image, 1 has no width left
    assert r["id"] == [4, 5]
    assert np.array_equal(r["box"][1], [60, 10, 90, 40])         # the unmatched track does not move
    h.record("clean_up")


def test_two_streams_swap_rows_and_sit_out(backend):
    """Which row belongs to which slot is data: two streams over 6 ticks in changing rows, each sitting out ticks."""
    h = Harness(backend, 2, 3, 8)
    a = lambda t: dets(grid_boxes(3, shift=(2 * t, t)), labels=[0, 1, 0])
    c = lambda t: dets(grid_boxes(4, shift=(t, 3 * t + 40)), labels=[1, 1, 2, 2])
    h.tick([row(2, a(0), first=True), row(0, c(0), first=True)])
    h.tick([row(0, c(1), horizon=1.0), row(2, a(1))])
    h.tick([None, row(2, a(2), horizon=0.5)])                    # stream c sits out
    res = h.tick([row(0, c(3), dt=2), None])                     # stream a sits out
    assert res[0]["id"] == [0, 1, 2, 3]
    res = h.tick([row(2, a(4), dt=2, horizon=2.0), row(0, c(4))])
    assert res[0]["id"] == [0, 1, 2] and res[1]["id"] == [0, 1, 2, 3]
    h.tick([row(0, c(5), divisor=0.5), row(1, a(0), first=True)])     # (c's boxes double: nothing matches, fresh ids)
    h.record("two_streams")


def test_smooth_motion_over_20_ticks(backend):
    """One stream, 20 ticks, boxes in smooth motion (non-integer, another divisor): the error against float64 stays bounded."""
    h = Harness(backend, 1, 1, 16)
    for t in range(20):
        boxes = [[20.3 + 3.1 * t, 15.2 + 1.3 * t + 0.05 * t * t, 60.9 + 3.4 * t, 70.1 + 1.2 * t + 0.05 * t * t],
                 [300.7 - 4.2 * t, 40.4 + 0.5 * t, 360.2 - 4.0 * t, 95.8 + 0.9 * t],
                 [150.1 + 0.7 * t, 180.6 - 2.2 * t, 210.5 + 0.9 * t, 230.3 - 2.0 * t]]
        r = h.tick([row(0, dets(np.float32(boxes) * np.float32(0.4), labels=[0, 0, 3]), first=t == 0, horizon=1.5,
                        img=(480.0, 300.0), divisor=0.4)])[0]
        assert sorted(r["id"]) == [0, 1, 2]
    h.record("smooth_20_ticks")


def test_forecast_reads_the_state_only(backend):
    """sy_track_forecast at the horizon of the last update == what the update wrote; other horizons == the restatement; the
    pools stay bit-equal; an entry without a slot reports 0."""
    h = Harness(backend, 2, 3, 8)
    h.tick([row(1, dets(grid_boxes(4)), first=True), row(2, dets(grid_boxes(2, shift=(0, 50))), first=True)])
    h.tick([row(2, dets(grid_boxes(2, shift=(4, 53))), horizon=2.0), row(1, dets(grid_boxes(3, shift=(3, 1))), horizon=2.0)])
    out, out_id, out_cnt = h.last
    q = np.zeros(4, QUERY)
    q[0], q[1], q[2], q[3] = (1, 2.0, 192.0, 128.0), (-1, 2.0, 192.0, 128.0), (2, 2.0, 192.0, 128.0), (1, 30.0, 100.0, 128.0)
    before = [t.clone() for t in h.state.tensors()]
    fo = torch.full((4, 8, 6), -7.0, dtype=torch.float32, device=backend)
    fi = torch.full((4, 8), -7, dtype=torch.int32, device=backend)
    fc = torch.full((4,), -7, dtype=torch.int32, device=backend)
    ops.track_forecast(torch.from_numpy(q.view(np.uint8)).to(backend), 4, h.state, h.prm, fo, fi, fc)
    assert all(torch.equal(a, b) for a, b in zip(before, h.state.tensors()))
    fo, fi, fc = fo.cpu().numpy(), fi.cpu().numpy(), fc.cpu().numpy()
    assert fc[0] == out_cnt[1] and np.array_equal(fo[0], out[1]) and np.array_equal(fi[0], out_id[1])
    assert fc[2] == out_cnt[0] and np.array_equal(fo[2], out[0]) and np.array_equal(fi[2], out_id[0])
    assert fc[1] == 0 and (fo[1] == -7.0).all()
    want, w32 = h.ref.forecast(1, 30.0, 100.0, 128.0), h.r32.forecast(1, 30.0, 100.0, 128.0)
    assert h.ref.clean_ok
    n = len(want["id"])
    assert fc[3] == n and fi[3, :n].tolist() == want["id"]
    ek, e32 = np.abs(fo[3, :n, :4] - want["box"]).max(initial=0.0), np.abs(w32["box"] - want["box"]).max(initial=0.0)
    assert ek <= max(4.0 * e32, 1e-3)


def test_bad_arguments(backend):
    h = Harness(backend, 1, 1, 8)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=backend)
    det, cnt, slot, first, ticks = z(1, 4, 7), z(1, dt=torch.int32), z(1, dt=torch.int32), z(1, dt=torch.uint8), z(32, dt=torch.uint8)
    lib, st, sm = _lib.lib(), h.state.c_struct(), ops.stream_of(det)
    import ctypes as C

    def update(det_p=det.data_ptr(), B=1, max_det=4, state=st, prm=h.prm, out_p=h.out.data_ptr()):
        return lib.sy_track_update(det_p, cnt.data_ptr(), B, max_det, slot.data_ptr(), first.data_ptr(), ticks.data_ptr(),
                                   C.byref(state) if state is not None else None, C.byref(prm) if prm is not None else None, out_p,
                                   h.out_id.data_ptr(), h.out_cnt.data_ptr(), sm)
    assert update() == 0
    assert update(det_p=None) == 1 and update(out_p=None) == 1 and update(state=None) == 1 and update(prm=None) == 1
    assert update(B=0) == 1 and update(max_det=0) == 1
    for field, bad in (("max_tracks", 0), ("max_tracks", _lib.TRACK_MAX_TRACKS + 1), ("n_slots", 0), ("P", None)):
        s2 = h.state.c_struct()
        setattr(s2, field, bad)
        assert update(state=s2) == 1, field
        assert lib.sy_track_forecast(ticks.data_ptr(), 1, C.byref(s2), C.byref(h.prm), h.out.data_ptr(), h.out_id.data_ptr(),
                                     h.out_cnt.data_ptr(), sm) == 1, field
    assert update(prm=ops.track_params(match_iou_th=0.0)) == 1
    assert lib.sy_track_forecast(None, 1, C.byref(st), C.byref(h.prm), h.out.data_ptr(), h.out_id.data_ptr(), h.out_cnt.data_ptr(), sm) == 1
    assert lib.sy_track_forecast(ticks.data_ptr(), 0, C.byref(st), C.byref(h.prm), h.out.data_ptr(), h.out_id.data_ptr(),
                                 h.out_cnt.data_ptr(), sm) == 1
    with pytest.raises(_lib.HipLibraryError, match="bad argument"):
        ops.track_update(det, cnt, slot, first, ticks, h.state, ops.track_params(match_iou_th=-1.0), h.out, h.out_id, h.out_cnt)
    with pytest.raises(AssertionError):                          # an output of the wrong shape never reaches the library
        ops.track_update(det, cnt, slot, first, ticks, h.state, h.prm, h.out[:, :4].contiguous(), h.out_id, h.out_cnt)

"""streamyolo_amd.scoring: score_coco on the rows the streaming glue produces, and DetectionScorer fed with a detector's device
tensors tick by tick.  The yardstick is the float64 restatement of COCOeval in tests/test_score_kernel.py, run on what the host
sees of the same data; the demand is equality to the last bit."""
import numpy as np
import pytest
import torch

from conftest import record_parity
from streamyolo_amd import _lib
from streamyolo_amd import streaming as S
from streamyolo_amd.scoring import DetectionScorer, score_coco
from test_score_kernel import assert_same, restate_rows

K = 8


def _restate_dicts(results, annotations, class_ids, image_ids):
    """The restatement on COCO-format dicts: images in ascending id, rows in the order given."""
    cls = {c: n for n, c in enumerate(class_ids)}
    per_image = []
    for i in sorted(set(image_ids)):
        dets = [{"bbox": [float(np.float32(v)) for v in r["bbox"]], "score": np.float32(r["score"]), "label": cls[int(r["category_id"])]}
                for r in results if r["image_id"] == i and int(r["category_id"]) in cls]
        gts = [{"bbox": [float(v) for v in a["bbox"]], "label": cls[a["category_id"]], "iscrowd": int(a.get("iscrowd", 0)),
                "area": float(a["area"]) if "area" in a else float(a["bbox"][2]) * float(a["bbox"][3])}
               for a in annotations if a["image_id"] == i and a["category_id"] in cls]
        per_image.append((dets, gts))
    return restate_rows(per_image, len(class_ids))


class SimClock:
    def __init__(self):
        self.t, self.tick = 100.0, 1e-4

    def __call__(self):
        self.t += self.tick
        return self.t


def _synthetic_sequence(n_frames=20, seed=5):
    """A run_sequence result over fake frames (the detector answers after 20-50 ms with boxes around the frame's objects) and
    the sequence's COCO annotations: objects drifting 3 px per frame."""
    rs = np.random.RandomState(seed)
    objects = [(rs.randint(0, 300), rs.randint(0, 200), rs.randint(12, 120), rs.randint(12, 120), rs.randint(K)) for _ in range(7)]
    image_ids = [1000 + 2 * n for n in range(n_frames)]
    annotations = []
    for n, image_id in enumerate(image_ids):
        for j, (x, y, w, h, c) in enumerate(objects):
            a = {"image_id": image_id, "bbox": [x + 3.0 * n, y + 1.0 * n, float(w), float(h)], "category_id": c}
            if j == 2:
                a["iscrowd"] = 1
            if j != 4:
                a["area"] = float(w * h)
            annotations.append(a)
    clock = SimClock()

    def detect(frame):
        clock.t += 0.02 + 0.03 * rs.rand()
        boxes, scores, labels = [], [], []
        for (x, y, w, h, c) in objects:
            for _ in range(rs.randint(0, 3)):
                dx, dy = rs.randint(-6, 7, 2) * 0.5
                boxes.append([x + 3.0 * frame + dx, y + 1.0 * frame + dy, x + 3.0 * frame + dx + w, y + 1.0 * frame + dy + h])
                scores.append(rs.randint(1, 9) / 8.0)
                labels.append(c if rs.rand() < 0.9 else rs.randint(K))
        order = np.argsort(-np.asarray(scores), kind="mergesort") if scores else []
        return (np.asarray(boxes, dtype=np.float32).reshape(-1, 4)[order], np.asarray(scores, dtype=np.float32)[order],
                np.asarray(labels, dtype=np.int32)[order], None)
    results = S.run_sequence(list(range(n_frames)), detect, fps=30.0, clock=clock)
    return results, image_ids, annotations


def test_score_coco_on_paired_streaming_rows(backend):
    results, image_ids, annotations = _synthetic_sequence()
    rows, stats = S.pair_with_ground_truth(results, image_ids, fps=30.0)
    assert len(rows) > 50 and stats["mismatch"] > 0                  # late results: the boxes lag their ground truth
    class_ids = list(range(K))
    got = score_coco(rows, annotations, class_ids, device=backend, batch=6)
    want = _restate_dicts(rows, annotations, class_ids, image_ids)
    assert_same(got, want)
    assert 0.0 < want["AP"] < 1.0 and 0.0 < want["AR100"] < 1.0
    again = score_coco(rows, annotations, class_ids, image_ids=image_ids, device=backend, batch=64)    # another batching: same bits
    assert_same(again, want)
    # category ids need not be positions: the evaluator's own ids, and a category the dataset does not know is left out
    ids = [3, 1, 4, 15, 9, 2, 6, 5]
    mapped_rows = [dict(r, category_id=ids[int(r["category_id"])]) for r in rows] + [dict(rows[0], category_id=77)]
    mapped_ann = [dict(a, category_id=ids[a["category_id"]]) for a in annotations]
    assert_same(score_coco(mapped_rows, mapped_ann, ids, device=backend), want)
    record_parity("score_coco_paired_%s" % backend.type, max_abs_diff=0.0, AP=got["AP"], rows=len(rows))


def test_score_coco_refuses_a_result_on_an_unknown_image(backend):
    results, image_ids, annotations = _synthetic_sequence(6)
    rows, _ = S.pair_with_ground_truth(results, image_ids, fps=30.0)
    with pytest.raises(ValueError, match="unknown image"):
        score_coco(rows + [dict(rows[0], image_id=999)], annotations, list(range(K)), device=backend)
    with pytest.raises(ValueError, match="unknown image"):
        score_coco(rows, annotations, list(range(K)), image_ids=image_ids[:1], device=backend)
    for bad in (-0.25, float("nan")):                                # the device orders scores by their bits: >= 0 only
        with pytest.raises(ValueError, match="scores must be"):
            score_coco(rows + [dict(rows[0], score=bad)], annotations, list(range(K)), device=backend)


# ---- the detector's own device tensors ------------------------------------------------------------------------------------------
HW, BATCH, T = (128, 192), 2, 32


def _model():
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    sd = synth_state_dict(O.param_shapes(O.OracleConfig.named("nano")), seed=0, bn_stats=load_bn_stats("nano"))
    model = sy.build_model("nano")
    model.load_state_dict(sd, strict=True)
    return model


def _clip(hw, seed, n, step=(1, 2)):
    base = np.random.RandomState(seed).randint(0, 256, tuple(hw) + (3,)).astype(np.uint8)
    return [np.roll(base, (step[0] * t, step[1] * t), axis=(0, 1)) for t in range(n)]


def _parse_nms(det, cnt, n, div):
    """What MultiStreamDetector.__call__ returns for a tick, from copies of the device tensors."""
    det, cnt = det.cpu().numpy(), cnt.cpu().numpy()
    return [(det[b, :cnt[b], :4] / div, det[b, :cnt[b], 4] * det[b, :cnt[b], 5], det[b, :cnt[b], 6].astype(np.int32)) for b in range(n)]


def _parse_track(out, out_cnt, n):
    out, cnt = out.cpu().numpy(), out_cnt.cpu().numpy()
    return [(out[b, :cnt[b], :4], out[b, :cnt[b], 4], out[b, :cnt[b], 5].astype(np.int32)) for b in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("track", [False, True])
def test_detector_ticks_scored_on_the_device_equal_host_scoring(track):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda:0")
    det = S.MultiStreamDetector(_model(), HW, max_streams=2, batch=BATCH, device=dev, track=S.TrackConfig(max_tracks=T) if track else None)
    det.warm_up(2)
    sids = [det.open(), det.open()]
    clips = [_clip(HW, 60 + k, 6, step=(1 + k, 2)) for k in range(2)]
    div = det._geom[sids[0]][2]
    divisor = None if track else torch.full((BATCH,), div, dtype=torch.float32, device=dev)
    max_gt = 128
    scorer = DetectionScorer(K, capacity=4096, max_gt=max_gt, device=dev)
    prev = [None, None]                                              # per stream: the previous frame's host-parsed detections
    per_image = []
    for t in range(6):
        res = det.detect_device([clips[k][t] for k in range(2)], sids, **({"horizon": 1.0} if track else {}))
        parsed = _parse_track(res[-3], res[-1], 2) if track else _parse_nms(res[0], res[1], 2, div)
        gt = np.zeros((BATCH, max_gt, 7), dtype=np.float64)
        gcnt = np.zeros(BATCH, dtype=np.int32)
        for b in range(2):
            gts = []
            if prev[b] is not None:                                  # ground truth of frame n: frame n - 1's detections above 0.3
                boxes, scores, labels = prev[b]
                ltwh = S.ltrb2ltwh(boxes).astype(np.float64)
                gts = [[ltwh[j, 0], ltwh[j, 1], ltwh[j, 2], ltwh[j, 3], int(labels[j]), 0, ltwh[j, 2] * ltwh[j, 3]]
                       for j in range(len(boxes)) if scores[j] > 0.3][:max_gt]
            gcnt[b] = len(gts)
            if gts:
                gt[b, :len(gts)] = gts
            boxes, scores, labels = parsed[b]
            ltwh = S.ltrb2ltwh(boxes)                                # float32, as pair_with_ground_truth forms the rows
            dets = [{"bbox": [float(v) for v in ltwh[j]], "score": np.float32(scores[j]), "label": int(labels[j])} for j in range(len(boxes))]
            per_image.append((dets, [{"bbox": g[:4], "label": g[4], "iscrowd": 0, "area": g[6]} for g in gts]))
        if track:
            scorer.add(res[-3], res[-1], torch.from_numpy(gt).to(dev), torch.from_numpy(gcnt).to(dev), rows=2, layout="track")
        else:
            scorer.add(res[0], res[1], torch.from_numpy(gt).to(dev), torch.from_numpy(gcnt).to(dev), divisor=divisor, rows=2)
        prev = parsed
    want = restate_rows(per_image, K)
    assert 0.0 < want["AP"] < 1.0                                    # the case is not vacuous
    assert sum(len(d) for d, _ in per_image) > 20 and sum(len(g) for _, g in per_image) > 5
    got = scorer.summarize()
    assert_same(got, want)
    record_parity("score_detector_%s" % ("track" if track else "nms"), max_abs_diff=0.0, AP=got["AP"], AR100=got["AR100"],
                  detections=sum(len(d) for d, _ in per_image))
    for s in sids:
        det.close(s)

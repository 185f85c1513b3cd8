"""sy_score_match / sy_score_accumulate (csrc/score.hip) on hand-made images, on the SIMT emulator and on the MI355X.

pycocotools is not a dependency, so the yardstick is `restate` below: COCOeval's computeIoU, evaluateImg, accumulate and summarize
for boxes, in COCOeval's own loop form, in float64 numpy.  Every operation of it is one IEEE double operation in a fixed order on
float32-exact inputs, and the kernels do the same operations in the same order on thresholds the host computed: the demand is
EQUALITY TO THE LAST BIT of `precision`, `recall` and the twelve statistics — no tolerance anywhere in this file.

An image is a dict: "det" = float32 rows as the kernel receives them (layout "nms": x1, y1, x2, y2, obj, class_conf, class;
"track": x1, y1, x2, y2, score, label), "gt" = float64 rows x, y, w, h, class, iscrowd, area, "div" = the row's divisor or None."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import record_parity
from streamyolo_amd import _lib, ops
from streamyolo_amd.scoring import DetectionScorer

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]
RECORD = np.dtype(_lib.SCORE_RECORD)
assert RECORD.itemsize == 32


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def host_dets(det, layout, div):
    """What the kernel makes of an image's rows before it turns to double: divide in float32, w = x2 - x1, h = y2 - y1 in float32.
    -> list of dicts (bbox = float64 x, y, w, h; score float32; label) in input order."""
    det = np.asarray(det, dtype=np.float32).reshape(-1, 7 if layout == "nms" else 6)
    out = []
    for r in det:
        xyxy = r[:4] / np.float32(div) if div is not None else r[:4]
        if layout == "xywh":
            w, h = xyxy[2], xyxy[3]
        else:
            w, h = np.float32(xyxy[2] - xyxy[0]), np.float32(xyxy[3] - xyxy[1])
        score = np.float32(r[4] * r[5]) if layout == "nms" else np.float32(r[4])
        out.append({"bbox": [float(xyxy[0]), float(xyxy[1]), float(w), float(h)], "score": score, "label": int(r[-1])})
    return out


def bb_iou(d, g, crowd):
    """maskApi.c::bbIou for one pair."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        w = 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        h = 0.0
    i = w * h
    da, ga = d[2] * d[3], g[2] * g[3]
    u = da if crowd else da + ga - i
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(i) / np.float64(u)


def evaluate_img(dt, gt, a_rng, max_det):
    """COCOeval.evaluateImg for one image, class and area range: dt / gt are that class's rows in input order."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    gt_ignore = [1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(gt_ignore, kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(g["iscrowd"]) for g in gt]
    ious = np.zeros((len(dt), len(gt)))
    for di, d in enumerate(dt):
        for gi, g in enumerate(gt):
            ious[di, gi] = bb_iou(d["bbox"], g["bbox"], iscrowd[gi])
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
    gt_ig = np.array([gt_ignore[i] for i in gtind])
    dt_ig = np.zeros((T, D))
    for tind, t in enumerate(IOU_THRS):
        for dind, d in enumerate(dt):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind, g in enumerate(gt):
                if gtm[tind, gind] > 0 and not iscrowd[gind]:
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break
                if ious[dind, gind] < iou:
                    continue
                iou = ious[dind, gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = gt_ig[m]
            dtm[tind, dind] = 1 + m
            gtm[tind, m] = 1 + dind
    a = np.array([d["bbox"][2] * d["bbox"][3] < a_rng[0] or d["bbox"][2] * d["bbox"][3] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}


def accumulate(eval_imgs, K):
    """COCOeval.accumulate: eval_imgs[k][a] = the per-image results (None left out) in image order."""
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                E = [e for e in eval_imgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E]).astype(np.float32)
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def summarize(precision, recall):
    """COCOeval.summarize's twelve numbers."""
    def stat(ap, iou_thr=None, area=0, m=2):
        s = precision[:, :, :, area, m] if ap else recall[:, :, area, m]
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return {"AP": stat(1), "AP50": stat(1, .5), "AP75": stat(1, .75), "APs": stat(1, area=1), "APm": stat(1, area=2),
            "APl": stat(1, area=3), "AR1": stat(0, m=0), "AR10": stat(0, m=1), "AR100": stat(0, m=2), "ARs": stat(0, area=1),
            "ARm": stat(0, area=2), "ARl": stat(0, area=3)}


def restate_rows(per_image, K):
    """per_image: [(dets, gts)] with dets = [{bbox, score, label}], gts = [{bbox, label, iscrowd, area}] -> summarize()'s dict."""
    eval_imgs = [[[] for _ in AREA_RNG] for _ in range(K)]
    for dets, gts in per_image:
        for k in range(K):
            dt, gt = [d for d in dets if d["label"] == k], [g for g in gts if g["label"] == k]
            for a, rng in enumerate(AREA_RNG):
                eval_imgs[k][a].append(evaluate_img(dt, gt, rng, MAX_DETS[-1]))
    precision, recall = accumulate(eval_imgs, K)
    out = summarize(precision, recall)
    out["precision"], out["recall"] = precision, recall
    return out


def restate(images, K, layout="nms"):
    per_image = []
    for im in images:
        gts = [{"bbox": [float(v) for v in g[:4]], "label": int(g[4]), "iscrowd": int(g[5]), "area": float(g[6])}
               for g in np.asarray(im["gt"], dtype=np.float64).reshape(-1, 7)]
        per_image.append((host_dets(im["det"], layout, im.get("div")), gts))
    return restate_rows(per_image, K)


# ---- the kernel side ------------------------------------------------------------------------------------------------------------
def pack(images, layout, device, D=None, G=None):
    cols = 7 if layout == "nms" else 6
    dets = [np.asarray(im["det"], dtype=np.float32).reshape(-1, cols) for im in images]
    gts = [np.asarray(im["gt"], dtype=np.float64).reshape(-1, 7) for im in images]
    D, G = D or max([len(d) for d in dets] + [1]), G or max([len(g) for g in gts] + [1])
    det, gt = np.zeros((len(images), D, cols), dtype=np.float32), np.zeros((len(images), G, 7), dtype=np.float64)
    det[:] = 7.0                                                 # rows beyond cnt hold plausible junk of class 7 % K: never read
    for b in range(len(images)):
        det[b, :len(dets[b])], gt[b, :len(gts[b])] = dets[b], gts[b]
    cnt = np.array([len(d) for d in dets], dtype=np.int32)
    gcnt = np.array([len(g) for g in gts], dtype=np.int32)
    use_div = any(im.get("div") is not None for im in images)
    div = torch.tensor([im.get("div") or 1.0 for im in images], dtype=torch.float32, device=device) if use_div else None
    t = lambda a: torch.from_numpy(a).to(device)
    return t(det), t(cnt), t(gt), t(gcnt), div


def run_kernel(device, images, K, layout="nms", batches=None, capacity=512, max_gt=64):
    scorer = DetectionScorer(K, capacity=capacity, max_gt=max_gt, device=device)
    n0 = 0
    for n in batches or [len(images)]:
        det, cnt, gt, gcnt, div = pack(images[n0:n0 + n], layout, device)
        scorer.add(det, cnt, gt, gcnt, divisor=div, layout=layout)
        n0 += n
    assert n0 == len(images) == scorer.images
    return scorer, scorer.summarize()


def records(scorer, k):
    used, _, _ = scorer.counters()
    K, cap = scorer.num_classes, scorer.capacity
    head = ((5 * K + 1) * 4 + 31) // 32 * 32
    raw = scorer.state[head + k * cap * 32:head + (k * cap + int(used[k])) * 32].cpu().numpy().view(RECORD)
    return raw[np.argsort(raw["seq"])]


def bits(word, a):
    """The ten threshold bits of area range a as a list of 0 / 1."""
    return [(int(word) >> (a * len(IOU_THRS) + t)) & 1 for t in range(len(IOU_THRS))]


def assert_same(got, want):
    assert got["precision"].shape == want["precision"].shape and got["recall"].shape == want["recall"].shape
    assert np.array_equal(got["precision"], want["precision"])
    assert np.array_equal(got["recall"], want["recall"])
    for name in ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"):
        assert got[name] == want[name], (name, got[name], want[name])


def det_row(x1, y1, x2, y2, score, label=0):
    return [x1, y1, x2, y2, score, 1.0, label]


def gt_row(x, y, w, h, label=0, crowd=0, area=None):
    return [x, y, w, h, label, crowd, w * h if area is None else area]


def check(device, images, K=1, **kw):
    scorer, got = run_kernel(device, images, K, **kw)
    want = restate(images, K, kw.get("layout", "nms"))
    assert_same(got, want)
    return scorer, got


# ---- 1-4: the rules, one at a time ----------------------------------------------------------------------------------------------
def test_iou_exactly_on_a_threshold_matches(backend):
    assert IOU_THRS[0] == 0.5 and IOU_THRS[5] == 0.75
    half = [{"det": [det_row(0, 0, 10, 10, 0.9)], "gt": [gt_row(0, 0, 10, 20)]}]                 # 100 / 200
    scorer, got = check(backend, half)
    r = records(scorer, 0)
    assert len(r) == 1 and bits(r[0]["matched"], 0) == [1] + [0] * 9 and bits(r[0]["ignored"], 0) == [0] * 10
    assert got["precision"][0, 0, 0, 0, 2] == 1.0 / (1.0 + np.spacing(1)) and got["precision"][1, 0, 0, 0, 2] == 0.0
    three_quarters = [{"det": [det_row(0, 0, 30, 10, 0.9)], "gt": [gt_row(0, 0, 40, 10)]}]       # 300 / 400
    scorer, _ = check(backend, three_quarters)
    assert bits(records(scorer, 0)[0]["matched"], 0) == [1] * 6 + [0] * 4


def test_crowd_matches_many_and_counts_for_nothing(backend):
    images = [{"det": [det_row(10, 10, 20, 20, 0.9), det_row(30, 30, 50, 40, 0.8)], "gt": [gt_row(0, 0, 100, 100, crowd=1)]}]
    scorer, got = check(backend, images)
    r = records(scorer, 0)
    assert len(r) == 2
    for rec in r:                                                # union = the detection's own area: IoU 1 at every threshold
        assert bits(rec["matched"], 0) == [1] * 10 and bits(rec["ignored"], 0) == [1] * 10
    _, npig, overflow = scorer.counters()
    assert npig.tolist() == [[0, 0, 0, 0]] and overflow == 0
    assert (got["precision"] == -1).all() and (got["recall"] == -1).all() and got["AP"] == -1.0


def test_area_ranges_are_inclusive_at_both_ends(backend):
    images = [{"det": [det_row(100, 100, 110, 110, 0.9)], "gt": [gt_row(0, 0, 32, 32)]}]       # area exactly 1024; a stray 10 x 10 box
    scorer, _ = check(backend, images)
    _, npig, _ = scorer.counters()
    assert npig.tolist() == [[1, 1, 1, 0]]
    r = records(scorer, 0)[0]
    assert [bits(r["matched"], a) for a in range(4)] == [[0] * 10] * 4
    assert [bits(r["ignored"], a)[0] for a in range(4)] == [0, 0, 1, 1]    # a false positive in all and small only


def test_walk_prefers_a_counted_ground_truth_and_the_later_of_equals(backend):
    # 0.6 with the counted ground truth, 0.9 with the crowd one: the counted one wins wherever it reaches the threshold
    images = [{"det": [det_row(0, 0, 10, 10, 0.9)], "gt": [gt_row(0, 0, 9, 10, crowd=1), gt_row(0, 0, 10, 6)]}]
    scorer, _ = check(backend, images)
    r = records(scorer, 0)[0]
    assert bits(r["matched"], 0)[:2] == [1, 1] and bits(r["ignored"], 0)[:2] == [0, 0]            # t = 0.5, 0.55
    assert bits(r["matched"], 0)[3:8] == [1] * 5 and bits(r["ignored"], 0)[3:8] == [1] * 5        # 0.65 .. 0.85: the crowd one
    # two counted ground truths at IoU 0.8 each: the LATER one is taken, so the second detection still finds the first one free
    images = [{"det": [det_row(0, 0, 10, 10, 0.9), det_row(0, 0, 10, 8, 0.8)], "gt": [gt_row(0, 0, 10, 8), gt_row(0, 2, 10, 8)]}]
    scorer, _ = check(backend, images)
    r = records(scorer, 0)
    assert bits(r[0]["matched"], 0)[:6] == [1] * 6 and bits(r[0]["matched"], 0)[7:] == [0] * 3
    assert bits(r[1]["matched"], 0) == [1] * 10
    # a ground truth taken by the higher score is gone for the next detection
    images = [{"det": [det_row(0, 0, 10, 10, 0.5), det_row(0, 0, 10, 10, 0.9)], "gt": [gt_row(0, 0, 10, 10)]}]
    scorer, got = check(backend, images)
    r = records(scorer, 0)
    assert r[0]["score_bits"] == np.float32(0.9).view(np.uint32) and r[0]["rank"] == 0 and r[1]["rank"] == 1
    assert bits(r[0]["matched"], 0) == [1] * 10 and bits(r[1]["matched"], 0) == [0] * 10 and bits(r[1]["ignored"], 0) == [0] * 10


# ---- 5-7: order, truncation, emptiness --------------------------------------------------------------------------------------------
def _tie_images():
    s = 0.5
    return [
        {"det": [det_row(0, 0, 10, 10, s), det_row(50, 50, 60, 60, s), det_row(0, 0, 10, 9, s)], "gt": [gt_row(0, 0, 10, 10)]},
        {"det": [det_row(50, 50, 60, 60, s), det_row(0, 0, 20, 20, s)], "gt": [gt_row(0, 0, 20, 20), gt_row(100, 100, 5, 5)]},
        {"det": [det_row(0, 0, 10, 10, 0.75)], "gt": []},
        {"det": [det_row(5, 5, 45, 45, s), det_row(5, 5, 45, 45, 0.75)], "gt": [gt_row(5, 5, 40, 40)]},
        {"det": [det_row(0, 0, 10, 10, s)], "gt": [gt_row(0, 0, 10, 10)]},
    ]


def test_score_ties_are_image_major_then_input_order(backend):
    images = _tie_images()
    _, one = check(backend, images, batches=[3, 2])
    _, other = check(backend, images, batches=[1, 4])
    assert np.array_equal(one["precision"], other["precision"]) and np.array_equal(one["recall"], other["recall"])
    assert 0.0 < one["AP"] < 1.0


def test_only_the_best_hundred_detections_of_an_image_count(backend):
    rs = np.random.RandomState(3)
    scores = rs.permutation(130).astype(np.float32) / np.float32(256)                 # distinct, in no order
    dets = [det_row(4 * (i % 13), 6 * (i // 13), 4 * (i % 13) + 8, 6 * (i // 13) + 10, scores[i]) for i in range(130)]
    gts = [gt_row(4 * (i % 13), 6 * (i // 13), 8, 10) for i in range(0, 130, 9)]
    images = [{"det": dets, "gt": gts}]
    scorer, got = check(backend, images)
    r = records(scorer, 0)
    assert len(r) == 100 and r["rank"].tolist() == list(range(100))
    assert sorted(np.ascontiguousarray(r["score_bits"]).view(np.float32).tolist(), reverse=True) == sorted(scores.tolist(), reverse=True)[:100]
    assert got["AR1"] <= got["AR10"] <= got["AR100"] and got["AR1"] < got["AR100"]
    # 300 detections of two interleaved classes: the ranking buffer is refilled more than once
    dets = [det_row(3 * (i % 20), 5 * (i // 20), 3 * (i % 20) + 7, 5 * (i // 20) + 9, np.float32((i * 37) % 300) / np.float32(512), i % 2)
            for i in range(300)]
    gts = [gt_row(3 * (i % 20), 5 * (i // 20), 7, 9, i % 2) for i in range(0, 300, 7)]
    check(backend, [{"det": dets, "gt": gts}], K=2)


def test_empty_images_and_classes(backend):
    images = [
        {"det": [], "gt": []},                                                          # nothing at all
        {"det": [], "gt": [gt_row(0, 0, 10, 10, 0), gt_row(0, 0, 50, 50, 2)]},          # ground truth, no detection: cnt == 0
        {"det": [det_row(0, 0, 10, 10, 0.9, 0), det_row(0, 0, 10, 10, 0.8, 1)], "gt": [gt_row(0, 0, 10, 10, 0)]},
        {"det": [], "gt": []},
    ]
    scorer, got = check(backend, images, K=3)
    used, npig, _ = scorer.counters()
    assert used.tolist() == [1, 1, 0] and npig[:, 0].tolist() == [2, 0, 1]
    assert (got["precision"][:, :, 1] == -1).all() and (got["recall"][:, 1] == -1).all()     # class 1: never any ground truth
    assert got["recall"][0, 0, 0, 2] == 0.5 and got["recall"][0, 2, 0, 2] == 0.0
    assert got["AR100"] == 0.25                                                          # the mean skips class 1
    scorer.reset()
    assert scorer.images == 0 and scorer.counters()[0].tolist() == [0, 0, 0]
    empty = scorer.summarize()
    assert (empty["precision"] == -1).all() and empty["AP"] == -1.0


# ---- 8: a seeded random set ---------------------------------------------------------------------------------------------------------
def _random_images(layout, seed=11, n=24, K=3):
    rs = np.random.RandomState(seed)
    obj = np.array([0.25, 0.5, 0.8125, 0.9], dtype=np.float32)
    conf = np.array([0.3, 0.5, 0.75, 1.0], dtype=np.float32)
    images = []
    for _ in range(n):
        div = [1.0, 0.5, 0.625][rs.randint(3)]
        gts = []
        for _ in range(rs.randint(0, 13)):
            x, y = rs.randint(0, 600, 2) * 0.25
            w, h = rs.randint(8, 400, 2) * 0.25
            gts.append(gt_row(x, y, min(w, 200 - x), min(h, 200 - y), rs.randint(K), int(rs.rand() < 0.1)))
        dets = []
        for j in range(rs.randint(0, 41)):
            if gts and rs.rand() < 0.7:                              # near a ground truth, shifted by a few quarter pixels
                g = gts[rs.randint(len(gts))]
                x, y = g[0] + rs.randint(-8, 9) * 0.25, g[1] + rs.randint(-8, 9) * 0.25
                w, h = max(g[2] + rs.randint(-8, 9) * 0.25, 1.0), max(g[3] + rs.randint(-8, 9) * 0.25, 1.0)
                label = int(g[4]) if rs.rand() < 0.8 else rs.randint(K)
            else:
                x, y = rs.randint(0, 600, 2) * 0.25
                w, h = rs.randint(8, 400, 2) * 0.25
                label = rs.randint(K)
            x, y = min(max(x, 0.0), 199.0), min(max(y, 0.0), 199.0)
            x2, y2 = min(x + w, 200.0), min(y + h, 200.0)
            # the kernel receives network coordinates: camera coordinates times the divisor (exact for these divisors? no: the
            # product is rounded to float32 and the division by the divisor rounds again — that is the point of the case)
            box = [np.float32(v * div) for v in (x, y, x2, y2)]
            o, c = obj[rs.randint(4)], conf[rs.randint(4)]
            dets.append(box + ([o, c, label] if layout == "nms" else [np.float32(o * c), label]))
        images.append({"det": dets, "gt": gts, "div": div})
    return images


@pytest.mark.parametrize("layout", ["nms", "track"])
def test_random_set_equals_the_restatement_bit_for_bit(backend, layout):
    images = _random_images(layout)
    scores = {float(d["score"]) for im in images for d in host_dets(im["det"], layout, im["div"])}
    assert len(scores) <= 16 and sum(len(im["det"]) for im in images) > 300
    scorer, got = check(backend, images, K=3, layout=layout, batches=[7, 1, 16], capacity=1024)
    assert 0.0 < got["AP"] < 1.0 and 0.0 < got["AR100"] < 1.0 and got["APs"] > -1 and got["APm"] > -1
    record_parity("score_random_%s_%s" % (layout, backend.type), max_abs_diff=0.0, AP=got["AP"], AR100=got["AR100"],
                  records=int(scorer.counters()[0].sum()))


# ---- 9: capacity, bad arguments -------------------------------------------------------------------------------------------------------
def test_overflow_is_counted_and_nothing_is_written_past_the_arena(backend):
    K, cap = 2, 4
    images = [{"det": [det_row(10 * i, 0, 10 * i + 8, 8, 0.9 - 0.05 * i, i % 2) for i in range(12)], "gt": [gt_row(0, 0, 8, 8, 0)]},
              {"det": [det_row(0, 0, 8, 8, 0.5, 1)], "gt": []}]
    scorer = DetectionScorer(K, capacity=cap, max_gt=4, device=backend)
    nbytes = ops.score_state_bytes(K, cap)
    assert scorer.state.numel() == nbytes
    guarded = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=backend)
    scorer.state = guarded[:nbytes]
    scorer.reset()
    det, cnt, gt, gcnt, _ = pack(images, "nms", backend)
    scorer.add(det, cnt, gt, gcnt)
    used, _, overflow = scorer.counters()
    assert overflow == 2 + 2 + 1 and used.tolist() == [6, 7]
    assert (guarded[nbytes:].cpu() == 0xA5).all()
    with pytest.raises(RuntimeError, match="did not fit"):
        scorer.summarize()
    assert (guarded[nbytes:].cpu() == 0xA5).all()


def test_bad_arguments_are_refused(backend):
    lib = _lib.lib()
    K, cap = 2, 8
    scorer = DetectionScorer(K, capacity=cap, max_gt=4, device=backend)
    det, cnt, gt, gcnt, _ = pack([{"det": [det_row(0, 0, 8, 8, 0.5)], "gt": [gt_row(0, 0, 8, 8)]}], "nms", backend)
    good = scorer.params

    def match(B=1, layout=0, params=good, state=scorer.state.data_ptr(), det_p=det.data_ptr(), max_gt=1, base=0, cap_=cap):
        return lib.sy_score_match(det_p, cnt.data_ptr(), B, 1, layout, None, gt.data_ptr(), gcnt.data_ptr(), max_gt, base,
                                  C.byref(params), state, K, cap_, ops.stream_of(det))

    def params(**kw):
        p = ops.score_params(IOU_THRS, REC_THRS, AREA_RNG, MAX_DETS, np.spacing(1))
        for name, v in kw.items():
            if name == "maxdet0":
                p.maxdet[0] = v
            else:
                setattr(p, name, v)
        return p

    assert match() == 0 and match(B=0) == 0
    assert match(B=-1) == 1 and match(layout=3) == 1 and match(state=None) == 1 and match(det_p=None) == 1
    assert match(max_gt=257) == 1 and match(max_gt=0) == 1 and match(base=1 << 25) == 1 and match(cap_=0) == 1
    assert match(params=params(n_area=5)) == 1 and match(params=params(n_thr=17)) == 1 and match(params=params(maxdet0=101)) == 1
    assert match(params=params(n_rec=129)) == 1 and match(params=params(n_maxdet=0)) == 1
    ws = torch.empty(ops.score_workspace_bytes(K, cap), dtype=torch.uint8, device=backend)
    pr = torch.empty((10, 101, K, 4, 3), dtype=torch.float64, device=backend)
    rc = torch.empty((10, K, 4, 3), dtype=torch.float64, device=backend)

    def acc(state=scorer.state.data_ptr(), ws_p=ws.data_ptr(), pr_p=pr.data_ptr(), rc_p=rc.data_ptr(), p=good, k=K):
        return lib.sy_score_accumulate(state, k, cap, C.byref(p), ws_p, pr_p, rc_p, None, ops.stream_of(det))

    assert acc() == 0                                            # (the overflow output is optional)
    assert acc(state=None) == 1 and acc(ws_p=None) == 1 and acc(pr_p=None) == 1 and acc(rc_p=None) == 1 and acc(k=0) == 1
    assert acc(p=params(n_area=5)) == 1 and acc(p=params(maxdet0=0)) == 1
    assert lib.sy_score_reset(None, K, cap, ops.stream_of(det)) == 1 and lib.sy_score_reset(scorer.state.data_ptr(), 0, cap, None) == 1
    assert lib.sy_score_state_bytes(0, 8) == -1 and lib.sy_score_workspace_bytes(8, 0) == -1
    assert lib.sy_score_state_bytes(8, 100) == 192 + 8 * 100 * 32 and lib.sy_score_workspace_bytes(8, 100) == 8 * 128 * 16
    with pytest.raises(ValueError):
        DetectionScorer(K, capacity=cap, max_gt=300, device=backend)
    with pytest.raises(ValueError):
        scorer.add(det, cnt, gt, gcnt, layout="xyxy")

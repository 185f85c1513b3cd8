"""sy_postprocess_rows: the device NMS with one sy_det_policy per batch row (thresholds, class mask, class-agnostic mode, caps on
the candidates and on the detections), ops.postprocess_rows, DetectionPolicy and postprocess(class_agnostic=True).

Every comparison is bit-exact (torch.equal on det, array_equal on index, equal counts).  The yardsticks are the semantics of the
header comment restated with what exists already: the old entry point (ops.postprocess) and the oracle for default rows; the
reference's yolox.utils.postprocess restatement (oracle/ref_shim) and an independent numpy walk for the agnostic mode; and, for
the class mask and max_candidates, the RESTRICTION: the remaining candidates computed in numpy, gathered in ascending anchor
order into a smaller tensor, run through the old entry point (or the numpy walk), indices mapped back."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from streamyolo_amd import _lib, ops
from streamyolo_amd.postprocess import postprocess_device
from oracle import streamyolo_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "streamyolo_hip.h")
NC = 8


def _shim_postprocess():
    """yolox.utils.postprocess of oracle/ref_shim, loaded by path (nothing named `yolox` enters sys.modules)."""
    spec = importlib.util.spec_from_file_location("_policy_test_yolox_utils",
                                                  os.path.join(ROOT, "oracle", "ref_shim", "yolox", "utils", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.postprocess


def _random_preds(B, A, nc, seed, img=(600.0, 960.0), tie_free=True):
    """tests/test_kernels_misc.py::_random_preds."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(B, A, 5 + nc)
    p[..., 0] = torch.rand(B, A, generator=g) * img[1]
    p[..., 1] = torch.rand(B, A, generator=g) * img[0]
    p[..., 2] = torch.rand(B, A, generator=g) * 200 + 8
    p[..., 3] = torch.rand(B, A, generator=g) * 200 + 8
    p[..., 4] = torch.rand(B, A, generator=g)
    p[..., 5:] = torch.rand(B, A, nc, generator=g)
    if tie_free:
        p[..., 4] = p[..., 4] * 0.5 + 0.25 + torch.arange(A)[None] * 2.0 ** -20
    return p


def _clustered_preds(B, A, nc, seed):
    """Boxes in clusters (suppression happens, across classes too), tie-free scores."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(B, A, 5 + nc)
    for b in range(B):
        centres = torch.rand(max(1, A // 6), 2, generator=g) * 200 + 50
        which = torch.randint(0, centres.shape[0], (A,), generator=g)
        p[b, :, 0:2] = centres[which] + torch.randn(A, 2, generator=g) * 4
        p[b, :, 2:4] = torch.rand(A, 2, generator=g) * 40 + 10
        p[b, :, 4] = torch.rand(A, generator=g) * 0.5 + 0.25 + torch.arange(A) * 2.0 ** -20
        p[b, :, 5:] = torch.rand(A, nc, generator=g)
    return p


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------
def _parts(p, nc):
    """One image [A, 5+nc] -> (corner boxes, arg-max class (first maximum), class_conf, score), float32."""
    a = p.numpy().astype(np.float32)
    box = np.stack([a[:, 0] - a[:, 2] / 2, a[:, 1] - a[:, 3] / 2, a[:, 0] + a[:, 2] / 2, a[:, 1] + a[:, 3] / 2], 1)
    cls = a[:, 5:5 + nc].argmax(1)
    cconf = a[:, 5:5 + nc].max(1)
    return box, cls, cconf, (a[:, 4] * cconf).astype(np.float32)


def _remaining(p, nc, conf, classes=None, max_candidates=0):
    """Semantics 1 + 2: anchors of the remaining candidates in NMS order (score descending, ties by ascending anchor)."""
    _, cls, _, score = _parts(p, nc)
    ok = score >= np.float32(conf)
    if classes is not None:
        ok &= np.isin(cls, np.asarray(sorted(classes), dtype=np.int64))
    cand = np.nonzero(ok)[0]
    cand = cand[np.argsort(-score[cand], kind="stable")]
    return cand[:max_candidates] if max_candidates > 0 else cand


def _walk(p, nc, order, thr, class_aware=False):
    """_greedy_nms_reference of tests/test_kernels_misc.py over the anchors `order`, without the class check (agnostic)."""
    box, cls, _, _ = _parts(p, nc)
    keep = []
    for i in order:
        ok = True
        for j in keep:
            if class_aware and cls[j] != cls[i]:
                continue
            lt = np.maximum(box[i, :2], box[j, :2]); rb = np.minimum(box[i, 2:], box[j, 2:])
            wh = np.maximum(rb - lt, np.float32(0))
            inter = wh[0] * wh[1]
            a = (box[i, 2] - box[i, 0]) * (box[i, 3] - box[i, 1]); b = (box[j, 2] - box[j, 0]) * (box[j, 3] - box[j, 1])
            if inter / (a + b - inter) > np.float32(thr):
                ok = False
                break
        if ok:
            keep.append(int(i))
    return keep


def _det_rows(p, nc, anchors):
    """The output rows (x1, y1, x2, y2, obj, class_conf, class) of the given anchors, fp32 torch arithmetic."""
    q = p[torch.as_tensor(np.asarray(anchors, dtype=np.int64))]
    cconf, cls = torch.max(q[:, 5:5 + nc], 1)
    return torch.stack([q[:, 0] - q[:, 2] / 2, q[:, 1] - q[:, 3] / 2, q[:, 0] + q[:, 2] / 2, q[:, 1] + q[:, 3] / 2,
                        q[:, 4], cconf, cls.float()], 1)


def _restriction(p, nc, backend, conf, thr, classes=None, agnostic=False, max_candidates=0, max_det=0):
    """The yardstick of one image under a policy: (det [n, 7], anchors [n])."""
    rem = np.sort(_remaining(p, nc, conf, classes, max_candidates))
    if rem.size == 0:
        return torch.zeros((0, 7)), np.zeros(0, np.int32)
    sub = p[torch.from_numpy(rem)].contiguous()
    if agnostic:
        keep = rem[np.asarray(_walk(sub, nc, _remaining(sub, nc, conf), thr), dtype=np.int64)]
        det = _det_rows(p, nc, keep)
    else:
        d, i, c = ops.postprocess(sub[None].to(backend), nc, conf, thr)       # the old entry point on the restricted tensor
        n = int(c[0])
        keep, det = rem[i[0, :n].cpu().numpy().astype(np.int64)], d[0, :n].cpu()
    if max_det > 0:
        keep, det = keep[:max_det], det[:max_det]
    return det, keep.astype(np.int32)


def _record(conf=0.01, thr=0.65, classes=None, agnostic=False, max_candidates=0, max_det=0):
    return ops.det_policy_record(conf, thr, range(NC) if classes is None else classes, agnostic, max_candidates, max_det)


def _rows(pred, records, backend, nc=NC):
    """ops.postprocess_rows -> [(det [n, 7] cpu, anchors [n] int32)] per image."""
    det, idx, cnt = ops.postprocess_rows(pred.to(backend), nc, ops.det_policy_table(records, backend))
    cnt = cnt.cpu().tolist()
    return [(det[b, :n].cpu(), idx[b, :n].cpu().numpy()) for b, n in enumerate(cnt)]


def _assert_same(got, want, what=""):
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), what      # count and order
    assert torch.equal(got[0], want[0]), what


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 64, 257, 1500])
def test_default_rows_equal_the_old_entry_point(backend, A):
    pred = _random_preds(2, A, NC, seed=A)
    pred[1, :, 4] *= 0.02                       # second image: most anchors fall under the threshold
    got = _rows(pred, [_record()] * 2, backend)
    det, idx, cnt = ops.postprocess(pred.to(backend), NC, 0.01, 0.65)
    ref = O.postprocess(pred, NC, 0.01, 0.65)
    for b in range(2):
        n = int(cnt[b])
        _assert_same(got[b], (det[b, :n].cpu(), idx[b, :n].cpu().numpy()), (A, b))
        _assert_same(got[b], (ref[b][0], ref[b][1].numpy().astype(np.int32)), (A, b))
    assert len(got[0][1]) > 0


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def test_class_agnostic_equals_the_reference_and_an_independent_walk(backend):
    """A = 1: yolox.utils.postprocess itself cannot take a one-anchor image (its `.squeeze()` turns the confidence mask into a
    scalar and the indexing that follows adds a dimension: IndexError, in the reference as in its restatement), so that shape is
    held against the independent walk and the rows built from it; the in-place rewrite is still compared (it happens first)."""
    shim = _shim_postprocess()
    differs = False
    for A in (1, 64, 65, 400):
        pred = _clustered_preds(2, A, NC, seed=100 + A)
        mine, theirs = pred.clone().to(backend), pred.clone()
        got = sy.postprocess(mine, NC, 0.01, 0.65, class_agnostic=True)
        if A == 1:
            with pytest.raises(IndexError):
                shim(theirs, NC, 0.01, 0.65, class_agnostic=True)
            want = [_det_rows(pred[b], NC, [0]) for b in range(2)]
        else:
            want = shim(theirs, NC, 0.01, 0.65, class_agnostic=True)
        assert torch.equal(mine.cpu(), theirs)                                   # the in-place corner rewrite of `prediction`
        _, idx, cnt = postprocess_device(pred.to(backend), NC, 0.01, 0.65, class_agnostic=True)
        for b in range(2):
            assert (got[b] is None) == (want[b] is None)
            assert got[b] is not None and torch.equal(got[b].cpu(), want[b]), (A, b)
            keep = _walk(pred[b], NC, _remaining(pred[b], NC, 0.01), 0.65)
            assert np.array_equal(idx[b, :int(cnt[b])].cpu().numpy(), np.asarray(keep, dtype=np.int32)), (A, b)
            assert torch.equal(got[b].cpu(), _det_rows(pred[b], NC, keep)), (A, b)
            differs = differs or keep != _walk(pred[b], NC, _remaining(pred[b], NC, 0.01), 0.65, class_aware=True)
    assert differs                              # (precondition: suppression across classes happened somewhere)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clustered():
    return _clustered_preds(1, 300, NC, seed=7)


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("classes", [[3], [0, 1, 2, 3, 4, 6, 7], []])
def test_class_mask_equals_the_restriction(backend, clustered, classes, agnostic):
    got = _rows(clustered, [_record(classes=classes, agnostic=agnostic)], backend)[0]
    _assert_same(got, _restriction(clustered[0], NC, backend, 0.01, 0.65, classes=classes, agnostic=agnostic))
    assert (len(got[1]) == 0) == (not classes)
    assert set(got[0][:, 6].int().tolist()) <= set(classes)


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 305])
def test_max_candidates_equals_the_restriction(backend, clustered, k, agnostic):
    assert len(_remaining(clustered[0], NC, 0.01)) == 300                       # (305 = all + 5)
    got = _rows(clustered, [_record(agnostic=agnostic, max_candidates=k)], backend)[0]
    _assert_same(got, _restriction(clustered[0], NC, backend, 0.01, 0.65, agnostic=agnostic, max_candidates=k))
    assert 0 < len(got[1]) <= k


@pytest.mark.parametrize("agnostic", [False, True])
def test_max_candidates_cut_inside_a_run_of_tied_scores(backend, agnostic):
    """Anchors 40..99 share one score exactly: a cut after 70 candidates falls inside the run, the anchor index decides."""
    pred = _clustered_preds(1, 160, NC, seed=11)
    pred[0, 40:100, 4] = 0.5
    pred[0, 40:100, 5:] = 0.0
    pred[0, 40:100, 5 + 2] = 0.75
    _, _, _, score = _parts(pred[0], NC)
    order = _remaining(pred[0], NC, 0.01)
    first = int(np.nonzero(score[order] == score[40])[0][0])
    k = first + 25
    assert first > 0 and np.array_equal(order[first:first + 60], np.arange(40, 100))      # the run, in anchor order
    got = _rows(pred, [_record(agnostic=agnostic, max_candidates=k)], backend)[0]
    _assert_same(got, _restriction(pred[0], NC, backend, 0.01, 0.65, agnostic=agnostic, max_candidates=k))
    assert not set(got[1].tolist()) & set(range(65, 100))                       # anchors 40..64 of the run remained, 65..99 did not


def test_max_candidates_drops_the_largest_coordinate(backend):
    """The lowest-scoring candidate reaches furthest right: cut away, the class offset unit of the rest is another number."""
    pred = _clustered_preds(1, 130, NC, seed=13)
    pred[0, 77, 0], pred[0, 77, 4] = 5000.0, 0.05
    assert len(_remaining(pred[0], NC, 0.01)) == 130
    box, _, _, _ = _parts(pred[0], NC)
    rem = _remaining(pred[0], NC, 0.01, max_candidates=129)
    assert 77 not in rem and len(rem) == 129 and box[rem].max() < box[77].max()
    got = _rows(pred, [_record(max_candidates=129)], backend)[0]
    _assert_same(got, _restriction(pred[0], NC, backend, 0.01, 0.65, max_candidates=129))
    _assert_same(got, (_det_rows(pred[0], NC, _walk(pred[0], NC, rem, 0.65, class_aware=True)),
                       np.asarray(_walk(pred[0], NC, rem, 0.65, class_aware=True), dtype=np.int32)))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_masked_boxes_do_not_suppress(backend):
    pred = torch.zeros(1, 3, 5 + NC)
    pred[0, 0, :5] = torch.tensor([100.0, 100.0, 50.0, 50.0, 0.9]); pred[0, 0, 5 + 0] = 0.9        # class 0, the top score
    pred[0, 1, :5] = torch.tensor([102.0, 101.0, 50.0, 50.0, 0.8]); pred[0, 1, 5 + 1] = 0.9        # class 1, IoU ~ 0.9 with it
    pred[0, 2, :5] = torch.tensor([300.0, 300.0, 20.0, 20.0, 0.7]); pred[0, 2, 5 + 0] = 0.9        # class 0, far away
    everything = _rows(pred, [_record(thr=0.5, agnostic=True)], backend)[0]
    without0 = _rows(pred, [_record(thr=0.5, agnostic=True, classes=[1, 2, 3, 4, 5, 6, 7])], backend)[0]
    aware = _rows(pred, [_record(thr=0.5)], backend)[0]
    assert everything[1].tolist() == [0, 2] and without0[1].tolist() == [1] and aware[1].tolist() == [0, 1, 2]
    assert without0[0][0].tolist() == _det_rows(pred[0], NC, [1])[0].tolist()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
def test_max_det_is_a_prefix_of_the_uncapped_list(backend, agnostic):
    pred = _random_preds(1, 400, NC, seed=21, img=(2400.0, 3840.0))
    full = _rows(pred, [_record(agnostic=agnostic)], backend)[0]
    kept = len(full[1])
    assert kept > 130                                                            # the caps cross two chunk boundaries
    caps = [1, 63, 64, 65, kept, kept + 1]
    got = _rows(pred.expand(len(caps), -1, -1).contiguous(), [_record(agnostic=agnostic, max_det=c) for c in caps], backend)
    for cap, g in zip(caps, got):
        n = min(kept, cap)
        _assert_same(g, (full[0][:n], full[1][:n]), cap)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent(backend):
    pred = _clustered_preds(4, 200, NC, seed=31)
    recs = [_record(0.01, 0.65, agnostic=True, max_det=20), _record(0.3, 0.45, classes=[1, 2, 5]),
            _record(0.01, 0.65, max_candidates=100), _record(0.3, 0.45, agnostic=True, classes=[0, 3, 4, 6, 7], max_candidates=70, max_det=9)]
    alone = [[_rows(pred[b:b + 1], [r], backend)[0] for r in recs] for b in range(4)]          # [image][policy]
    assert len({tuple(alone[0][k][1].tolist()) for k in range(4)}) == 4                         # the policies differ in effect
    for perm in ([0, 1, 2, 3], [2, 0, 3, 1], [3, 2, 1, 0]):
        got = _rows(pred, [recs[k] for k in perm], backend)
        for b, k in enumerate(perm):
            _assert_same(got[b], alone[b][k], (perm, b))
    for b in range(4):                                                                          # ... and each is its yardstick
        _assert_same(alone[b][1], _restriction(pred[b], NC, backend, 0.3, 0.45, classes=[1, 2, 5]))
        _assert_same(alone[b][3], _restriction(pred[b], NC, backend, 0.3, 0.45, classes=[0, 3, 4, 6, 7], agnostic=True,
                                               max_candidates=70, max_det=9))


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_empty_and_degenerate_rows(backend):
    pred = _random_preds(2, 100, NC, seed=9)
    quiet = pred.clone()
    quiet[..., 4] = 0.0                                                          # nothing over conf_thre
    for agnostic in (False, True):
        assert [len(r[1]) for r in _rows(quiet, [_record(agnostic=agnostic, max_det=5, max_candidates=7)] * 2, backend)] == [0, 0]
        one = _rows(pred[:, :1].contiguous(), [_record(agnostic=agnostic)] * 2, backend)       # A = 1
        assert [r[1].tolist() for r in one] == [[0], [0]]
        assert torch.equal(one[1][0], _det_rows(pred[1, :1], NC, [0]))
        got = _rows(pred, [_record(classes=[], agnostic=agnostic), _record(agnostic=agnostic)], backend)   # a zero mask beside a full row
        assert len(got[0][1]) == 0
        _assert_same(got[1], _restriction(pred[1], NC, backend, 0.01, 0.65, agnostic=agnostic))
    zero = torch.zeros(2 * ops.DET_POLICY_BYTES, dtype=torch.uint8, device=backend)             # the all-zero record
    assert ops.postprocess_rows(pred.to(backend), NC, zero)[2].cpu().tolist() == [0, 0]


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_policy_struct_size_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu\\n", sizeof(sy_det_policy));return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    size = int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    assert size == ctypes.sizeof(_lib.DetPolicy) == np.dtype(_lib.DetPolicy).itemsize == ops.DET_POLICY_BYTES == 40


def test_rows_entry_point_rejects_bad_arguments(backend):
    lib = _lib.lib()
    B, A = 1, 8
    ws = ops.PostprocessWorkspace(B, A, backend)
    tab = ops.det_policy_table([_record()], backend)

    def call(nc, pred, rows=tab, det=ws.det, index=ws.index, count=ws.count, work=ws.ws, max_det=A):
        p = lambda t: None if t is None else t.data_ptr()                       # noqa: E731
        return lib.sy_postprocess_rows(p(pred), B, A, nc, p(rows), max_det, p(det), p(index), p(count), p(work), ops.stream_of(ws.det))
    assert call(128, torch.zeros(B, A, 5 + 128, device=backend)) == 0
    assert call(129, torch.zeros(B, A, 5 + 129, device=backend)) == _lib.SY_ERR_UNSUPPORTED
    pred = torch.zeros(B, A, 5 + NC, device=backend)
    assert call(NC, pred) == 0
    for k in ("rows", "det", "index", "count", "work"):
        assert call(NC, pred, **{k: None}) == 1, k
    assert call(NC, None) == 1 and call(NC, pred, max_det=0) == 1 and call(0, pred) == 1
    big = ops.PostprocessWorkspace(1, 16385, backend, max_det=8)                # above the LDS sort limit, as sy_postprocess
    assert lib.sy_postprocess_rows(pred.data_ptr(), 1, 16385, NC, tab.data_ptr(), 8, big.det.data_ptr(), big.index.data_ptr(),
                                   big.count.data_ptr(), big.ws.data_ptr(), ops.stream_of(pred)) == _lib.SY_ERR_UNSUPPORTED


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_detection_policy_validation():
    P = sy.DetectionPolicy
    for kw in (dict(conf_thre=float("nan")), dict(conf_thre=float("inf")), dict(nms_thresh=float("nan")), dict(nms_thresh=-0.1),
               dict(conf_thre="x"), dict(classes=[-1]), dict(classes=[1.5]), dict(max_candidates=0), dict(max_det=0),
               dict(max_det=-3), dict(max_candidates=2.5), dict(max_det=True)):
        with pytest.raises(ValueError):
            P(**kw)
    with pytest.raises(ValueError):
        P(classes=[8]).record(8, 0.01, 0.65)                                    # ids lie in [0, num_classes)
    with pytest.raises(ValueError):
        P().record(129, 0.01, 0.65)
    with pytest.raises(ValueError):
        P().record(8, float("nan"), 0.65)
    assert P().record(8, 0.01, 0.65) == _record()
    assert P(classes=[]).record(8, 0.01, 0.65)[6] == (0, 0, 0, 0)               # allowed: nothing is reported
    assert P(0.3, 0.45, classes=(5, 1, 5), class_agnostic=True, max_candidates=7, max_det=3).record(8, 0.01, 0.65) == \
        (0.3, 0.45, 1, 7, 3, 0, (0b100010, 0, 0, 0))
    assert P(classes=range(100, 128)).record(128, 0.5, 0.5)[6] == (0, 0, 0, 0xfffffff0)


# ---- 11 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def survey_preds():
    pred = _random_preds(2, 11850, NC, seed=41, img=(2400.0, 3840.0))
    pred[1, :, 4] *= 0.02
    return pred


@pytest.mark.gpu
def test_default_rows_at_the_survey_size(survey_preds):
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda:0")
    got = _rows(survey_preds, [_record()] * 2, dev)
    det, idx, cnt = ops.postprocess(survey_preds.to(dev), NC, 0.01, 0.65)
    for b in range(2):
        n = int(cnt[b])
        assert n > 0
        _assert_same(got[b], (det[b, :n].cpu(), idx[b, :n].cpu().numpy()), b)


@pytest.mark.gpu
def test_capped_rows_at_the_survey_size(survey_preds):
    """Row 0 agnostic, row 1 class-aware, both with max_candidates = 4096 and max_det = 100, at A = 11850."""
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda:0")
    pred = survey_preds.clone()
    pred[1] = pred[0]
    got = _rows(pred, [_record(agnostic=True, max_candidates=4096, max_det=100), _record(max_candidates=4096, max_det=100)], dev)
    assert len(_remaining(pred[0], NC, 0.01)) > 4096
    # the agnostic walk stops at 100 survivors too: the yardstick's walk over 4096 boxes is cut there (a prefix is a prefix)
    rem = _remaining(pred[0], NC, 0.01, max_candidates=4096)
    box = _parts(pred[0], NC)[0]
    keep = []
    for i in rem:
        if len(keep) == 100:
            break
        k = np.asarray(keep, dtype=np.int64)
        lt, rb = np.maximum(box[i, :2], box[k, :2]), np.minimum(box[i, 2:], box[k, 2:])
        wh = np.maximum(rb - lt, np.float32(0))
        inter = wh[:, 0] * wh[:, 1]
        area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        if not (inter / (area[i] + area[k] - inter) > np.float32(0.65)).any():
            keep.append(int(i))
    assert len(keep) == 100
    _assert_same(got[0], (_det_rows(pred[0], NC, keep), np.asarray(keep, dtype=np.int32)))
    _assert_same(got[1], _restriction(pred[1], NC, dev, 0.01, 0.65, max_candidates=4096, max_det=100))

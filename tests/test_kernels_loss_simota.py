"""SimOTA matching of sy_tal_loss where dynamic k > 1 and the ten-entry lists of tal_match_kernel fill.

The golden and the random inputs of test_kernels_loss.py give every ground truth k = 1: the per-thread sorted lists, the per-wave merge,
the four-list merge, kg = int(sum) and the kg > C clamp never decide an outcome there.  Here every anchor inside a ground truth predicts
that box almost perfectly, so the ten largest IoUs sum to 8-9, and the assignment is compared EXACTLY with a float64 restatement
(`simota_f64`).  A discrete outcome can be compared exactly only where fp32 rounding cannot flip it: the restatement also returns the
decision margins of its input, and every test asserts them before it calls the kernel (they are properties of the input alone).
The loss entries and the gradient are checked against the fp32 oracle with the tolerances of test_kernels_loss.py."""
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import streamyolo_oracle as O
from streamyolo_amd import ops

CFG = O.OracleConfig.named("nano")
# fp32 error of a cost of size ~10 or of a sum of ten IoUs is ~1e-5: two orders of magnitude below these
COST_MARGIN, K_MARGIN, GEO_MARGIN = 1e-3, 1e-3, 5e-3
HW_315 = ((12, 20), (6, 10), (3, 5))
HW_32 = ((4, 6), (2, 3), (1, 2))
HW_840 = ((20, 32), (10, 16), (5, 8))
HW_5040 = ((48, 80), (24, 40), (12, 20))
HW_4032 = ((12, 256), (6, 128), (3, 64))
GT_OVERLAP = ((1, 40.3, 30.7, 50, 40), (2, 60.9, 40.1, 56, 44), (5, 120.6, 60.2, 60, 50), (3, 110.3, 50.9, 30, 30))


def simota_f64(raw, hw, strides, gt, nc, dtype=torch.float64):
    """SimOTA assignment of ONE image (tal_head.py get_in_boxes_info / get_assignments / dynamic_k_matching) in `dtype`, plain torch.
    raw [A, 5+nc] head outputs, gt [G, 5] rows (cls, cx, cy, w, h).  Returns a dict: `matched` [A] (ground-truth index, -1 =
    background), `iou` [A] (IoU with the matched ground truth, 0 on background), `pair_iou` [G, A] (IoU of every pair, 0 off the
    candidates), and the margins / shape figures the tests assert on (see the module docstring)."""
    A = raw.shape[0]
    gx, gy, gs = O.anchor_grid(hw, strides, dtype)
    raw = raw.to(dtype)
    G = gt.shape[0]
    gtb, gtc = gt[:, 1:5].to(dtype), gt[:, 0].long()
    boxes = torch.stack([(raw[:, 0] + gx) * gs, (raw[:, 1] + gy) * gs, raw[:, 2].exp() * gs, raw[:, 3].exp() * gs], 1)
    # candidates: anchor centre in any box or in any 2.5-stride centre square
    xc, yc = gx * gs + 0.5 * gs, gy * gs + 0.5 * gs
    bl, br = (gtb[:, 0] - 0.5 * gtb[:, 2])[:, None], (gtb[:, 0] + 0.5 * gtb[:, 2])[:, None]
    bt, bb = (gtb[:, 1] - 0.5 * gtb[:, 3])[:, None], (gtb[:, 1] + 0.5 * gtb[:, 3])[:, None]
    d_box = torch.stack([xc[None] - bl, yc[None] - bt, br - xc[None], bb - yc[None]], 2)             # [G, A, 4]
    rad = 2.5 * gs[None]
    d_ctr = torch.stack([xc[None] - (gtb[:, 0:1] - rad), yc[None] - (gtb[:, 1:2] - rad),
                         (gtb[:, 0:1] + rad) - xc[None], (gtb[:, 1:2] + rad) - yc[None]], 2)
    geo_margin = float(torch.minimum(d_box.abs().min(), d_ctr.abs().min()))
    in_box, in_ctr = d_box.min(2).values > 0, d_ctr.min(2).values > 0
    ci = (in_box.any(0) | in_ctr.any(0)).nonzero().squeeze(1)
    C = len(ci)
    both = (in_box & in_ctr)[:, ci]
    # cost
    ious = O.pairwise_iou_cxcywh(gtb, boxes[ci])                                                       # [G, C]
    prob = (torch.sigmoid(raw[ci, 5:]) * torch.sigmoid(raw[ci, 4])[:, None]).sqrt()
    onehot = F.one_hot(gtc, nc).to(dtype)
    cls_cost = F.binary_cross_entropy(prob[None].expand(G, -1, -1), onehot[:, None, :].expand(-1, C, -1), reduction="none").sum(-1)
    cost = cls_cost + 3.0 * (-torch.log(ious + 1e-8)) + 100000.0 * (~both).to(dtype)
    # dynamic k and the k cheapest candidates
    top_iou = torch.topk(ious, min(10, C), dim=1)
    ksum = top_iou.values.sum(1)
    ks = torch.clamp(ksum.floor().long(), min=1)
    k_margin = float(torch.minimum(ksum - ksum.floor(), ksum.floor() + 1 - ksum).min())
    order = torch.sort(cost, dim=1)
    match = torch.zeros(G, C, dtype=torch.bool)
    cost_margin, cost_margin_ulp = float("inf"), float("inf")
    ulp32 = lambda v: float(np.spacing(np.float32(abs(float(v)))))
    for g in range(G):
        k = int(ks[g])
        match[g, order.indices[g, :k]] = True
        if k < C:
            gap = float(order.values[g, k] - order.values[g, k - 1])
            cost_margin = min(cost_margin, gap)
            cost_margin_ulp = min(cost_margin_ulp, gap / ulp32(order.values[g, k]))
    # anchors claimed more than once go to the arg-min cost over all ground truths
    multi = match.sum(0) > 1
    n_conflict = int(multi.sum())
    if n_conflict:
        two = torch.topk(cost[:, multi], 2, dim=0, largest=False).values
        cost_margin = min(cost_margin, float((two[1] - two[0]).min()))
        cost_margin_ulp = min(cost_margin_ulp, min((float(b - a) / ulp32(b)) for a, b in zip(two[0], two[1])))
        amin = cost[:, multi].argmin(0)
        match[:, multi] = False
        match[amin, multi] = True
    fg = match.any(0)
    matched = torch.full((A,), -1, dtype=torch.int32)
    matched[ci[fg]] = match[:, fg].to(torch.int8).argmax(0).to(torch.int32)
    pair_iou = torch.zeros(G, A, dtype=dtype)
    pair_iou[:, ci] = ious
    iou = torch.zeros(A, dtype=dtype)
    iou[ci[fg]] = (match.to(dtype) * ious).sum(0)[fg]

    # how the ten best of either key fall on tal_match_kernel's threads (anchor % 256) and waves
    def crowd(idx):
        t = ci[idx] % 256
        return int(torch.bincount(t).max()), int(torch.bincount(t // 64).max())
    n10 = min(10, C)
    by_iou = [crowd(top_iou.indices[g]) for g in range(G)]
    by_cost = [crowd(order.indices[g, :n10]) for g in range(G)]
    return dict(matched=matched, iou=iou, pair_iou=pair_iou, cand=ci, G=G, C=C, k=ks.tolist(), ksum=ksum.tolist(),
                n_conflict=n_conflict, n_both=both.sum(1).tolist(), cost_margin=cost_margin, cost_margin_ulp32=cost_margin_ulp,
                k_margin=k_margin, geo_margin=geo_margin,
                lane_iou=[c[0] for c in by_iou], wave_iou=[c[1] for c in by_iou],
                lane_cost=[c[0] for c in by_cost], wave_cost=[c[1] for c in by_cost])


def _make_raw(hw, strides, images, nc, seed, noise, level0_only):
    """randn * 0.5 like the other loss tests; every anchor whose centre lies strictly inside a ground truth then predicts that box
    (the decode's inverse, + randn * noise per channel) and leans to its class and to objectness by +1."""
    g = torch.Generator().manual_seed(seed)
    A = sum(h * w for h, w in hw)
    raw = torch.randn(len(images), A, 5 + nc, generator=g) * 0.5
    gx, gy, gs = O.anchor_grid(hw, strides)
    xc, yc = gx * gs + 0.5 * gs, gy * gs + 0.5 * gs
    for i, rows in enumerate(images):
        for (c, bx, by, bw, bh) in rows:
            idx = (((xc - bx).abs() < bw / 2) & ((yc - by).abs() < bh / 2)).nonzero().squeeze(1)
            if level0_only:
                idx = idx[idx < hw[0][0] * hw[0][1]]
            n = len(idx)
            raw[i, idx, 0] = bx / gs[idx] - gx[idx] + torch.randn(n, generator=g) * noise
            raw[i, idx, 1] = by / gs[idx] - gy[idx] + torch.randn(n, generator=g) * noise
            raw[i, idx, 2] = torch.log(bw / gs[idx]) + torch.randn(n, generator=g) * noise
            raw[i, idx, 3] = torch.log(bh / gs[idx]) + torch.randn(n, generator=g) * noise
            raw[i, idx, 4] += 1.0
            raw[i, idx, 5 + int(c)] += 1.0
    return raw


def _random_boxes(n, seed=13):
    """n boxes, cx in [10, 246], cy in [10, 150], w in [12, 62], h in [12, 52], classes 0..7.  Even integer sizes and centres at
    x.x3: an edge or a centre-square side is then >= 0.03 px from every anchor centre (those are integers)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 4, generator=g)
    cls = torch.randint(0, 8, (n,), generator=g)
    cx = torch.floor((10 + 235.9 * u[:, 0]) * 10) / 10 + 0.03
    cy = torch.floor((10 + 139.9 * u[:, 1]) * 10) / 10 + 0.03
    w = 2 * torch.floor(6 + 25.5 * u[:, 2])
    h = 2 * torch.floor(6 + 20.5 * u[:, 3])
    return tuple((int(c), round(float(x), 2), round(float(y), 2), float(ww), float(hh)) for c, x, y, ww, hh in zip(cls, cx, cy, w, h))


@functools.lru_cache(maxsize=None)
def _case(hw, images, noise, seed=0, nc=8, max_labels=120, level0_only=False, use_l1=True):
    """Inputs and every reference of one scenario, computed once and shared by the backends (nothing here is modified later)."""
    c = types.SimpleNamespace()
    c.hw, c.nc, c.max_labels, c.use_l1 = [tuple(x) for x in hw], nc, max_labels, use_l1
    c.cfg = dataclasses.replace(CFG, num_classes=nc)
    B = len(images)
    c.A = sum(h * w for h, w in hw)
    c.raw = _make_raw(c.hw, c.cfg.strides, images, nc, seed, noise, level0_only)
    c.lab = torch.zeros(B, max_labels, 5)
    c.sup = torch.zeros(B, max_labels, 5)
    for i, rows in enumerate(images):
        for j, r in enumerate(rows):
            c.lab[i, j] = torch.tensor([float(v) for v in r])
            # support box: the label a few pixels away and a few percent larger / smaller (unequal trend weights)
            c.sup[i, j] = torch.tensor([r[0], r[1] + 3.0 + (j % 3), r[2] - 2.0, r[3] * (1.04 + 0.02 * (j % 2)), r[4] * 0.97])
    c.num_gt = sum(len(rows) for rows in images)
    c.ref, c.e32 = [], 0.0
    for i, rows in enumerate(images):
        if not rows:
            c.ref.append(None)
            continue
        r64 = simota_f64(c.raw[i], c.hw, c.cfg.strides, c.lab[i, :len(rows)], nc)
        r32 = simota_f64(c.raw[i], c.hw, c.cfg.strides, c.lab[i, :len(rows)], nc, torch.float32)
        assert torch.equal(r32["cand"], r64["cand"])
        fg = (r64["matched"] >= 0).nonzero().squeeze(1)
        mg = r64["matched"][fg].long()
        # the fp32 restatement's IoU of the pairs float64 matched (its own matching plays no part)
        c.e32 = max(c.e32, float((r32["pair_iou"][mg, fg].double() - r64["pair_iou"][mg, fg]).abs().max()))
        c.ref.append(r64)
    # fp32 oracle loss and autograd gradient (without the L1 term: total - l1, whose gradient drops exactly that term)
    r = c.raw.clone().requires_grad_(True)
    levels, a0 = [], 0
    for (h, w) in c.hw:
        levels.append(r[:, a0:a0 + h * w].permute(0, 2, 1).reshape(B, 5 + nc, h, w))
        a0 += h * w
    out = O.tal_loss(levels, c.lab, c.sup, c.cfg)
    total = out["total_loss"] if use_l1 else out["total_loss"] - out["l1_loss"]
    total.backward()
    c.grad = r.grad
    want = {k: float(torch.as_tensor(out[k]).detach()) for k in ("iou_loss", "l1_loss", "conf_loss", "cls_loss", "num_fg")}
    want["total_loss"] = float(total.detach())
    if not use_l1:
        want["l1_loss"] = 0.0
    c.want = np.array([want[k] for k in ("total_loss", "iou_loss", "l1_loss", "conf_loss", "cls_loss", "num_fg")])
    c.oracle_matched = out["_matched_gt"]
    return c


def _assert_margins(c):
    """The preconditions every scenario shares — on the input (the float64 restatement), before the kernel runs."""
    for i, r in enumerate(c.ref):
        if r is None:
            assert int((c.oracle_matched[i] >= 0).sum()) == 0
            continue
        assert r["cost_margin"] >= COST_MARGIN, (i, r["cost_margin"])
        assert r["k_margin"] >= K_MARGIN, (i, r["k_margin"])
        assert r["geo_margin"] >= GEO_MARGIN, (i, r["geo_margin"])
        # a cost that carries the 1e5 penalty has an fp32 spacing of 0.0078: a decision between two such costs needs more than
        # the absolute margin, so every deciding gap is also at least 16 fp32 spacings of the larger cost
        assert r["cost_margin_ulp32"] >= 16.0, (i, r["cost_margin_ulp32"])
        # the fp32 oracle that supplies loss and gradient took the same decisions
        assert torch.equal(c.oracle_matched[i], r["matched"]), i


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _check_kernel(backend, c):
    B = c.raw.shape[0]
    ws = ops.TalLossWorkspace(B, c.A, 5 + c.nc, c.hw, c.cfg.strides, backend, max_labels=c.max_labels)
    raw = c.raw.to(backend)

    def call():
        losses, d_raw, fg = ops.tal_loss(raw, c.lab, c.sup, c.nc, c.cfg.gamma, c.cfg.ignore_thr, c.cfg.ignore_value, c.use_l1, ws)
        mg, mi = ops.tal_assignment(ws)
        return losses.cpu().clone(), d_raw.cpu().clone(), fg.cpu().clone(), mg.cpu(), mi.cpu()

    losses, d_raw, fg, mg, mi = call()
    # 1. the matched ground truth of every anchor, exactly
    num_fg, dev = 0, 0.0
    for i, r in enumerate(c.ref):
        want = r["matched"] if r is not None else torch.full((c.A,), -1, dtype=torch.int32)
        bad = (mg[i] != want).nonzero().squeeze(1)
        assert len(bad) == 0, "image %d: %d anchors differ, first %s: kernel %s, float64 %s" % (
            i, len(bad), bad[:8].tolist(), mg[i][bad[:8]].tolist(), want[bad[:8]].tolist())
        assert torch.equal(fg[i].bool(), want >= 0)
        num_fg += int((want >= 0).sum())
        # 2. the matched IoU: 0 on background, within 4 x the fp32 restatement's own error of float64 elsewhere
        assert int((mi[i][want < 0] != 0).sum()) == 0
        if r is not None:
            dev = max(dev, float((mi[i].double() - r["iou"])[want >= 0].abs().max()))
    print("matched IoU: |kernel - float64| %.3e, |fp32 restatement - float64| %.3e (%s)" % (dev, c.e32, backend))
    assert dev <= 4 * c.e32 + 1e-7, (dev, c.e32)
    # 3. loss entries and gradient against the fp32 oracle
    got = losses[:6].numpy()
    rel = np.abs(got - c.want) / np.maximum(np.abs(c.want), 1e-30)              # per entry (an entry that must be 0 has to be 0)
    print("losses: worst relative error of an entry %.2e; gradient %.2e" % (rel.max(), _rel(d_raw, c.grad)))
    assert rel.max() < 2e-5, (got, c.want)
    assert float(losses[6]) == num_fg and float(losses[7]) == c.num_gt
    if not c.use_l1:
        assert float(losses[2]) == 0.0
    assert _rel(d_raw, c.grad) < 2e-4
    # 4. background rows: only the objectness channel carries gradient
    bgrows = d_raw[mg < 0]
    assert float(bgrows[:, :4].abs().max()) == 0.0 and float(bgrows[:, 5:].abs().max()) == 0.0
    # 5. a second call on the same workspace: the same bits (several workgroups write W.mgt of a multiply-claimed anchor)
    again = call()
    for a, b in zip((losses, d_raw, fg, mg, mi), again):
        assert torch.equal(a, b)


def _refs(c):
    return [r for r in c.ref if r is not None]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_simota_overlapping_boxes(backend, seed):
    c = _case(HW_315, (GT_OVERLAP,), 0.1, seed=seed)
    _assert_margins(c)
    assert min(c.ref[0]["k"]) >= 8, c.ref[0]["k"]
    _check_kernel(backend, c)


def test_simota_without_l1(backend):
    """use_l1 = False: the L1 entry is exactly 0 and the gradient is that of total - l1 (autograd then drops exactly the L1 term)."""
    c = _case(HW_315, (GT_OVERLAP,), 0.1, use_l1=False)
    _assert_margins(c)
    assert min(c.ref[0]["k"]) >= 8, c.ref[0]["k"]
    _check_kernel(backend, c)


@pytest.mark.parametrize("nc", [80, 1])
def test_simota_class_counts(backend, nc):
    gts = GT_OVERLAP if nc > 1 else tuple((0,) + g[1:] for g in GT_OVERLAP)
    c = _case(HW_315, (gts,), 0.1, nc=nc)
    _assert_margins(c)
    assert min(c.ref[0]["k"]) >= 8, c.ref[0]["k"]
    _check_kernel(backend, c)


def test_simota_batch_of_three(backend):
    c = _case(HW_315, (GT_OVERLAP, (), GT_OVERLAP[2:]), 0.1)
    _assert_margins(c)
    assert c.ref[1] is None and c.num_gt == 6
    assert min(min(r["k"]) for r in _refs(c)) >= 8
    _check_kernel(backend, c)


def test_simota_near_duplicate_ground_truths(backend):
    """Three boxes on one object: most of their cheapest candidates are claimed two or three times."""
    c = _case(HW_315, (((1, 60.3, 40.7, 50, 40), (1, 62.9, 42.1, 52, 42), (2, 61.1, 41.9, 48, 44)),), 0.1)
    _assert_margins(c)
    assert c.ref[0]["n_conflict"] >= 5 and min(c.ref[0]["k"]) >= 8, (c.ref[0]["n_conflict"], c.ref[0]["k"])
    _check_kernel(backend, c)


def test_simota_fewer_candidates_than_anchors_of_one_wave(backend):
    """32 anchors in all, 28 of them candidates (fewer than a wave of tal_match_kernel has lanes), k = 9: most lanes and three of the
    four waves hand empty lists to the merges."""
    c = _case(HW_32, (((1, 20.3, 14.1, 30, 20),),), 0.05)
    _assert_margins(c)
    r = c.ref[0]
    assert r["C"] < 32 and r["k"] == [9], (r["C"], r["k"])
    _check_kernel(backend, c)


def test_simota_tiny_box_k_is_one_by_the_clamp(backend):
    c = _case(HW_32, (((1, 3.1, 2.9, 2, 2),),), 0.1)
    _assert_margins(c)
    assert c.ref[0]["ksum"][0] < 1.0 and c.ref[0]["k"] == [1]
    _check_kernel(backend, c)


@pytest.mark.parametrize("n_gt", [128, 100])
def test_simota_many_ground_truths(backend, n_gt):
    """max_labels = 128 = the kernel's kMaxGT, all rows filled, and 100 of the 128."""
    c = _case(HW_840, (_random_boxes(128)[:n_gt],), 0.1, max_labels=128)
    _assert_margins(c)
    r = c.ref[0]
    assert r["G"] == n_gt and r["n_conflict"] >= 50 and min(r["k"]) == 1 and max(r["k"]) >= 8, (r["n_conflict"], min(r["k"]), max(r["k"]))
    _check_kernel(backend, c)


def test_simota_thousands_of_candidates(backend):
    """More than 2560 candidates: every thread of tal_match_kernel ranks more than ten."""
    c = _case(HW_5040, (((1, 320.4, 190.3, 560, 330), (2, 300.7, 200.9, 400, 300), (4, 100.2, 80.6, 90, 70)),), 0.05)
    _assert_margins(c)
    assert c.ref[0]["C"] > 2560 and min(c.ref[0]["k"]) >= 8, (c.ref[0]["C"], c.ref[0]["k"])
    _check_kernel(backend, c)


def test_simota_top_ten_in_one_lane(backend):
    """A column of a 256-wide level: all ten largest IoUs and all ten cheapest candidates belong to ONE thread of tal_match_kernel
    (anchor % 256), so that thread's sorted lists must hold all ten and its wave must hand all ten on."""
    c = _case(HW_4032, (((1, 812.3, 48.2, 7, 92),),), 0.02, level0_only=True)
    _assert_margins(c)
    r = c.ref[0]
    assert r["lane_iou"] == [10] and r["lane_cost"] == [10] and r["k"][0] >= 8, (r["lane_iou"], r["lane_cost"], r["k"])
    _check_kernel(backend, c)


def test_simota_top_ten_in_one_wave(backend):
    """A run along one row: the ten cheapest candidates sit in ten different lanes of ONE wave."""
    c = _case(HW_315, (((1, 80.3, 44.2, 150, 7),),), 0.03, level0_only=True)
    _assert_margins(c)
    r = c.ref[0]
    assert r["wave_cost"] == [10] and r["lane_cost"] == [1] and r["k"][0] >= 8, (r["wave_cost"], r["lane_cost"], r["k"])
    _check_kernel(backend, c)

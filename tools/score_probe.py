#!/usr/bin/env python
"""DetectionScorer at the size of a validation pass, beside the host path it replaces.

Synthetic data from a seed: --images images of --classes classes, ~--dets detections and ~--gts ground truths per image (boxes
on a quarter-pixel grid, detections scattered around the ground truths, scores from 1024 float32 values).  Reports
  add_ms_total / add_us_per_image   every image appended in batches of --batch (device tensors, no host read; one synchronise at
                                    the end)
  summarize_ms                      wall time of summarize(): sy_score_accumulate + the evaluation's one host read (best and all
                                    of --rounds calls)
  host_*                            the host path on the FIRST --host-images images of the same data, on this machine's CPU:
                                    building the dict rows as streaming.pair_with_ground_truth builds them (host_rows_ms), then the
                                    float64 numpy restatement of COCOeval that the tests use as their yardstick (host_restatement_ms)
                                    — a loop-form restatement, NOT pycocotools, whose inner loops are C.  host_scaled_to_all_s
                                    scales both linearly to --images.
When the host path ran on every image, `bit_equal` says whether both paths produced the same arrays.  Prints one JSON line.

    python tools/score_probe.py --images 15000 --host-images 1500 --out profiles/r13/score_probe.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=15000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--dets", type=int, default=50)
    ap.add_argument("--gts", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-images", type=int, default=1500)
    ap.add_argument("--emulator", type=int, default=0, help="1: rehearse on the SIMT emulator build (no timing means anything)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from streamyolo_amd import _lib
    from streamyolo_amd import streaming as S
    from streamyolo_amd.scoring import DetectionScorer
    if args.emulator:
        _lib.use_library(os.path.join(ROOT, "tests", "emu", "_build", "libstreamyolo_emu.so"))
        dev, sync, name = torch.device("cpu"), (lambda: None), "SIMT emulator (rehearsal)"
    else:
        _lib.use_library(_lib.DEFAULT_PATH)
        dev, sync, name = torch.device("cuda:0"), torch.cuda.synchronize, torch.cuda.get_device_name(0)
    N, K, D, G = args.images, args.classes, 2 * args.dets, 2 * args.gts
    rs = np.random.RandomState(0)
    n_gt = rs.randint(0, G + 1, N).astype(np.int32)
    n_det = rs.randint(0, D + 1, N).astype(np.int32)
    gt = np.zeros((N, G, 7))
    gt[:, :, 0:2] = rs.randint(0, 4 * 1500, (N, G, 2)) * 0.25
    gt[:, :, 2:4] = rs.randint(4 * 8, 4 * 300, (N, G, 2)) * 0.25
    gt[:, :, 4] = rs.randint(0, K, (N, G))
    gt[:, :, 5] = rs.rand(N, G) < 0.05
    gt[:, :, 6] = gt[:, :, 2] * gt[:, :, 3]
    src = rs.randint(0, G, (N, D))                               # every detection sits near one of the image's ground-truth slots
    near = np.take_along_axis(gt, src[:, :, None].repeat(7, 2), axis=1)
    det = np.zeros((N, D, 7), dtype=np.float32)
    det[:, :, 0:2] = near[:, :, 0:2] + rs.randint(-24, 25, (N, D, 2)) * 0.25
    det[:, :, 2:4] = det[:, :, 0:2] + np.maximum(near[:, :, 2:4] + rs.randint(-24, 25, (N, D, 2)) * 0.25, 1.0)
    det[:, :, 4] = (rs.randint(1, 1025, (N, D)) / 1024.0)
    det[:, :, 5] = 1.0
    det[:, :, 6] = np.where(rs.rand(N, D) < 0.85, near[:, :, 4], rs.randint(0, K, (N, D)))
    order = np.argsort(-det[:, :, 4], axis=1, kind="mergesort")  # a detector delivers descending scores
    det = np.take_along_axis(det, order[:, :, None].repeat(7, 2), axis=1)

    res = {"tool": "score_probe", "images": N, "classes": K, "mean_dets": float(n_det.mean()), "mean_gts": float(n_gt.mean()),
           "batch": args.batch, "device": name, "cpu_threads": torch.get_num_threads()}
    d_det, d_cnt = torch.from_numpy(det).to(dev), torch.from_numpy(n_det).to(dev)
    d_gt, d_gcnt = torch.from_numpy(gt).to(dev), torch.from_numpy(n_gt).to(dev)
    scorer = DetectionScorer(K, capacity=int(n_det.sum()), max_gt=G, device=dev)

    def add_all():
        scorer.reset()
        for n0 in range(0, N, args.batch):
            n1 = min(n0 + args.batch, N)
            scorer.add(d_det[n0:n1], d_cnt[n0:n1], d_gt[n0:n1], d_gcnt[n0:n1])
    add_all()                                                    # (warm-up: code objects loaded)
    scorer.summarize()
    adds, walls = [], []
    for _ in range(args.rounds):
        sync()
        t0 = time.perf_counter()
        add_all()
        sync()
        adds.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        out = scorer.summarize()
        walls.append((time.perf_counter() - t0) * 1e3)
    res.update({"add_ms_total": min(adds), "add_ms_rounds": adds, "add_us_per_image": 1e3 * min(adds) / N,
                "summarize_ms": min(walls), "summarize_ms_rounds": walls, "records_per_class": scorer.counters()[0].tolist(),
                "AP": out["AP"], "AR100": out["AR100"]})

    H = min(args.host_images, N)
    if H > 0:
        from test_score_kernel import restate_rows
        t0 = time.perf_counter()
        parsed = [(det[n, :n_det[n], :4], det[n, :n_det[n], 4] * det[n, :n_det[n], 5], det[n, :n_det[n], 6].astype(np.int32), None)
                  for n in range(H)]
        results = {"timestamps": [n / 30.0 for n in range(H)], "input_fidx": list(range(H)), "results_parsed": parsed}
        rows, _ = S.pair_with_ground_truth(results, list(range(H)), fps=30.0)
        t_rows = time.perf_counter() - t0
        t0 = time.perf_counter()
        per_image = [([], [{"bbox": [float(v) for v in g[:4]], "label": int(g[4]), "iscrowd": int(g[5]), "area": float(g[6])}
                           for g in gt[n, :n_gt[n]]]) for n in range(H)]
        for r in rows:
            per_image[r["image_id"]][0].append({"bbox": [float(v) for v in r["bbox"]], "score": r["score"], "label": int(r["category_id"])})
        want = restate_rows(per_image, K)
        t_host = time.perf_counter() - t0
        res.update({"host_images": H, "host_rows": len(rows), "host_rows_ms": 1e3 * t_rows, "host_restatement_ms": 1e3 * t_host,
                    "host_scaled_to_all_s": (t_rows + t_host) * N / H, "host_is": "float64 numpy restatement in loop form, not pycocotools"})
        if H == N:
            res["bit_equal"] = bool(np.array_equal(want["precision"], out["precision"]) and np.array_equal(want["recall"], out["recall"]))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Batched streaming ticks of MultiStreamDetector against the same number of single-camera frames.

StreamYOLO-l, fp16, 1200x1920 uint8 camera frames already on the device (the pattern of `bench.py --workload stream
--u8-input 1`: 2x decimation + Focus packing, network, decode, NMS with a realistic candidate count; no host read inside the
timed region).  Reports ms per tick and frames/s for batch in {1, 2, 4, 8, 16} with every row active, for n in {1, 4, 8} active
rows at batch 8, and — the yardstick — for StreamingDetector's taped frame issued n times back to back.  Warm-up ticks (they
build, tune and record the plans), then `--ticks` timed ticks between two events, `--rounds` times alternating with the
yardstick; the best round counts.  Prints one JSON line (and writes it to --out).

    python tools/multistream_probe.py --out profiles/r08/multistream_probe.json
    python tools/multistream_probe.py --trace 8      # only warm up batch 8 and run 20 ticks (for rocprofv3 --kernel-trace --stats)
    python tools/multistream_probe.py --mixed 1 --batches 1,4,8 --out profiles/r08/multistream_probe_mixed.json

--mixed 1: the detector runs in mixed mode (max_frame_hw) and the rows' cameras cycle through three sizes — the frame size
(2x decimation), the network input size (copy) and 3/4 x 5/6 of the frame (`preproc`'s letterbox, r = 0.6 for 1200x1920) — all
packed by the ONE sy_frames_u8_pack_rows launch of the tape.  Every row of the result also carries the uniform detector's tick
at the same batch, measured in the same process, alternating (`uniform_ms_per_tick`, `mixed_over_uniform`).

--pixel-format nv12 (or rgb): the detector is built for cameras that deliver that format (the same pictures converted on the
host before the timed region; NV12 frames are half the bytes) and the pack launch converts.  Every row also carries the BGR
detector's tick at the same batch, measured in the same process, alternating: `bgr_ms_per_tick`, `nv12_over_bgr` (best round
over best round) and the per-round times of both (`ms_rounds`, `bgr_ms_rounds`: the spread the ratio has to be read against).

    python tools/multistream_probe.py --pixel-format nv12 --batches 1,8 --out profiles/r09/multistream_probe_nv12.json

--surfaces 1: the mixed-mode tick (max_frame_hw; every stream a --pixel-format camera of the frame size) timed two ways in one
process, alternating: `staged` — the frames are plain tensors, copied into the detector's arena every tick — and `surfaces` —
MultiStreamDetector(surfaces=True) with every row a data.Surface read where it lies (no copy).  Rows carry
`staged_ms_per_tick`, `surfaces_ms_per_tick`, the per-round times of both and `surfaces_over_staged`.  --staged-only 1 leaves
the second detector out (the same measurement on a tree that has no surfaces).

    python tools/multistream_probe.py --surfaces 1 --pixel-format nv12 --batches 1,8

--track 1: the tick of MultiStreamDetector(track=True) — the tracker launch (sy_track_update) behind the NMS on the same tape —
beside the untracked tick at the same batch (two detectors over two copies of the model), in one process, alternating: `untracked_ms_per_tick`, `tracked_ms_per_tick`, the
per-round times of both, `tracked_minus_untracked_ms` (best round minus best round; to be read against the spread) and the mean
detections per row the tracker saw.  Every row also carries `track_kernel_us`: sy_track_update alone at this batch on synthetic
rows of 30 and of 256 persisting detections (every detection matches its track: the whole serial association loop runs),
--ticks launches replayed back to back from a launch tape between two events (the launch gaps included).  --untracked-only 1 leaves the tracked detector out, and
--tree PATH imports the package of another checkout of the repository (its own library): together the same measurement on
a tree that has no tracker.

    python tools/multistream_probe.py --track 1 --batches 1,8
    python tools/multistream_probe.py --track 1 --untracked-only 1 --tree _base --batches 1,8

--score 1: the tick of one detector with and without DetectionScorer.add behind it (sy_score_match on the tick's device tensors,
twelve synthetic ground truths per row; `add` is not on the tape), alternating: `tick_ms_per_tick`, `tick_add_ms_per_tick`, the
per-round times and `add_ms_per_tick` (best minus best, to be read against the spread); then `summarize_ms`: the wall time of
one summarize() over everything the timed ticks added (sy_score_accumulate + the evaluation's host read).

    python tools/multistream_probe.py --score 1 --batches 1,8

--policy 1: the tick of MultiStreamDetector(policy=True) — sy_postprocess_rows on the tape, one sy_det_policy per row — beside
today's tick (sy_postprocess) at the same batch, two detectors over two copies of the model, in one process, alternating.  The
rows detector is timed with default rows, with max_det=100 and with max_candidates=1024 at the detector's conf_thre = 0.01 (the
realistic candidate count: ~1 % of the anchors), and the same three with conf_thre = 0 in the rows (EVERY anchor a candidate:
the serial sweep at its full 185 chunks, where the caps shorten it); the policies are switched with set_policy between the timed
runs, on the one tape.  Today's tick is timed twice per round (`today`, `today_again`): `today_spread_ms` over all of those
rounds is what `rows_default_minus_today_ms` has to be read against.  Two controls over model copies of their own: `today_twin`, a
second detector of today's kind, and `today_with_table`, a policy=True detector whose post step is swapped back to sy_postprocess
before its tape is recorded (the table and its bookkeeping, but today's launches).  `nms_us`: the three NMS launches alone at the
plan's anchor count on synthetic predictions (every anchor / 1 % of the anchors a candidate), both entry points and capped rows.

    python tools/multistream_probe.py --policy 1 --batches 1,8

--overlay 1: drawing the tick's boxes into the camera frames on the device (MultiStreamDetector.draw, sy_overlay_draw; not on the
tape), three things in one process, alternating.  `tick_ms_per_tick` / `tick_draw_ms_per_tick`: the tick alone and with one draw()
of every row into a BGR frame behind it (style: min_score 0.01, at most 128 boxes; `boxes_drawn_per_row`), per-round times and
`draw_ms_per_tick` (best minus best, to be read against the spread).  `overlay_kernel_us`: the launch alone on B 1200x1920 BGR
and NV12 surfaces with 30 and with 256 boxes per row (a grid of 150 x 100 px / 56 x 36 px boxes with labels), --ticks launches
replayed back to back from a launch tape between two events (the launch gaps included).  `clone_us`: the yardstick — a plain device
copy of the same B surfaces (Surface.clone()), which is what drawing on the host would at least have to move once more.

    python tools/multistream_probe.py --overlay 1 --batches 1,8

--crops 1: cropping the tick's boxes out of the camera frames on the device (MultiStreamDetector.crops, sy_crop_gather; not on the
tape), three things in one process, alternating.  `tick_ms_per_tick` / `tick_crops_ms_per_tick`: the tick alone and with one
crops() of every row's BGR frame behind it (64 x 64 fp16 crops, min_score 0.01, at most 32 per row; `boxes_cropped_per_row`),
per-round times and `crops_ms_per_tick` (best minus best, to be read against the spread).  `crop_kernel_us`: the call alone (its
two launches) on B 1200x1920 BGR and NV12 surfaces for 32 and 256 crops in all (spread evenly over the B rows; synthetic lists
of 40..112 x 30..110 px boxes on a grid) of 64 x 64 and of 224 x 224 fp16, keep-aspect with 10 % padding, --ticks calls replayed
back to back from a launch tape between two events (the launch gaps included).  `copy_us`: the yardstick — a plain device copy
of a tensor the size of the crops written, the bytes any method must store — timed the same way (sy_view_copy replayed from a
launch tape); `copy_eager_us`: torch's copy_ of the same tensor issued eagerly.

    python tools/multistream_probe.py --crops 1 --batches 1,8

--redact 1: pixelating the tick's boxes in the camera frames on the device (MultiStreamDetector.redact, sy_redact; not on the
tape), three things in one process, alternating.  `tick_ms_per_tick` / `tick_redact_ms_per_tick`: the tick alone and with one
redact() of every row's BGR frame behind it (pixelate, cell 16, pad 0.1, min_score 0.01; `boxes_redacted_per_row`), per-round
times and `redact_ms_per_tick` (best minus best, to be read against the spread).  `redact_kernel_us`: the launch alone on B
1200x1920 BGR and NV12 surfaces, PIXELATE cell 16 and FILL, with 30 and with 256 boxes per row (the grids of --overlay 1), --ticks
launches replayed back to back from a launch tape between two events (the launch gaps included).  `clone_us`: the yardstick — a
plain device copy of the same B surfaces (Surface.clone()), timed in the same run.

    python tools/multistream_probe.py --redact 1 --batches 1,8
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:                                   # (before anything of the package is imported)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="l")
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--active", default="1,4,8", help="active rows measured at batch 8")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0, help="batch: warm up, run 20 ticks of that batch and exit (profiler runs)")
    ap.add_argument("--baseline-only", type=int, default=0, help="1: only the single-camera yardstick (also runs on older trees)")
    ap.add_argument("--mixed", type=int, default=0, help="1: mixed-mode detector, row cameras cycling through three sizes")
    ap.add_argument("--pixel-format", default="bgr", choices=["bgr", "rgb", "nv12"],
                    help="the format the cameras deliver; not bgr: timed beside the BGR tick of the same batch")
    ap.add_argument("--surfaces", type=int, default=0,
                    help="1: the mixed-mode tick of --pixel-format cameras, staged beside every row a Surface read in place")
    ap.add_argument("--staged-only", type=int, default=0, help="with --surfaces 1: only the staged tick (runs on older trees)")
    ap.add_argument("--track", type=int, default=0, help="1: the tracked tick beside the untracked tick of the same batch")
    ap.add_argument("--untracked-only", type=int, default=0, help="with --track 1: only the untracked tick (runs on older trees)")
    ap.add_argument("--score", type=int, default=0, help="1: the tick with and without DetectionScorer.add, and one summarize()")
    ap.add_argument("--policy", type=int, default=0, help="1: the tick through sy_postprocess_rows (default and capped rows) beside today's")
    ap.add_argument("--overlay", type=int, default=0, help="1: the tick with and without draw(), the overlay launch alone, Surface.clone()")
    ap.add_argument("--crops", type=int, default=0, help="1: the tick with and without crops(), the crop call alone, a copy of the crops' bytes")
    ap.add_argument("--redact", type=int, default=0, help="1: the tick with and without redact(), the redact launch alone, Surface.clone()")
    ap.add_argument("--tree", default=None, help="root of another checkout of the repository to import the package from")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd import _lib
    from streamyolo_amd.streaming import StreamingDetector
    from streamyolo_amd.utils.synth import synth_state_dict, synth_frames, bgr_to_nv12
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda:0")
    hw = (args.height, args.width)
    cfg = O.OracleConfig.named(args.model)
    model = sy.build_model(args.model)
    model.load_state_dict(synth_state_dict(O.param_shapes(cfg), seed=0), strict=True)
    batches = [int(b) for b in args.batches.split(",") if b]
    nmax = max(batches + [8])
    # distinct pictures per row, every pixel repeated 2x2 so that the decimation returns the synthetic frame
    x = synth_frames(nmax, hw[0] // 2, hw[1] // 2, seed=2)[:, 0:3]
    raw = x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    raw = raw.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous().to(dev)
    frames = [raw[i] for i in range(nmax)]

    single = StreamingDetector(model, hw, dtype=args.dtype, device=dev)
    # a trained StreamYOLO passes ~1 % of its anchors through conf 0.01, random weights all of them: shift the objectness biases
    # by one constant found by bisection on the first frame's own scores (bench.py --candidates realistic)
    with torch.no_grad():
        single._slot[0].copy_(frames[0])
        dec = single.plan.run_stream(single._in, first=True).clone()
        obj, cls = dec[0, :, 4].double().clamp(1e-12, 1 - 1e-12), dec[0, :, 5:].double().max(dim=1).values
        logit = torch.log(obj / (1 - obj))
        lo, hi = -40.0, 0.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            frac = float(((torch.sigmoid(logit + mid) * cls) >= 0.01).double().mean())
            lo, hi = (mid, hi) if frac < 0.01 else (lo, mid)
        for conv in model.head.obj_preds:
            conv.bias.add_(0.5 * (lo + hi))
    single.warm_up(args.warmup)

    def single_tick(n):
        with torch.no_grad():
            for i in range(n):
                single._slot[0].copy_(frames[i], non_blocking=True)
                single.plan.run_stream_taped(single._in, post=single._post, check_params=False)

    def timed(fn, ticks):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(ticks):
            fn()
        host = (time.perf_counter() - t0) * 1e3 / ticks
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / ticks, host

    res = {"tool": "multistream_probe", "model": args.model, "dtype": args.dtype, "frame": list(hw), "ticks": args.ticks,
           "warmup": args.warmup, "rounds": args.rounds, "kernel_source_key": _lib.kernel_source_key(),
           "device": torch.cuda.get_device_name(0), "rows": []}
    # --mixed: camera i has size sizes[i % 3]; its pictures are the frame itself, every second pixel of it, its top-left part
    sizes = [hw, (hw[0] // 2, hw[1] // 2), (hw[0] * 3 // 4, hw[1] * 5 // 6)]
    if args.mixed:
        res["mixed_sizes"] = [list(v) for v in sizes]
        mixed_frames = [(raw[i], raw[i][::2, ::2].contiguous(), raw[i][:sizes[2][0], :sizes[2][1]].contiguous())[i % 3]
                        for i in range(nmax)]

    def emit():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    fmt = args.pixel_format
    if fmt != "bgr":
        if args.mixed:
            ap.error("--pixel-format and --mixed are separate measurements")
        res["pixel_format"] = fmt
        fmt_frames = [bgr_to_nv12(f) if fmt == "nv12" else f.flip(-1).contiguous() for f in frames]
    alt = bool(args.mixed) or fmt != "bgr"                       # a second detector of the batch is timed beside the uniform BGR one

    if args.surfaces:
        if args.mixed:
            ap.error("--surfaces and --mixed are separate measurements")
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"pixel_format": fmt, "surfaces": True})
        cam = frames if fmt == "bgr" else fmt_frames
        for B in batches:
            kw = dict(max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            staged = MultiStreamDetector(model, hw, max_frame_hw=hw, **kw)
            staged.warm_up(args.warmup)
            s_sids = [staged.open(pixel_format=fmt) for _ in range(B)]
            ticks = {"staged": lambda: staged.detect_device(cam[:B], s_sids)}
            if not args.staged_only:
                from streamyolo_amd.data import Surface
                inplace = MultiStreamDetector(model, hw, surfaces=True, **kw)
                inplace.warm_up(args.warmup)
                i_sids = [inplace.open(pixel_format=fmt) for _ in range(B)]
                surfs = [Surface((f[:hw[0]], f[hw[0]:]), fmt) if fmt == "nv12" else Surface(f, fmt) for f in cam[:B]]
                ticks["surfaces"] = lambda: inplace.detect_device(surfs, i_sids)
            rounds = {k: [] for k in ticks}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                for k, fn in ticks.items():
                    fn()                                         # (untimed: first rows done; a tape re-recorded after a switch)
                    rounds[k].append(timed(fn, args.ticks)[0])
            row = {"batch": B, "active": B, "pixel_format": fmt}
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v, k + "_spread_over_rounds": (max(v) - min(v)) / min(v)})
            if "surfaces" in rounds:
                row["surfaces_over_staged"] = min(rounds["surfaces"]) / min(rounds["staged"])
            res["rows"].append(row)
            emit()
            del ticks, staged
            if not args.staged_only:
                del inplace, surfs
        print(emit())
        return

    if args.track:
        if args.mixed or args.surfaces or fmt != "bgr":
            ap.error("--track is a separate measurement")
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"track": True, "tree": ROOT})
        for B in batches:
            kw = dict(max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            plain = MultiStreamDetector(model, hw, **kw)
            plain.warm_up(args.warmup)
            p_sids = [plain.open() for _ in range(B)]
            ticks = {"untracked": lambda: plain.detect_device(frames[:B], p_sids)}
            row = {"batch": B, "active": B}
            if not args.untracked_only:
                twin = sy.build_model(args.model)                # (its own plan: no tape is re-recorded when the ticks alternate)
                twin.load_state_dict(model.state_dict(), strict=True)
                tracked = MultiStreamDetector(twin, hw, track=True, **kw)
                tracked.warm_up(args.warmup)
                t_sids = [tracked.open() for _ in range(B)]
                ticks["tracked"] = lambda: tracked.detect_device(frames[:B], t_sids)
            rounds = {k: [] for k in ticks}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                for k, fn in ticks.items():
                    fn()                                         # (untimed: first rows done; a tape re-recorded after a switch)
                    rounds[k].append(timed(fn, args.ticks)[0])
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v, k + "_spread_ms": max(v) - min(v)})
            if "tracked" in rounds:
                from streamyolo_amd import ops
                row["tracked_minus_untracked_ms"] = min(rounds["tracked"]) - min(rounds["untracked"])
                r = tracked.detect_device(frames[:B], t_sids)    # (one more tick: what the tracker had to do)
                row["detections_per_row"] = r[1][:B].cpu().tolist()
                row["tracks_out_per_row"] = r[-1][:B].cpu().tolist()
                row["tracks_matched_per_row"] = tracked.tracks.state.hdr[:, 1].cpu().tolist()
                # the kernel alone: rows of k boxes on a grid that come back every tick
                ts, T, us = tracked.tracks, tracked.tracks.T, {}
                for k in (30, T):
                    g = torch.arange(k, device=dev, dtype=torch.float32)
                    box = torch.stack([(g % 32) * 40, (g // 32) * 40, (g % 32) * 40 + 32, (g // 32) * 40 + 32,
                                       1.0 - g / (2 * T), torch.ones_like(g), g % 8], dim=1)
                    det_k = torch.zeros((B, T, 7), device=dev)
                    det_k[:, :k] = box
                    cnt_k = torch.full((B,), k, dtype=torch.int32, device=dev)
                    ts.set_rows([(1, 0.0, float(hw[1]), float(hw[0]), 0.5)] * B)
                    ts.upload()
                    slot = torch.arange(B, dtype=torch.int32, device=dev)
                    first = torch.zeros(B, dtype=torch.uint8, device=dev)

                    def kernel():
                        ops.track_update(det_k, cnt_k, slot, first, ts.ticks, ts.state, tracked._track_prm, ts.out, ts.out_id, ts.out_cnt)
                    ops.track_update(det_k, cnt_k, slot, first.fill_(1), ts.ticks, ts.state, tracked._track_prm, ts.out, ts.out_id, ts.out_cnt)
                    first.zero_()
                    kernel()
                    tape = _lib.NativeTape()                     # (the launches re-issued from C: the Python wrapper costs more than
                    with tape:                                   #  the kernel takes at 30 detections)
                        for _ in range(args.ticks):
                            kernel()
                    stream = ops.stream_of(det_k)
                    tape.replay(stream, None)
                    us[str(k)] = 1e3 * min(timed(lambda: tape.replay(stream, None), 3)[0] for _ in range(args.rounds)) / args.ticks
                    assert int(ts.state.hdr[:B, 1].min()) == k   # every detection matched its track
                row["track_kernel_us"] = us
                del tracked, twin
            res["rows"].append(row)
            emit()
            del ticks, plain
        print(emit())
        return

    if args.overlay:
        if args.mixed or args.surfaces or args.track or args.score or args.policy or fmt != "bgr":
            ap.error("--overlay is a separate measurement")
        from streamyolo_amd import ops
        from streamyolo_amd.data import Surface
        from streamyolo_amd.overlay import OverlayRows, OverlayStyle
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"overlay": True})
        style = OverlayStyle(min_score=0.01, max_boxes=128)
        for B in batches:
            det = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            det.warm_up(args.warmup)
            sids = [det.open() for _ in range(B)]
            canvases = [f.clone() for f in frames[:B]]           # drawn on again and again: the cost does not depend on what is there

            def tick_draw():
                det.detect_device(frames[:B], sids)
                det.draw(canvases, sids, style)
            ticks = {"tick": lambda: det.detect_device(frames[:B], sids), "tick_draw": tick_draw}
            rounds = {k: [] for k in ticks}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                for k, fn in ticks.items():
                    fn()
                    rounds[k].append(timed(fn, args.ticks)[0])
            row = {"batch": B, "active": B}
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v, k + "_spread_ms": max(v) - min(v)})
            row["draw_ms_per_tick"] = min(rounds["tick_draw"]) - min(rounds["tick"])
            r = det.detect_device(frames[:B], sids)
            score = (r[0][:B, :128, 4] * r[0][:B, :128, 5] >= 0.01) & (torch.arange(128, device=dev)[None] < r[1][:B, None])
            row["boxes_drawn_per_row"] = score.sum(dim=1).cpu().tolist()
            # the launch alone, and the copy it stands against
            nv12 = [bgr_to_nv12(f) for f in frames[:B]]
            surfs = {"bgr": [Surface(f.clone(), "bgr") for f in frames[:B]],
                     "nv12": [Surface((f[:hw[0]], f[hw[0]:]), "nv12") for f in nv12]}
            pal, text, glyphs = style.tables(dev)
            us, clone = {}, {}
            for name, ss in surfs.items():
                table = OverlayRows(B, dev)
                for b, sf in enumerate(ss):
                    table.set_row(b, sf, 1.0, style)
                table._rows["max_boxes"] = 0                     # (the launch's cap: 256)
                table.upload()
                for k, (gw, bw, bh) in ((30, (6, 150, 100)), (256, (32, 56, 36))):
                    g = torch.arange(256, device=dev, dtype=torch.float32)
                    x1, y1 = (g % gw) * (hw[1] // gw) + 8, (g // gw) * (hw[0] // -(-256 // gw) if k == 256 else hw[0] // 5) + 40
                    box = torch.stack([x1, y1, x1 + bw, y1 + bh, 1.0 - g / 512, g % 8], dim=1)
                    lists = box[None].repeat(B, 1, 1).contiguous()
                    ids_k = torch.arange(256, dtype=torch.int32, device=dev)[None].repeat(B, 1).contiguous()
                    cnt_k = torch.full((B,), k, dtype=torch.int32, device=dev)

                    def kernel():
                        ops.overlay_draw(table.table, B, hw, lists, 1, ids_k, cnt_k, pal, text, glyphs)
                    kernel()
                    tape = _lib.NativeTape()
                    with tape:
                        for _ in range(args.ticks):
                            kernel()
                    stream = ops.stream_of(lists)
                    tape.replay(stream, None)
                    us["%s_%d" % (name, k)] = 1e3 * min(timed(lambda: tape.replay(stream, None), 3)[0] for _ in range(args.rounds)) / args.ticks
                [sf.clone() for sf in ss]
                clone[name] = 1e3 * min(timed(lambda: [sf.clone() for sf in ss], args.ticks)[0] for _ in range(args.rounds))
            row["overlay_kernel_us"], row["clone_us"] = us, clone
            res["rows"].append(row)
            emit()
            del ticks, det, surfs
        print(emit())
        return

    if args.redact:
        if args.mixed or args.surfaces or args.track or args.score or args.policy or args.overlay or args.crops or fmt != "bgr":
            ap.error("--redact is a separate measurement")
        from streamyolo_amd import ops
        from streamyolo_amd.data import Surface
        from streamyolo_amd.redact import RedactRows, RedactSpec
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"redact": True})
        tick_spec = RedactSpec(mode="pixelate", cell=16, pad=0.1, min_score=0.01)
        for B in batches:
            det = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            det.warm_up(args.warmup)
            sids = [det.open() for _ in range(B)]
            canvases = [f.clone() for f in frames[:B]]           # redacted again and again: the cost does not depend on what is there

            def tick_redact():
                det.detect_device(frames[:B], sids)
                det.redact(canvases, sids, tick_spec)
            ticks = {"tick": lambda: det.detect_device(frames[:B], sids), "tick_redact": tick_redact}
            rounds = {k: [] for k in ticks}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                for k, fn in ticks.items():
                    fn()
                    rounds[k].append(timed(fn, args.ticks)[0])
            row = {"batch": B, "active": B}
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v, k + "_spread_ms": max(v) - min(v)})
            row["redact_ms_per_tick"] = min(rounds["tick_redact"]) - min(rounds["tick"])
            r = det.detect_device(frames[:B], sids)
            L = r[0].shape[1]
            score = (r[0][:B, :, 4] * r[0][:B, :, 5] >= 0.01) & (torch.arange(L, device=dev)[None] < r[1][:B, None])
            row["boxes_redacted_per_row"] = score.sum(dim=1).cpu().tolist()
            # the launch alone, and the copy it stands against
            nv12 = [bgr_to_nv12(f) for f in frames[:B]]
            surfs = {"bgr": [Surface(f.clone(), "bgr") for f in frames[:B]],
                     "nv12": [Surface((f[:hw[0]], f[hw[0]:]), "nv12") for f in nv12]}
            us, clone = {}, {}
            for name, ss in surfs.items():
                for mode in ("pixelate", "fill"):
                    table = RedactRows(B, dev)
                    for b, sf in enumerate(ss):
                        table.set_row(b, sf, 1.0, RedactSpec(mode=mode, cell=16, pad=0.0, fill=(40, 40, 40)))
                    table.upload()
                    for k, (gw, bw, bh) in ((30, (6, 150, 100)), (256, (32, 56, 36))):       # (the boxes of --overlay 1)
                        g = torch.arange(256, device=dev, dtype=torch.float32)
                        x1, y1 = (g % gw) * (hw[1] // gw) + 8, (g // gw) * (hw[0] // -(-256 // gw) if k == 256 else hw[0] // 5) + 40
                        box = torch.stack([x1, y1, x1 + bw, y1 + bh, 1.0 - g / 512, g % 8], dim=1)
                        lists = box[None].repeat(B, 1, 1).contiguous()
                        cnt_k = torch.full((B,), k, dtype=torch.int32, device=dev)

                        def kernel():
                            ops.redact(table.table, B, hw, lists, 1, cnt_k)
                        kernel()
                        tape = _lib.NativeTape()
                        with tape:
                            for _ in range(args.ticks):
                                kernel()
                        stream = ops.stream_of(lists)
                        tape.replay(stream, None)
                        us["%s_%s_%d" % (name, mode, k)] = \
                            1e3 * min(timed(lambda: tape.replay(stream, None), 3)[0] for _ in range(args.rounds)) / args.ticks
                [sf.clone() for sf in ss]
                clone[name] = 1e3 * min(timed(lambda: [sf.clone() for sf in ss], args.ticks)[0] for _ in range(args.rounds))
            row["redact_kernel_us"], row["clone_us"] = us, clone
            res["rows"].append(row)
            emit()
            del ticks, det, surfs
        print(emit())
        return

    if args.crops:
        if args.mixed or args.surfaces or args.track or args.score or args.policy or args.overlay or fmt != "bgr":
            ap.error("--crops is a separate measurement")
        from streamyolo_amd import ops
        from streamyolo_amd.crops import CropRows, Crops, CropSpec
        from streamyolo_amd.data import Surface
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"crops": True})
        tick_spec = CropSpec(size=(64, 64), pad=0.1, min_score=0.01, max_per_stream=32)
        for B in batches:
            det = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            det.warm_up(args.warmup)
            sids = [det.open() for _ in range(B)]

            def tick_crops():
                det.detect_device(frames[:B], sids)
                det.crops(frames[:B], sids, tick_spec)
            ticks = {"tick": lambda: det.detect_device(frames[:B], sids), "tick_crops": tick_crops}
            rounds = {k: [] for k in ticks}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                for k, fn in ticks.items():
                    fn()
                    rounds[k].append(timed(fn, args.ticks)[0])
            row = {"batch": B, "active": B}
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v, k + "_spread_ms": max(v) - min(v)})
            row["crops_ms_per_tick"] = min(rounds["tick_crops"]) - min(rounds["tick"])
            det.detect_device(frames[:B], sids)
            got = det.crops(frames[:B], sids, tick_spec)
            row["boxes_cropped_per_row"] = torch.bincount(got.index[:int(got.count[0]), 0], minlength=B).cpu().tolist()
            # the call alone, and the copy it stands against
            nv12 = [bgr_to_nv12(f) for f in frames[:B]]
            surfs = {"bgr": [Surface(f, "bgr") for f in frames[:B]],
                     "nv12": [Surface((f[:hw[0]], f[hw[0]:]), "nv12") for f in nv12]}
            us, copy, copy_eager, rounds_us = {}, {}, {}, {}
            for side in (64, 224):
                for total in (32, 256):
                    per = total // B                             # boxes per row: a grid over the frame, sizes cycling
                    spec = CropSpec(size=(side, side), pad=0.1, capacity=total)
                    g = torch.arange(per, device=dev, dtype=torch.float32)
                    gw = max(int(per ** 0.5), 1)
                    x1, y1 = (g % gw) * ((hw[1] - 160) // gw) + 8, (g // gw) * ((hw[0] - 160) // -(-per // gw)) + 8
                    box = torch.stack([x1, y1, x1 + 40 + (g % 7) * 12, y1 + 30 + (g % 5) * 20, 1.0 - g / 512, g % 8], dim=1)
                    lists = box[None].repeat(B, 1, 1).contiguous()
                    ids_k = torch.arange(per, dtype=torch.int32, device=dev)[None].repeat(B, 1).contiguous()
                    cnt_k = torch.full((B,), per, dtype=torch.int32, device=dev)
                    out = Crops.empty(spec, total, dev)
                    twin = torch.empty_like(out.images)
                    key = "%dx%d_%d" % (side, side, total)
                    for name, ss in surfs.items():
                        table = CropRows(B, dev)
                        for b, sf in enumerate(ss):
                            table.set_row(b, sf, 1.0, spec)
                        table.upload()

                        def kernel():
                            ops.crop_gather(table.table, B, lists, 1, ids_k, cnt_k, out.images, out.index, out.rect, out.count, flags=spec.flags)
                        kernel()
                        assert out.count.tolist() == [total, total]
                        tape = _lib.NativeTape()
                        with tape:
                            for _ in range(args.ticks):
                                kernel()
                        stream = ops.stream_of(lists)
                        tape.replay(stream, None)
                        v = [1e3 * timed(lambda: tape.replay(stream, None), 3)[0] / args.ticks for _ in range(args.rounds)]
                        us["%s_%s" % (name, key)], rounds_us["%s_%s" % (name, key)] = min(v), v
                    # the yardstick, timed the same way: the library's own copy kernel (16 bytes per thread) replayed from a tape;
                    # beside it torch's copy_ issued eagerly, whose small sizes show the enqueue, not the copy
                    def copy_kernel():
                        _lib.check(_lib.lib().sy_view_copy(out.images.data_ptr(), 64, twin.data_ptr(), 64, out.images.numel() // 64, 64,
                                                           _lib.DT_F16, 0, ops.stream_of(twin)), "sy_view_copy")
                    copy_kernel()
                    assert torch.equal(twin, out.images)
                    tape = _lib.NativeTape()
                    with tape:
                        for _ in range(args.ticks):
                            copy_kernel()
                    stream = ops.stream_of(twin)
                    tape.replay(stream, None)
                    copy[key] = 1e3 * min(timed(lambda: tape.replay(stream, None), 3)[0] for _ in range(args.rounds)) / args.ticks
                    copy_eager[key] = 1e3 * min(timed(lambda: twin.copy_(out.images), args.ticks)[0] for _ in range(args.rounds))
            row["crop_kernel_us"], row["crop_kernel_us_rounds"], row["copy_us"], row["copy_eager_us"] = us, rounds_us, copy, copy_eager
            row["ratio_to_copy"] = {k: v / copy[k.split("_", 1)[1]] for k, v in us.items()}
            res["rows"].append(row)
            emit()
            del ticks, det, surfs
        print(emit())
        return

    if args.score:
        if args.mixed or args.surfaces or args.track or fmt != "bgr":
            ap.error("--score is a separate measurement")
        from streamyolo_amd.scoring import DetectionScorer
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"score": True})
        for B in batches:
            det = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            det.warm_up(args.warmup)
            sids = [det.open() for _ in range(B)]
            n_img = B * (args.ticks + 1) * args.rounds + B
            scorer = DetectionScorer(8, capacity=min(100 * n_img, 1 << 20), max_gt=16, device=dev)
            # ground truth: twelve fixed boxes per row in camera coordinates, classes cycling
            g = torch.arange(12, dtype=torch.float64)
            gt = torch.stack([100.0 + 140.0 * g, 80.0 + 60.0 * g, 60.0 + 10.0 * g, 50.0 + 8.0 * g, g % 8, torch.zeros(12).double(),
                              (60.0 + 10.0 * g) * (50.0 + 8.0 * g)], dim=1)
            gt = torch.cat([gt, torch.zeros((4, 7), dtype=torch.float64)]).repeat(B, 1, 1).contiguous().to(dev)
            gcnt = torch.full((B,), 12, dtype=torch.int32, device=dev)
            divisor = torch.full((B,), det._geom[sids[0]][2], dtype=torch.float32, device=dev)

            def tick():
                det.detect_device(frames[:B], sids)

            def tick_add():
                d, c, n = det.detect_device(frames[:B], sids)
                scorer.add(d, c, gt, gcnt, divisor=divisor, rows=n)
            ticks = {"tick": tick, "tick_add": tick_add}
            rounds = {k: [] for k in ticks}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                for k, fn in ticks.items():
                    fn()
                    rounds[k].append(timed(fn, args.ticks)[0])
            row = {"batch": B, "active": B}
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v, k + "_spread_ms": max(v) - min(v)})
            row["add_ms_per_tick"] = min(rounds["tick_add"]) - min(rounds["tick"])
            row["detections_per_row"] = det.detect_device(frames[:B], sids)[1][:B].cpu().tolist()
            walls = []
            for _ in range(args.rounds):                         # summarize() twice and more: the first call allocates its workspace
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = scorer.summarize()
                walls.append((time.perf_counter() - t0) * 1e3)
            row.update({"summarize_ms": min(walls), "summarize_ms_rounds": walls, "images_scored": scorer.images,
                        "records_per_class": scorer.counters()[0].tolist(), "AP": out["AP"], "AR100": out["AR100"]})
            res["rows"].append(row)
            emit()
            del det, scorer
        print(emit())
        return

    if args.policy:
        if args.mixed or args.surfaces or args.track or args.score or fmt != "bgr":
            ap.error("--policy is a separate measurement")
        from streamyolo_amd import DetectionPolicy, ops
        from streamyolo_amd.streaming import MultiStreamDetector
        res.update({"policy": True})
        variants = {"rows_default": None, "rows_max_det100": DetectionPolicy(max_det=100),
                    "rows_max_cand1024": DetectionPolicy(max_candidates=1024),
                    "rows_conf0": DetectionPolicy(conf_thre=0.0), "rows_conf0_max_det100": DetectionPolicy(conf_thre=0.0, max_det=100),
                    "rows_conf0_max_cand1024": DetectionPolicy(conf_thre=0.0, max_candidates=1024)}
        for B in batches:
            kw = dict(max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
            plain = MultiStreamDetector(model, hw, **kw)
            plain.warm_up(args.warmup)
            p_sids = [plain.open() for _ in range(B)]
            twin = sy.build_model(args.model)                    # (its own plan: no tape is re-recorded when the ticks alternate)
            twin.load_state_dict(model.state_dict(), strict=True)
            rows = MultiStreamDetector(twin, hw, policy=True, **kw)
            rows.warm_up(args.warmup)
            r_sids = [rows.open() for _ in range(B)]
            twin2 = sy.build_model(args.model)                   # the control: today's detector over a model copy of its own, as
            twin2.load_state_dict(model.state_dict(), strict=True)   # the rows detector is (two plans are two tunings and placements)
            plain2 = MultiStreamDetector(twin2, hw, **kw)
            plain2.warm_up(args.warmup)
            q_sids = [plain2.open() for _ in range(B)]

            def today_twin():
                plain2.detect_device(frames[:B], q_sids)
            # second control: everything policy=True allocates and does per tick (table, pinned mirrors, set_rows), but today's
            # three launches on the tape — the post step is swapped back before anything is recorded
            twin3 = sy.build_model(args.model)
            twin3.load_state_dict(model.state_dict(), strict=True)
            mixed_det = MultiStreamDetector(twin3, hw, policy=True, **kw)
            mixed_det._post = lambda out, d=mixed_det: ops.postprocess(out, d.num_classes, d.conf_thre, d.nms_thresh, d._ws)
            mixed_det.warm_up(args.warmup)
            m_sids = [mixed_det.open() for _ in range(B)]

            def today_with_table():
                mixed_det.detect_device(frames[:B], m_sids)

            def today():
                plain.detect_device(frames[:B], p_sids)

            def rows_tick():
                rows.detect_device(frames[:B], r_sids)
            rounds = {k: [] for k in ["today", "today_again", "today_twin", "today_with_table"] + list(variants)}
            stats = {}
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                today()
                rounds["today"].append(timed(today, args.ticks)[0])
                for k, pol in variants.items():
                    for s in r_sids:
                        rows.set_policy(s, pol)                  # table data: the tape stays
                    rows_tick()
                    rounds[k].append(timed(rows_tick, args.ticks)[0])
                    if k not in stats:
                        stats[k] = rows.detect_device(frames[:B], r_sids)[1][:B].cpu().tolist()
                today_twin()
                rounds["today_twin"].append(timed(today_twin, args.ticks)[0])
                today_with_table()
                rounds["today_with_table"].append(timed(today_with_table, args.ticks)[0])
                today()
                rounds["today_again"].append(timed(today, args.ticks)[0])   # the old path against itself: the spread of this box
            row = {"batch": B, "active": B, "detections_per_row": stats,
                   "detections_per_row_today": plain.detect_device(frames[:B], p_sids)[1][:B].cpu().tolist()}
            for k, v in rounds.items():
                row.update({k + "_ms_per_tick": min(v), k + "_ms_rounds": v})
            both = rounds["today"] + rounds["today_again"]
            row["today_spread_ms"] = max(both) - min(both)
            row["today_vs_today_again_ms"] = abs(min(rounds["today"]) - min(rounds["today_again"]))
            row["rows_default_minus_today_ms"] = min(rounds["rows_default"]) - min(both)
            row["today_twin_minus_today_ms"] = min(rounds["today_twin"]) - min(both)
            row["today_with_table_minus_today_ms"] = min(rounds["today_with_table"]) - min(both)
            row["rows_default_minus_today_twin_ms"] = min(rounds["rows_default"]) - min(rounds["today_twin"])
            # the NMS alone at this batch and the plan's anchor count on synthetic predictions (the network's own output leaves no
            # detection on these frames): `dense` = every anchor a candidate, `one_percent` = 1 % of them over conf 0.01; --ticks
            # calls (three launches each) replayed back to back from a launch tape between two events, launch gaps included
            A, nc = rows.plan.A, 8
            g = torch.Generator().manual_seed(5)
            pred = torch.zeros(B, A, 5 + nc)
            pred[..., 0] = torch.rand(B, A, generator=g) * hw[1] / 2
            pred[..., 1] = torch.rand(B, A, generator=g) * hw[0] / 2
            pred[..., 2:4] = torch.rand(B, A, 2, generator=g) * 200 + 8
            pred[..., 4] = torch.rand(B, A, generator=g) * 0.5 + 0.25 + torch.arange(A)[None] * 2.0 ** -20
            pred[..., 5:] = torch.rand(B, A, nc, generator=g)
            sparse = pred.clone()
            sparse[..., 4] = torch.where(torch.rand(B, A, generator=g) < 0.01, sparse[..., 4], torch.full((), 1e-4))
            ws = ops.PostprocessWorkspace(B, A, dev)
            rec = {"rows_default": DetectionPolicy(), "rows_max_det100": DetectionPolicy(max_det=100),
                   "rows_max_cand1024": DetectionPolicy(max_candidates=1024),
                   "rows_max_cand1024_max_det100": DetectionPolicy(max_candidates=1024, max_det=100),
                   "rows_agnostic": DetectionPolicy(class_agnostic=True)}
            row["nms_us"], row["nms_counts"] = {}, {}
            for name, p in (("dense", pred.to(dev)), ("one_percent", sparse.to(dev))):
                calls = {"today": lambda: ops.postprocess(p, nc, 0.01, 0.65, ws)}
                for k, pol in rec.items():
                    tab = ops.det_policy_table([pol.record(nc, 0.01, 0.65)] * B, dev)
                    calls[k] = lambda tab=tab: ops.postprocess_rows(p, nc, tab, ws)
                tapes = {}
                for k, fn in calls.items():
                    fn()
                    row["nms_counts"][name + "/" + k] = ws.count.cpu().tolist()
                    tapes[k] = _lib.NativeTape()
                    with tapes[k]:
                        for _ in range(args.ticks):
                            fn()
                stream = ops.stream_of(p)
                us = {k: [] for k in calls}
                for _ in range(args.rounds):                     # alternate
                    for k, t in tapes.items():
                        t.replay(stream, None)
                        us[k].append(1e3 * timed(lambda: t.replay(stream, None), 3)[0] / args.ticks)
                row["nms_us"][name] = {k: {"best": min(v), "rounds": v} for k, v in us.items()}
                del tapes
            res["rows"].append(row)
            emit()
            del plain, rows, twin, plain2, twin2, mixed_det, twin3
        print(emit())
        return

    if args.baseline_only:
        single_tick(1)
        for n in sorted(set(batches + [int(v) for v in args.active.split(",") if v])):
            ms = min(timed(lambda: single_tick(n), args.ticks)[0] for _ in range(args.rounds))
            res["rows"].append({"batch": 1, "active": n, "single_ms_per_tick": ms, "single_frames_per_s": 1e3 * n / ms})
        print(emit())
        return

    from streamyolo_amd.streaming import MultiStreamDetector
    single_tick(1)                                               # (steady state: the tape is recorded)
    for B in ([args.trace] if args.trace else batches):
        uni = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev)
        uni.warm_up(args.warmup)
        uni_sids = [uni.open() for _ in range(B)]
        uni.detect_device(frames[:B], uni_sids)                  # first rows done: steady state
        det, sids, tick_frames = uni, uni_sids, frames
        if args.mixed:
            det = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev, max_frame_hw=hw)
            det.warm_up(args.warmup)
            sids = [det.open(frame_hw=sizes[i % 3]) for i in range(B)]
            tick_frames = mixed_frames
            det.detect_device(tick_frames[:B], sids)
        elif fmt != "bgr":
            det = MultiStreamDetector(model, hw, max_streams=max(B, 2), batch=B, dtype=args.dtype, device=dev, pixel_format=fmt)
            det.warm_up(args.warmup)
            sids = [det.open() for _ in range(B)]
            tick_frames = fmt_frames
            det.detect_device(tick_frames[:B], sids)
        for n in ([B] if (B != 8 or args.trace) else sorted(set([int(v) for v in args.active.split(",") if v] + [B]))):
            def multi_tick():
                det.detect_device(tick_frames[:n], sids[:n])

            def uniform_tick():
                uni.detect_device(frames[:n], uni_sids[:n])
            if args.trace:
                timed(multi_tick, 20)
                print(json.dumps({"traced_batch": B, "ticks": 20}))
                return
            multi_tick()
            best_m, best_s, host_m, best_u = float("inf"), float("inf"), float("inf"), float("inf")
            m_rounds, u_rounds = [], []
            for _ in range(args.rounds):                         # alternate: clocks and neighbours drift between rounds
                if alt:
                    multi_tick()                                 # (two detectors of one batch share the plan: the untimed tick
                m, h = timed(multi_tick, args.ticks)             #  after a switch re-records its tape)
                m_rounds.append(m)
                if alt:
                    uniform_tick()
                    u_rounds.append(timed(uniform_tick, args.ticks)[0])
                    best_u = min(best_u, u_rounds[-1])
                s, _ = timed(lambda: single_tick(n), args.ticks)
                best_m, best_s, host_m = min(best_m, m), min(best_s, s), min(host_m, h)
            res["rows"].append({"batch": B, "active": n, "ms_per_tick": best_m, "frames_per_s": 1e3 * n / best_m,
                                "host_ms_per_tick": host_m, "single_ms_per_tick": best_s,
                                "single_frames_per_s": 1e3 * n / best_s, "tick_over_n_single_frames": best_m / best_s})
            if args.mixed:
                res["rows"][-1].update({"mixed": True, "uniform_ms_per_tick": best_u, "mixed_over_uniform": best_m / best_u})
            elif fmt != "bgr":
                res["rows"][-1].update({"pixel_format": fmt, "bgr_ms_per_tick": best_u, "%s_over_bgr" % fmt: best_m / best_u,
                                        "ms_rounds": m_rounds, "bgr_ms_rounds": u_rounds,
                                        "bgr_spread_over_rounds": (max(u_rounds) - min(u_rounds)) / min(u_rounds)})
            emit()
        del det, uni                                             # (their plans and pools go back to the allocator)
    print(emit())


if __name__ == "__main__":
    main()

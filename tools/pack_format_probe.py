#!/usr/bin/env python
"""The pack launch alone, per pixel format: sy_frames_u8_pack (BGR, the yardstick) against sy_frames_u8_pack_fmt (NV12 by default)
on the same pictures — batch 8 of 1200x1920 frames, decimate 2, Focus layout, fp16: the streaming detector's first launch.

Run mode issues `--launches` launches of each, interleaved (BGR, NV12, BGR, ...), after a few untimed ones; it is meant to run
under a kernel trace of its own, which the summary mode then reads: min / median / max of the kernel durations per kernel name.

    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pack_trace -- python tools/pack_format_probe.py
    python tools/pack_format_probe.py --summarize /tmp/pack_trace --out profiles/r09/pack_launch_nv12.json
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def summarize(d, out):
    dur = {}
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "frames_" in r["Kernel_Name"] and "to_focus_kernel" in r["Kernel_Name"]:
                dur.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    res = {"tool": "pack_format_probe", "what": "kernel durations in us from a rocprofv3 --kernel-trace run of this tool "
           "(launches interleaved; the first `skipped` launches of each kernel are warm-up)", "kernels": {}}
    for name, v in sorted(dur.items()):
        v = [x[1] / 1e3 for x in sorted(v)]
        skipped = min(5, max(len(v) - 1, 0))
        w = sorted(v[skipped:])
        res["kernels"][name] = {"launches": len(w), "skipped": skipped, "min_us": w[0], "median_us": w[len(w) // 2], "max_us": w[-1]}
    line = json.dumps(res, indent=1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--pixel-format", default="nv12", choices=["rgb", "nv12"])
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--summarize", default=None, help="directory of a kernel trace of this tool: print min / median / max per kernel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.out)

    import torch
    from streamyolo_amd import _lib
    from streamyolo_amd.data import FramePairsU8
    from streamyolo_amd.ops import View
    from streamyolo_amd.utils.synth import synth_frames, bgr_to_nv12
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda:0")
    B, hs, ws = args.batch, args.height, args.width
    canvas = (hs // 2, ws // 2)
    x = synth_frames(B, canvas[0], canvas[1], seed=2)[:, 0:3]
    raw = x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    raw = raw.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous().to(dev)
    other = bgr_to_nv12(raw) if args.pixel_format == "nv12" else raw.flip(-1).contiguous()
    a = FramePairsU8(raw, None, canvas, 2)
    b = FramePairsU8(other, None, canvas, 2, pixel_format=args.pixel_format)
    va = View.alloc(B, canvas[0] // 2, canvas[1] // 2, 16, args.dtype, dev)
    vb = View.alloc(B, canvas[0] // 2, canvas[1] // 2, 16, args.dtype, dev)
    for _ in range(args.launches + 5):
        a.pack_focus(va)
        b.pack_focus(vb)
    torch.cuda.synchronize()
    print(json.dumps({"launches_each": args.launches + 5, "bgr_bytes": raw.numel(), "other_bytes": other.numel(),
                      "max_abs_diff_of_outputs": float((va.buf.float() - vb.buf.float()).abs().max())}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Launch trace of the recorded training step: every C-ABI call (scalar arguments, the trailing stream dropped), every stream mark
and every snippet of the step that writes the tapes, in order, normalised (integers >= 2^32 — addresses — become p0, p1, ... in
order of first appearance) and hashed.  Two checkouts that print the same SHA-256 issue the same step.
    python tools/launch_trace.py --model nano --shape 2,32,64 --dtype fp32 --emu --set BWD_SPLIT_FRAMES=1 --out trace.txt"""
import argparse
import ast
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _Sink:
    """What _lib._TapeProxy appends to: (function, arguments without the stream, name) of every call that takes a stream."""

    def __init__(self, entries, names):
        self.entries, self.names = entries, names

    def _scalar(self, a):
        a = a.value if isinstance(a, C._SimpleCData) else a
        if isinstance(a, int) and not isinstance(a, bool) and abs(a) >= 1 << 32:
            return "p%d" % self.names.setdefault(a, len(self.names))
        return repr(a) if a is None or isinstance(a, (bool, int, float, str, bytes)) else type(a).__name__

    def append(self, call):
        self.entries.append("%s(%s)" % (call[2], ", ".join(self._scalar(a) for a in call[1])))


def trace(model="nano", shape=(2, 32, 64), dtype="fp32", device="cpu", sets=()):
    """Normalised launch trace (list of lines) of the SECOND step of a fresh model: the step that records the tapes.
    sets: (name, value) pairs assigned to train_engine module attributes or TrainPlan class attributes for the run."""
    import torch
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd import _lib, train_engine
    from streamyolo_amd.utils.synth import synth_state_dict, synth_frames, synth_labels
    saved = []
    for name, value in sets:
        holder = train_engine if hasattr(train_engine, name) else train_engine.TrainPlan
        saved.append((holder, name, getattr(holder, name)))            # AttributeError: no such switch
        setattr(holder, name, value)
    real_lib, real_mark, real_snippet = _lib.lib, _lib.NativeTape.mark, _lib.NativeTape.snippet
    entries = []
    try:
        B, H, W = shape
        cfg = O.OracleConfig.named(model)
        m = sy.build_model(model)
        m.load_state_dict(synth_state_dict(O.param_shapes(cfg), seed=0), strict=True)
        m = m.to(device).train().set_compute_dtype(dtype)
        x = synth_frames(B, H, W, seed=2).to(device)
        targets = tuple(t.to(device) for t in synth_labels(B, H, W, cfg.num_classes, num_gt=4, seed=3))
        st = train_engine.TrainStep(m, graph=False)
        st.step(x, targets)                                             # direct step: tunes
        proxy = _lib._TapeProxy(real_lib(), _Sink(entries, {}))

        def mark(self, name, arg=None):
            entries.append("mark %s %s" % (name, arg))
            return real_mark(self, name, arg)

        def snippet(self, fn):
            entries.append("snippet")
            return real_snippet(self, fn)
        _lib.lib, _lib.NativeTape.mark, _lib.NativeTape.snippet = (lambda: proxy), mark, snippet
        st.step(x, targets)                                             # recorded step
        if str(device) != "cpu":
            torch.cuda.synchronize()
        st.close()
    finally:
        _lib.lib, _lib.NativeTape.mark, _lib.NativeTape.snippet = real_lib, real_mark, real_snippet
        for holder, name, value in saved:
            setattr(holder, name, value)
    return entries


def digest(entries):
    return hashlib.sha256("\n".join(entries).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model", default="nano")
    ap.add_argument("--shape", default="2,32,64", help="B,H,W")
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE",
                    help="train_engine.NAME or TrainPlan.NAME for this run (a value is read as the type the attribute has now)")
    ap.add_argument("--emu", action="store_true", help="SIMT-emulator build of the kernels on the CPU instead of cuda:0")
    ap.add_argument("--out", help="write the normalised trace here, one entry per line")
    a = ap.parse_args()
    from streamyolo_amd import _lib, train_engine
    if a.emu:
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "streamyolo_amd", "csrc"), "-j8", "emu"], check=True)
        _lib.use_library(os.path.join(ROOT, "tests", "emu", "_build", "libstreamyolo_emu.so"))
    sets = []
    for s in a.set:
        name, _, raw = s.partition("=")
        holder = train_engine if hasattr(train_engine, name) else train_engine.TrainPlan
        sets.append((name, raw.strip("\"'") if isinstance(getattr(holder, name), str) else ast.literal_eval(raw)))
    entries = trace(a.model, tuple(int(v) for v in a.shape.split(",")), a.dtype, "cpu" if a.emu else "cuda:0", sets)
    marks = {}
    for e in entries:
        if e.startswith("mark "):
            marks[e.split()[1]] = marks.get(e.split()[1], 0) + 1
    calls = sum(1 for e in entries if not e.startswith(("mark ", "snippet")))
    print("%d entries, %d library calls, %d snippets, marks %s" % (len(entries), calls, entries.count("snippet"), dict(sorted(marks.items()))))
    print("sha256 %s" % digest(entries))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(entries) + "\n")


if __name__ == "__main__":
    main()

"""Measurements that go with the device-resident loss scaler (streamyolo_amd/amp.py); results: profiles/r07/README.md.

  python tools/scaler_probe.py timing   [--model l --batch 8 --dtype fp16 --rounds 4 --steps 10]
      same process, same box, alternating blocks: A = TrainStep.step(x, t) (today's step), B = step(x, t, scaler), and B with
      the scale pinned to 1 (same launches as B, same values as A);
      the optimizer side A = FusedSGDEMA.step(lr) vs B = step(lr, scaler=...) (check + scaled step + update);
      sy_grad_nonfinite alone over the model's arena: bytes / time.  HIP events around blocks of `steps` iterations.
  python tools/scaler_probe.py underflow [--model l --height 600 --width 960]
      one frame pair, synthetic weights (the setup of tests/test_lowp_yardstick.py): per parameter group, the fraction of
      gradient elements that are exactly zero and relative L2 / cosine to the exact-fp32 gradients, for the fp16 step at
      scale 1 and at the scale DeviceGradScaler settles on after its first skips (init 2^16).
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import streamyolo_amd as sy                                              # noqa: E402
from oracle import streamyolo_oracle as O                                # noqa: E402
from streamyolo_amd.amp import DeviceGradScaler                          # noqa: E402
from streamyolo_amd.optim import FusedSGDEMA, yolox_param_groups         # noqa: E402
from streamyolo_amd.train_engine import TrainStep                        # noqa: E402
from streamyolo_amd.utils.synth import load_bn_stats, synth_frames, synth_labels, synth_state_dict   # noqa: E402


def build(name, dtype, dev):
    cfg = O.OracleConfig.named(name)
    m = sy.build_model(name)
    m.load_state_dict(synth_state_dict(O.param_shapes(cfg), seed=0, bn_stats=load_bn_stats(name)), strict=True)
    return m.to(dev).set_compute_dtype(dtype), cfg


def block_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def timing(args, dev):
    model, cfg = build(args.model, args.dtype, dev)
    x = synth_frames(args.batch, args.height, args.width, seed=2).to(dev)
    lab, sup = [t.to(dev) for t in synth_labels(args.batch, args.height, args.width, cfg.num_classes, seed=3)]
    st, scaler = TrainStep(model, graph=False), DeviceGradScaler()
    for _ in range(4):
        st.step(x, (lab, sup))
    opt = FusedSGDEMA(model)
    for _ in range(3):                                           # let the scale settle (steps with a too large scale are skipped)
        for _ in range(6):
            st.step(x, (lab, sup), scaler=scaler)
            opt.step(1e-5, scaler=scaler)
    # the scaled code path on the UNSCALED step's data (scale pinned to 1): separates what the launch costs from what the values cost
    one = DeviceGradScaler(init_scale=1.0, growth_interval=2 ** 30)
    rows = {"step": [], "step_scaled": [], "step_scaled_at_1": [], "opt": [], "opt_scaled": [], "nonfinite": []}
    variants = [("step", None), ("step_scaled", scaler), ("step_scaled_at_1", one)]
    for r in range(3 * args.rounds):                             # back to back, the first variant of a round rotating: a block that
        for k in range(3):                                       # follows lighter work (or a pause) runs at a higher clock
            name, sc = variants[(r + k) % 3]
            rows[name].append(block_ms(lambda: st.step(x, (lab, sup), scaler=sc), args.steps))
    for _ in range(args.rounds):
        st.step(x, (lab, sup))                                   # unscaled gradients for the plain optimizer step
        rows["opt"].append(block_ms(lambda: opt.step(1e-5), args.steps))
        st.step(x, (lab, sup), scaler=scaler)
        rows["opt_scaled"].append(block_ms(lambda: opt.step(1e-5, scaler=scaler), args.steps))
        rows["nonfinite"].append(block_ms(lambda: scaler.check_gradients(opt.table, opt.n, opt.chunks), args.steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    gbytes = st.plan.arena.numel() * 4
    return {"mode": "timing", "model": args.model, "dtype": args.dtype, "batch": args.batch, "ms": rows, "median_ms": med,
            "arena_bytes": gbytes, "nonfinite_TBps": gbytes / (med["nonfinite"] * 1e-3) / 1e12, "scale": scaler.get_scale(),
            "counters": scaler.counters()}


def underflow(args, dev):
    cfg = O.OracleConfig.named(args.model)
    x = synth_frames(1, args.height, args.width, seed=2).to(dev)
    lab, sup = [t.to(dev) for t in synth_labels(1, args.height, args.width, cfg.num_classes, seed=3)]

    def grads(dtype, scaler=None, settle=0):
        model, _ = build(args.model, dtype, dev)
        st = TrainStep(model, graph=False)
        state0 = {k: v.clone() for k, v in model.state_dict().items()}
        opt = None
        for _ in range(settle):                                  # skipped steps change nothing but the scale; lr 0 on the taken ones
            model.load_state_dict(state0)
            st.step(x, (lab, sup), scaler=scaler)
            opt = opt or FusedSGDEMA(model, ema=False)
            opt.step(0.0, scaler=scaler)
        model.load_state_dict(state0)
        st.step(x, (lab, sup), scaler=scaler)
        s = 1.0 if scaler is None else scaler.get_scale()
        names = {id(p): n for n, p in model.named_parameters()}
        groups = dict(zip(("bn_weight", "weight", "bias"), yolox_param_groups(model)))
        return {g: {names[id(p)]: p.grad.detach().double().cpu() / s for p in ps} for g, ps in groups.items()}, s

    ref, _ = grads("fp32")
    out = {"mode": "underflow", "model": args.model, "size": [args.height, args.width], "columns": {}}
    scaler = DeviceGradScaler(init_scale=2.0 ** 16, growth_interval=1000)
    for tag, sc, settle in (("scale_1", None, 0), ("settled", scaler, 24)):
        got, s = grads("fp16", sc, settle)
        col = {"scale": s}
        for g in ref:
            a = torch.cat([got[g][n].reshape(-1) for n in ref[g]])
            b = torch.cat([ref[g][n].reshape(-1) for n in ref[g]])
            col[g] = {"zero_fraction": float((a == 0).double().mean()), "zero_fraction_fp32": float((b == 0).double().mean()),
                      "rel_l2": float((a - b).norm() / b.norm()), "cosine": float((a * b).sum() / (a.norm() * b.norm())),
                      "finite": bool(torch.isfinite(a).all())}
        out["columns"][tag] = col
    out["scaler_counters"] = scaler.counters()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["timing", "underflow"])
    ap.add_argument("--model", default="l")
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps(timing(args, dev) if args.mode == "timing" else underflow(args, dev)))


if __name__ == "__main__":
    main()

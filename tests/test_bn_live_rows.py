"""The exact BatchNorm-backward sums over the LIVE replica rows only (train_engine.LIVE_ROWS): the rows a reduce launch can write
come from the library's own launch geometry, the fold in front of the apply pass stops at the last of them — and every output
bit is what the fold over all rows gives.

Operands are random REAL values whose magnitudes spread over several binades, so the order of addition matters: bit equality
(torch.equal, no tolerance anywhere in this module) then says that the same additions were made in the same order.

  1. sy_bn_bwd_reduce_live_rows: rows at or above the reported count stay zero, rows below it are written;
  2. sy_bn_silu_bwd_apply_live == sy_bn_silu_bwd_apply (fold_replicas_kernel over all rows);
  3. a TrainStep with STREAMYOLO_LIVE_ROWS=1 == one with =0, in fresh processes on the same tile choices.

(The forward counterpart — live rows of the convolution statistics, finalize inside the apply pass — passed the same kind of
tests and bought no step time: it was removed together with them, profiles/r12/README.md.)"""
import os
import subprocess
import sys

import pytest
import torch

from streamyolo_amd import ops
from streamyolo_amd.ops import View

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -98765.0


def _real(shape, seed):
    """normal values times 2^k, k uniform in [-4, 4]: sums of them depend on the order of addition in fp32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * torch.exp2(torch.randint(-4, 5, shape, generator=g).float())


def _guarded(body):
    """(whole allocation, view of its middle = a copy of `body`) with a guard band of `body`'s size on either side"""
    n = body.numel()
    full = torch.full((3 * n,), SENTINEL, device=body.device)
    full[n:2 * n] = body.reshape(-1)
    return full, full[n:2 * n]


def _guards_untouched(full):
    n = full.numel() // 3
    return bool((full[:n] == SENTINEL).all()) and bool((full[2 * n:] == SENTINEL).all())


# ======================================================================================================================================
# 1. live rows are what the library says
# ======================================================================================================================================
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("C", [8, 64, 256, 1024])
def test_backward_reduce_live_rows_are_the_rows_a_launch_writes(backend, C, nseg):
    """768 rows per segment; the reduce runs min(cap / (nseg x slices), pixel rows / rows per workgroup) workgroups per segment
    and slice.  Pixel counts below and above cap x rows per workgroup (under a cap of 64 workgroups, so that "above" stays a
    small tensor): rows at or above the reported count are zero, rows below it are written."""
    dev, dt, copies, cap = backend, "bf16", 768, 64
    default = ops.bn_grid_caps()["bwd_reduce"]
    try:
        assert ops.bn_grid_caps(bwd_reduce=cap)["bwd_reduce"] == cap
        cs = max(c for c in range(8, 65, 8) if C % c == 0)                 # channel slice of a workgroup (<= 64, divides C)
        wg_cap, wg_rows = max(1, cap // (nseg * (C // cs))), 256 // (cs // 8)
        seen = set()
        for pixels in (3, wg_cap * wg_rows - 5, wg_cap * wg_rows + 7):
            if pixels < 1:
                continue
            y, da = _real((nseg, C, 1, pixels), 5 + C), _real((nseg, C, 1, pixels), 6 + C)
            yv = View.alloc(nseg, 1, pixels, C, dt, dev); yv.set_nchw(y.to(dev))
            dav = View.alloc(nseg, 1, pixels, C, dt, dev); dav.set_nchw(da.to(dev))
            aff = [_real((nseg * C,), 7 + j).to(dev) for j in range(3)] + [torch.ones(nseg * C, device=dev)]
            full, sums = _guarded(torch.zeros(nseg * copies * 2 * C, device=dev))
            ops.bn_silu_bwd_reduce(yv, dav, *aff, sums, nseg=nseg)
            live = ops.bn_bwd_reduce_live_rows(pixels, C, ops.dtype_code(dt), nseg)
            assert live == min(wg_cap, -(-pixels // wg_rows))
            rows = sums.view(nseg, copies, 2 * C).cpu()
            assert not bool(rows[:, live:].any())
            assert bool((rows[:, :live] != 0).any(2).all())
            assert _guards_untouched(full)
            seen.add(live == wg_cap)
        assert seen == {True, False}                                      # below and at the cap
    finally:
        ops.bn_grid_caps(bwd_reduce=default)


# ======================================================================================================================================
# 2. backward: replica fold over the live rows == fold_replicas_kernel over all rows
# ======================================================================================================================================
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("C", [8, 72, 256])
def test_backward_fold_over_live_rows_is_bit_equal(backend, C, nseg, dt):
    """copies = 768 (the reduce cap), n = 2C elements per row: dy, dgamma, dbeta and dres of the apply pass behind either fold."""
    dev, copies = backend, 768
    y, da = _real((nseg, C, 5, 7), 21 + C), _real((nseg, C, 5, 7), 22 + C)
    yv = View.alloc(nseg, 5, 7, C, dt, dev); yv.set_nchw(y.to(dev))
    dav = View.alloc(nseg, 5, 7, C, dt, dev); dav.set_nchw(da.to(dev))
    aff = [_real((nseg * C,), 23 + j).to(dev) for j in range(3)] + [(_real((nseg * C,), 26).abs() + 0.25).to(dev)]
    gamma = _real((C,), 27).to(dev)
    for live in (1, 3, 4, 5, 16, 17, 48, 192, 768):
        rows = _real((nseg, copies, 2 * C), 31 * live + C)
        rows[:, live:] = 0.0
        got = []
        for lv in (None, live):
            full, sums = _guarded(rows.to(dev))
            dyv, dresv = View.alloc(nseg, 5, 7, C, dt, dev, zero=True), View.alloc(nseg, 5, 7, C, dt, dev, zero=True)
            dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            ops.bn_silu_bwd_apply(yv, dav, *aff, gamma, sums, dyv, dgam, dbet, nseg=nseg, dres=dresv, live=lv)
            assert _guards_untouched(full)
            got.append((dyv.buf, dgam, dbet, dresv.buf))
        for name, a, b in zip(("dy", "dgamma", "dbeta", "dres"), *got):
            assert torch.equal(a, b), "%s differs at live %d" % (name, live)


# ======================================================================================================================================
# 3. plan level: a TrainStep with the switch on == one with it off
# ======================================================================================================================================
_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
name, dtype, where, out_path = sys.argv[2:6]
import streamyolo_amd as sy
from streamyolo_amd import _lib, train_engine
from streamyolo_amd.train_engine import TrainStep
from streamyolo_amd.utils.synth import synth_state_dict, synth_frames, synth_labels
from oracle import streamyolo_oracle as O
if where == "cpu":
    _lib.use_library(sys.argv[1] + "/tests/emu/_build/libstreamyolo_emu.so")       # built by the parent's `backend` fixture
else:
    _lib.use_library(_lib.DEFAULT_PATH)
dev = torch.device(where)
cfg = O.OracleConfig.named(name)
model = sy.build_model(name)
model.load_state_dict(synth_state_dict(O.param_shapes(cfg), seed=0), strict=True)
model = model.to(dev).train().set_compute_dtype(dtype)
model.head.use_l1 = True
x = synth_frames(2, 64, 96, seed=2).to(dev)
lab, sup = synth_labels(2, 64, 96, cfg.num_classes, num_gt=4, seed=3)
st = TrainStep(model, graph=False)
steps = []
for i in range(3):                      # direct (tuning), recorded, recorded AGAIN (the tapes are dropped in between)
    if i == 2:
        st.plan.programs.clear()
    out = st.step(x, (lab.to(dev), sup.to(dev)))
    plan = st.plan
    assert plan.exact_stats and plan.live_rows == (train_engine.LIVE_ROWS)
    steps.append(({k: v.detach().cpu().clone() for k, v in out.items() if torch.is_tensor(v)}, plan.arena.cpu().clone(),
                  {n: b.detach().cpu().clone() for n, b in model.named_buffers() if "running" in n}))
live = [(getattr(op, "live_bwd", None), op.bwd_copies) for op in plan.ops if op.kind == "conv"]
torch.save({"steps": steps, "live": live}, out_path)
"""


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["nano", "s"])
def test_train_step_is_bit_equal_with_and_without_live_rows(backend, tmp_path, name, dtype):
    """nano and s at 2 pairs of 64x96: three consecutive steps (direct, recorded, re-recorded after the tapes were dropped) with
    STREAMYOLO_LIVE_ROWS=1 against three with =0, each in a fresh process, the second on the tile choices the first one tuned
    (one tuner cache file for both; the emulator does not tune).  Loss dict, gradient arena and running statistics bit-equal."""
    res = {}
    for switch in ("0", "1"):
        env = dict(os.environ, STREAMYOLO_LIVE_ROWS=switch, STREAMYOLO_TUNE_CACHE=str(tmp_path / "tune.json"))
        out = tmp_path / ("steps_%s.pt" % switch)
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, dtype, "cpu" if str(backend) == "cpu" else "cuda:0", str(out)],
                       env=env, check=True, cwd=ROOT, timeout=1100)
        res[switch] = torch.load(out)
    assert all(lb is None for lb, _ in res["0"]["live"])
    live = res["1"]["live"]
    live = [(lb, bc) for lb, bc in live if lb is not None]          # (a paired launch notes its count on the current-frame op only)
    assert live and all(lb >= 1 for lb, _ in live)
    assert any(lb < bc for lb, bc in live)                          # the switch did cut the folds short somewhere
    for i, (a, b) in enumerate(zip(res["0"]["steps"], res["1"]["steps"])):
        assert sorted(a[0]) == sorted(b[0]) and a[0]
        for k in a[0]:
            assert torch.equal(a[0][k], b[0][k]), "step %d: %s" % (i, k)
        assert torch.equal(a[1], b[1]), "step %d: gradient arena" % i
        bad = [n for n in a[2] if not torch.equal(a[2][n], b[2][n])]
        assert not bad, "step %d: running statistics differ: %s" % (i, bad[:4])

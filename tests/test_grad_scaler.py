"""Device-resident dynamic loss scaling of the fused training path (streamyolo_amd/amp.py, sy_tal_loss_scaled,
sy_grad_nonfinite, sy_sgd_ema_step_scaled, sy_loss_scale_update) against torch.amp.GradScaler — what the reference's --fp16
trainer runs around its optimizer step (exps/train_utils/double_trainer.py:113-119)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import streamyolo_amd as sy
from oracle import streamyolo_oracle as O
from oracle.optim_oracle import ReferenceOptimEMA, param_groups
from streamyolo_amd import _lib, ops
from streamyolo_amd.amp import DeviceGradScaler
from streamyolo_amd.optim import FusedSGDEMA
from streamyolo_amd.utils.synth import synth_frames, synth_labels, synth_state_dict

FLT_MAX, FLT_MIN = 3.4028234663852886e38, 1.1754943508222875e-38


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _nano(device, dt):
    cfg = O.OracleConfig.named("nano")
    m = sy.build_model("nano")
    m.load_state_dict(synth_state_dict(O.param_shapes(cfg), seed=0), strict=True)
    m = m.to(device).train().set_compute_dtype(dt)
    m.head.use_l1 = True
    return m, cfg


def _nano_batch(device, cfg, B=2, H=64, W=96):
    x = synth_frames(B, H, W, seed=2).to(device)
    lab, sup = synth_labels(B, H, W, cfg.num_classes, num_gt=6, seed=3)
    return x, (lab.to(device), sup.to(device))


def _grad_table(tensors, device):
    """sy_optim_entry table whose gradients are `tensors` (nothing else of an entry is read by sy_grad_nonfinite)."""
    rows, chunks = [], 0
    for t in tensors:
        e = _lib.OptimEntry()
        e.p, e.g, e.buf, e.ema = t.data_ptr(), t.data_ptr(), None, None
        e.n, e.weight_decay, e.lr_mult, e.chunk0 = t.numel(), 0.0, 1.0, chunks
        chunks += -(-t.numel() // 1024)
        rows.append(e)
    arr = (_lib.OptimEntry * len(rows))(*rows)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device), len(rows), chunks


def _force_backoff(scaler, device):
    """Halve the scale ON THE DEVICE ONLY: the non-finite check over a one-element table holding inf, then the update launch."""
    bad = torch.full((1,), float("inf"), device=device)
    table, n, chunks = _grad_table([bad], device)
    scaler.check_gradients(table, n, chunks)
    scaler.update()


# ---- 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 7, 16])
def test_scaled_loss_kernel_is_the_unscaled_one_times_the_scale(backend, golden_dir, k):
    z = np.load(os.path.join(golden_dir, "nano_simota_2x96x160.npz"))
    cfg = O.OracleConfig.named("nano")
    raw = torch.from_numpy(z["raw"]).to(backend)
    lab, sup = torch.from_numpy(z["labels"]), torch.from_numpy(z["support"])
    hw = [tuple(int(v) for v in r) for r in z["hw"]]
    B, A, nch = raw.shape
    nc = cfg.num_classes
    ws = ops.TalLossWorkspace(B, A, nch, hw, cfg.strides, backend)
    args = (raw, lab, sup, nc, cfg.gamma, cfg.ignore_thr, cfg.ignore_value, True, ws)
    losses0, d0, _ = [t.clone() for t in ops.tal_loss(*args)]
    # the premise of bit-equality: a power-of-two factor is exact while nothing leaves fp32's normal range
    nz = d0[d0 != 0].abs()
    assert float(nz.min()) >= FLT_MIN and float(nz.max()) * 2.0 ** 16 < FLT_MAX
    scaler = DeviceGradScaler(init_scale=2.0 ** k)
    state = scaler.state(backend)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        pad0 = torch.zeros((B, A, 16), dtype=dt, device=backend)
        pad1 = torch.zeros((B, A, 16), dtype=dt, device=backend)
        l_null, d_null, _ = [t.clone() for t in ops.tal_loss(*args, d_pad=pad0)]
        assert torch.equal(_bits(l_null), _bits(losses0)) and torch.equal(_bits(d_null), _bits(d0))
        l1, d1, _ = [t.clone() for t in ops.tal_loss(*args, d_pad=pad1, scaler_state=state)]
        assert torch.equal(_bits(l1), _bits(losses0)), "the losses are the TRUE loss"
        assert torch.equal(_bits(d1), _bits(d0 * 2.0 ** k))
        want = torch.zeros_like(pad1)
        want[..., 0:5] = d1[..., 0:5].to(dt)                     # fp32 -> compute dtype AFTER the scaling (inf in fp16 at 2^16 included)
        want[..., 8:8 + nc] = d1[..., 5:].to(dt)
        assert torch.equal(_bits(pad1), _bits(want)), dt
        if k == 0:
            assert torch.equal(_bits(pad1), _bits(pad0))
    # NULL state pointer through the new entry point == sy_tal_loss, bit for bit
    lb = lab[..., :5].to(backend, torch.float32).contiguous()
    sp = sup[..., :5].to(backend, torch.float32).contiguous()
    ws.d_raw.zero_(); ws.losses.zero_()
    _lib.check(_lib.lib().sy_tal_loss_scaled(raw.data_ptr(), B, A, nc, lb.data_ptr(), sp.data_ptr(), ws.max_labels,
                                             C.cast(ws.lh, C.c_void_p), C.cast(ws.lw, C.c_void_p), C.cast(ws.ls, C.c_void_p),
                                             ws.nlevels, cfg.gamma, cfg.ignore_thr, cfg.ignore_value, 1, ws.d_raw.data_ptr(),
                                             ws.losses.data_ptr(), ws.fg.data_ptr(), ws.ws.data_ptr(), None, 0, None,
                                             ops.stream_of(raw)), "sy_tal_loss_scaled")
    assert torch.equal(_bits(ws.d_raw), _bits(d0)) and torch.equal(_bits(ws.losses), _bits(losses0))


# ---- 2 --------------------------------------------------------------------------------------------------------------------
def test_nonfinite_check_finds_every_planted_value_and_nothing_else(backend):
    g = torch.Generator().manual_seed(11)
    lengths = [1, 1023, 1024, 1025, 5000, 4096]
    starts = [0, 5, 1032, 2061, 3092, 8096]                      # element offsets: 16-byte aligned and not (4096-run: aligned)
    flat = (torch.randn(8096 + 4096, generator=g) * 0.1)
    flat[7] = 1e-40; flat[2062] = -1e-42                         # fp32 denormals
    flat[1033] = FLT_MAX; flat[3093] = -FLT_MAX; flat[8100] = FLT_MAX
    flat[9] = 0.0; flat[10] = -0.0
    flat = flat.to(backend)
    tensors = [flat[s:s + n] for s, n in zip(starts, lengths)]
    assert any(t.data_ptr() % 16 for t in tensors) and any(t.data_ptr() % 16 == 0 for t in tensors)
    table, n, chunks = _grad_table(tensors, backend)
    scaler = DeviceGradScaler()
    state = scaler.state(backend)

    def flag():
        scaler.check_gradients(table, n, chunks)
        f = scaler.found_inf()
        state[3] = 0
        return f
    assert not flag(), "finite values (denormals, FLT_MAX) must not trip the check"
    planted = 0
    for t in tensors:
        L = t.numel()
        spots = {0, L - 1}
        if L > 1024:
            spots |= {1023, 1024, (L // 1024) * 1024 + (L % 1024) // 2 if L % 1024 else L - 2}
        for i in sorted(spots):
            for v in (float("inf"), float("-inf"), float("nan")):
                keep = float(t[i])
                t[i] = v
                assert flag(), (L, i, v)
                t[i] = keep
                planted += 1
    assert planted >= 50 and not flag()
    # more chunks than workgroups (each workgroup then walks a run of chunks and entries): 5000 one-element tensors
    many = torch.zeros(5000 * 3, device=backend)
    mt, mn, mc = _grad_table([many[3 * j:3 * j + 1] for j in range(5000)], backend)
    assert mc > 4096
    for j in (None, 0, 2501, 4999):
        if j is not None:
            many[3 * j] = float("nan")
        scaler.check_gradients(mt, mn, mc)
        assert scaler.found_inf() == (j is not None), j
        state[3] = 0
        many.zero_()
    many[1] = float("inf")                                       # between two tensors of the table: not a gradient
    scaler.check_gradients(mt, mn, mc)
    assert not scaler.found_inf()
    # entries without gradients (EMA-only rows of the optimizer's table) are skipped, whatever their parameters hold
    e = _lib.OptimEntry()
    bad = torch.full((3,), float("nan"), device=backend)
    e.p, e.g, e.n, e.chunk0 = bad.data_ptr(), None, 3, 0
    tb = torch.frombuffer(bytearray(bytes((_lib.OptimEntry * 1)(e))), dtype=torch.uint8).to(backend)
    scaler.check_gradients(tb, 1, 1)
    assert not scaler.found_inf()


# ---- 3 --------------------------------------------------------------------------------------------------------------------
class _ThroughScaler:
    """What torch.amp.GradScaler needs of an optimizer — param_groups for unscale_, step() called only when it found no
    inf / nan — in front of the oracle's ReferenceOptimEMA.step (SGD step + EMA update)."""

    def __init__(self, ref):
        self.ref, self.param_groups, self.lr, self.taken = ref, ref.opt.param_groups, None, False

    def step(self):
        self.taken = True
        self.ref.step(self.lr, 1.0)


def _ema_only(ref, lr):
    """A skipped scaler.step is still followed by ema_model.update (double_trainer.py:115-119): the oracle's step with the
    optimizer's own step left out."""
    real = ref.opt.step
    ref.opt.step = lambda: None
    try:
        ref.step(lr, 1.0)
    finally:
        ref.opt.step = real


def test_scaled_optimizer_trajectory_matches_torch_gradscaler_sgd_ema(backend):
    cfg = O.OracleConfig.named("nano")
    sd = synth_state_dict(O.param_shapes(cfg), seed=0)
    ref_m = sy.build_model("nano"); ref_m.load_state_dict(sd, strict=True); ref_m.train()
    our_m = copy.deepcopy(ref_m).to(backend)
    ref = ReferenceOptimEMA(ref_m, lr=0.01)
    through = _ThroughScaler(ref)
    kw = dict(init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    t_scaler = torch.amp.GradScaler("cpu", **kw)
    scaler = DeviceGradScaler(**kw)
    overflow = {0: float("inf"), 4: float("nan"), 5: float("-inf"), 9: float("inf")}       # iteration 0, and two in a row
    g = torch.Generator().manual_seed(5)
    ours, pattern, scales = None, [], []
    ref_params, our_params = list(ref_m.parameters()), list(our_m.parameters())
    for it in range(14):
        lr = [0.01, 0.02, 0.005][it % 3]
        S = t_scaler.get_scale()
        assert scaler.get_scale() == S
        for j, (pr, po) in enumerate(zip(ref_params, our_params)):
            grad = torch.randn(pr.shape, generator=g) * 0.1 * S         # what a backward pass of the scaled loss leaves
            if it in overflow and j == (3 * it) % len(ref_params):
                grad.view(-1)[grad.numel() // 2] = overflow[it]
            pr.grad = grad.clone()
            if po.grad is None:
                po.grad = grad.clone().to(backend)
            else:
                po.grad.copy_(grad)
        with torch.no_grad():                                    # BatchNorm buffers move too (the EMA tracks them)
            for (_, br), (_, bo) in zip(ref_m.named_buffers(), our_m.named_buffers()):
                if br.dtype.is_floating_point:
                    delta = torch.randn(br.shape, generator=g) * 0.01
                    br.add_(delta); bo.add_(delta.to(backend))
        if ours is None:
            ours = FusedSGDEMA(our_m)
        p_before = [p.detach().clone() for p in our_params]
        buf_before, ema_before = ours.buf.clone(), ours.ema_flat.clone()
        c0 = scaler.counters()
        # reference: GradScaler.step's unscale / skip decision around the oracle's optimizer + EMA step
        through.lr, through.taken = lr, False
        t_scaler.scale(torch.zeros(1))                           # (GradScaler creates its scale tensor in scale())
        t_scaler.step(through)
        if not through.taken:
            _ema_only(ref, lr)
        t_scaler.update()
        ours.step(lr, scaler=scaler)
        c1 = scaler.counters()
        taken = c1["steps_taken"] - c0["steps_taken"]
        assert taken + (c1["steps_skipped"] - c0["steps_skipped"]) == 1
        assert bool(taken) == through.taken == (it not in overflow), it
        assert scaler.get_scale() == t_scaler.get_scale(), it
        assert c1["growth_tracker"] == t_scaler.state_dict()["_growth_tracker"], it
        assert not scaler.found_inf()
        if not taken:                                            # skipped: parameters and momentum bit-identical, EMA advanced
            assert all(torch.equal(_bits(a), _bits(p.detach())) for a, p in zip(p_before, our_params)), it
            assert torch.equal(_bits(buf_before), _bits(ours.buf)), it
            assert not torch.equal(ema_before, ours.ema_flat), it
        pattern.append(bool(taken))
        scales.append(scaler.get_scale())
    assert pattern.count(False) == 4 and max(scales) > min(scales) and 2.0 ** 10 in scales     # the scale both backed off and grew
    for (k, pr), (_, po) in zip(ref_m.named_parameters(), our_m.named_parameters()):
        assert _rel(po.detach().cpu(), pr.detach()) < 1e-6, k
    o = 0
    for p, pr in zip(ours.params, [q for grp in param_groups(ref_m) for q in grp]):
        buf = ours.buf[o:o + p.numel()].view(p.shape).cpu()
        o += p.numel()
        assert _rel(buf, ref.opt.state[pr]["momentum_buffer"]) < 1e-6
    esd, rsd = ours.ema_state_dict(), ref.ema.state_dict()
    assert set(esd) == set(rsd)
    for k in rsd:
        if rsd[k].dtype.is_floating_point:
            assert _rel(esd[k].cpu(), rsd[k]) < 1e-6, k


# ---- 4 --------------------------------------------------------------------------------------------------------------------
def test_replayed_step_reads_the_scale_from_the_device(backend):
    """Steady state (the forward / backward tapes replay), then the scale changes on the device only: the next step's arena is
    new_scale x the unscaled arena.  Exact-fp32 mode, power-of-two scales: the backward pass is linear in d_raw and every
    rounding commutes with the factor, so the comparison is bit-equality."""
    from streamyolo_amd.train_engine import TrainStep
    model, cfg = _nano(backend, "fp32")
    x, targets = _nano_batch(backend, cfg)
    st = TrainStep(model, graph=False)
    scaler = DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000)
    for _ in range(3):
        st.step(x, targets, scaler=scaler)
    replays = []
    real = st.plan._interpret
    st.plan._interpret = lambda tape: (replays.append(1), real(tape))[1]
    st.step(x, targets)                                          # same tapes, unscaled loss launch
    unscaled = st.plan.arena.clone()
    assert len(replays) == 2 and set(st.plan.programs) == {"fwd", "bwd"}
    assert float(unscaled.abs().max()) > 0 and bool(torch.isfinite(unscaled).all())
    st.step(x, targets, scaler=scaler)
    at_1024 = st.plan.arena.clone()
    _force_backoff(scaler, backend)                              # device-side only: no Python value of the scale changes hands
    st.step(x, targets, scaler=scaler)
    at_512 = st.plan.arena.clone()
    assert len(replays) == 6
    assert scaler.get_scale() == 512.0
    assert torch.equal(_bits(at_1024 / 1024.0), _bits(unscaled))
    assert torch.equal(_bits(at_512 / 512.0), _bits(unscaled))
    assert not torch.equal(at_512, at_1024)


# ---- 5 --------------------------------------------------------------------------------------------------------------------
def test_fp16_step_with_scaler_end_to_end(backend, monkeypatch):
    from streamyolo_amd.train_engine import TrainPlan, TrainStep
    monkeypatch.setattr(TrainPlan, "STAT_COPIES", 32)            # as tests/test_amp.py: keeps statistics-atomics noise out
    base, cfg = _nano(backend, "fp16")
    x, targets = _nano_batch(backend, cfg)
    x = x.to(torch.float16).float()                              # the fp16-rounded data of the drop-in AMP test
    targets = tuple(t.to(torch.float16).float() for t in targets)
    m0, m1 = copy.deepcopy(base), copy.deepcopy(base)
    st0, st1 = TrainStep(m0), TrainStep(m1)
    st0.step(x, targets)
    scaler = DeviceGradScaler(init_scale=128.0)
    st1.step(x, targets, scaler=scaler)
    g0 = dict(m0.named_parameters())
    worst = 0.0
    for n, p in m1.named_parameters():
        gr = g0[n].grad.double()
        worst = max(worst, float((p.grad.double() / 128.0 - gr).norm() / gr.norm().clamp_min(1e-12)))
    print("scaled (128) vs unscaled fp16 gradients: worst per-parameter relative L2 %.3e" % worst)
    assert worst < 2e-2

    # a scale far too large: non-finite gradients, skipped steps, the scale halves until a step is taken
    m2 = copy.deepcopy(base)
    st, big = TrainStep(m2), DeviceGradScaler(init_scale=2.0 ** 40)
    opt, taken_at = None, None
    for it in range(40):
        st.step(x, targets, scaler=big)
        if opt is None:
            opt = FusedSGDEMA(m2)
        before = [p.detach().clone() for p in m2.parameters()]
        opt.step(1e-3, scaler=big)
        c = big.counters()
        if c["steps_taken"]:
            taken_at = it
            break
        assert c["steps_skipped"] == it + 1 and big.get_scale() == 2.0 ** (40 - it - 1)
        assert all(torch.equal(_bits(a), _bits(p.detach())) for a, p in zip(before, m2.parameters())), it
    print("init_scale 2^40: first step taken at iteration %s, scale %g" % (taken_at, big.get_scale()))
    assert taken_at is not None and taken_at >= 1
    assert big.counters()["steps_skipped"] == taken_at
    assert all(bool(torch.isfinite(p.detach()).all()) for p in m2.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m2.parameters()))


# ---- 6 --------------------------------------------------------------------------------------------------------------------
def test_step_without_scaler_is_unchanged_and_scaler_adds_no_launch(backend):
    from streamyolo_amd.train_engine import TrainStep
    base, cfg = _nano(backend, "fp32")
    x, targets = _nano_batch(backend, cfg)
    runs = {}
    for tag, kw in (("plain", None), ("none", {"scaler": None}), ("one", {"scaler": DeviceGradScaler(init_scale=1.0)}),
                    ("off", {"scaler": DeviceGradScaler(enabled=False)})):
        m = copy.deepcopy(base)
        st = TrainStep(m, graph=False)
        for _ in range(3):
            out = st.step(x, targets) if kw is None else st.step(x, targets, **kw)
        runs[tag] = ({k: v.clone() for k, v in out.items()}, st.plan.arena.clone(),
                     {k: st.plan.programs[k][1].size() for k in ("fwd", "bwd")})
    for tag in ("none", "one", "off"):                           # scale 1.0: x 1.0f is exact, so even the scaled arena is bit-equal
        assert runs[tag][2] == runs["plain"][2], "launch count of the forward / backward tapes"
        assert torch.equal(_bits(runs[tag][1]), _bits(runs["plain"][1])), tag
        for k, v in runs["plain"][0].items():
            assert torch.equal(_bits(runs[tag][0][k].reshape(1)), _bits(v.reshape(1))), (tag, k)


# ---- 7 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scaled_iteration_has_no_host_synchronisation():
    from streamyolo_amd.train_engine import TrainStep
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda:0")
    model, cfg = _nano(dev, "fp16")
    x, targets = _nano_batch(dev, cfg, 2, 96, 160)
    st, scaler = TrainStep(model, graph=False), DeviceGradScaler()
    opt = None
    for _ in range(4):                                           # tuning step, recording step, two replays
        st.step(x, targets, scaler=scaler)
        if opt is None:
            opt = FusedSGDEMA(model)
        opt.step(1e-3, scaler=scaler)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if not honoured:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a deliberate .item() on this ROCm build")
        for _ in range(3):
            st.step(x, targets, scaler=scaler)
            opt.step(1e-3, scaler=scaler)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    c = scaler.counters()
    assert c["steps_taken"] + c["steps_skipped"] == 7


# ---- 8 --------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trips_with_torch_gradscaler():
    ours = DeviceGradScaler(init_scale=2.0 ** 12, growth_factor=3.0, backoff_factor=0.25, growth_interval=17)
    sd = ours.state_dict()
    assert set(sd) == set(torch.amp.GradScaler("cpu").state_dict())
    t = torch.amp.GradScaler("cpu")
    t.load_state_dict(sd)
    assert t.get_scale() == 4096.0 and t.get_growth_factor() == 3.0 and t.get_backoff_factor() == 0.25
    assert t.get_growth_interval() == 17 and t.state_dict()["_growth_tracker"] == 0
    src = torch.amp.GradScaler("cpu", init_scale=512.0, growth_factor=4.0, backoff_factor=0.125, growth_interval=9)
    tsd = src.state_dict()
    tsd["_growth_tracker"] = 5
    for materialised in (False, True):                           # before and after the device state exists
        mine = DeviceGradScaler()
        if materialised:
            mine.state("cpu")
        mine.load_state_dict(tsd)
        assert mine.state_dict() == tsd
        assert mine.get_scale() == 512.0 and mine.counters()["growth_tracker"] == 5
        st = _lib.ScalerState.from_buffer_copy(mine.state("cpu").numpy().tobytes())
        assert st.scale == 512.0 and st.inv_scale == 1.0 / 512.0 and st.growth_tracker == 5 and st.found_inf == 0
    assert DeviceGradScaler(enabled=False).state_dict() == torch.amp.GradScaler("cpu", enabled=False).state_dict() == {}
    with pytest.raises(RuntimeError):
        DeviceGradScaler().load_state_dict({})
    assert sy.DeviceGradScaler is DeviceGradScaler

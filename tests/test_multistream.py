"""Many camera streams from one batched on_pipe plan: the row-indexed state kernels (csrc/stream_state.hip), the plan's
run_stream_slots and streaming.MultiStreamDetector.

The expected values of the end-to-end tests come from the facade called the reference's way at the same batch
(`model(x, buffer=buf, mode="on_pipe")`, dfp_pafpn.py:177-228), with each row's buffer assembled by torch indexing from
per-stream buffers the test keeps itself: same plan shape, same kernels, so detections must be bit-identical
(tests/test_streaming.py::test_streaming_detector_end_to_end demands the same at batch 1)."""
import itertools

import numpy as np
import pytest
import torch

from streamyolo_amd import ops
from streamyolo_amd import streaming as S

HW, CANVAS = (128, 192), (64, 96)


def _models(backend, dtype):
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    cfg = O.OracleConfig.named("nano")
    sd = synth_state_dict(O.param_shapes(cfg), seed=0, bn_stats=load_bn_stats("nano"))
    model = sy.build_model("nano"); model.load_state_dict(sd, strict=True)
    ref = sy.build_model("nano"); ref.load_state_dict(sd, strict=True)
    return model, ref.to(backend).eval().set_compute_dtype(dtype)


def _frames(seed, n):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, HW + (3,)).astype(np.uint8) for _ in range(n)]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] is None


class _Facade:
    """The reference's loop for several cameras on a batch-`B` facade: per-stream buffers kept by the test."""

    def __init__(self, ref, backend, B):
        self.ref, self.backend, self.B = ref, backend, B
        self.buf = {}                                            # stream -> its previous buffer_ rows (3 tensors [C, H, W]) or None
        self.filler = _frames(99, 1)[0]

    def start(self, key):
        self.buf[key] = None

    def tick(self, frames, keys):
        from oracle import input_oracle as IO
        n = len(keys)
        rows = list(frames) + [self.filler] * (self.B - n)       # rows without a frame: arbitrary pixels
        x = IO.pair_tensor(np.stack(rows), None, CANVAS, 2).to(self.backend)
        with torch.no_grad():
            _, own = self.ref(x, buffer=None, mode="on_pipe")    # buffer_ = this frame's pre-fusion PAN outputs, per row
            buf = []
            for k in range(3):
                lvl = [own[k][b] if b >= n or self.buf[keys[b]] is None else self.buf[keys[b]][k] for b in range(self.B)]
                buf.append(torch.stack(lvl))
            out, _ = self.ref(x, buffer=tuple(buf), mode="on_pipe")
        for b, key in enumerate(keys):
            self.buf[key] = tuple(own[k][b].clone() for k in range(3))
        return [S.inference(out[b], 8, 0.01, 0.65, 0.5) for b in range(n)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_state_kernels_match_torch_indexing(backend, dtype):
    """sy_stream_state_gather / _scatter == torch indexing on sliced views (c_off > 0, ld > C), for every mix of first /
    continuing / inactive rows; rows the scatter must skip stay untouched."""
    g = torch.Generator().manual_seed(5)
    B, Sn = 3, 5
    shapes = [(6, 8, 32), (3, 4, 64), (2, 2, 128)]               # (H, W, C) of three levels
    ld_off = [(80, 16), (96, 32), (128, 0)]                      # (ld, c_off): channel slices of wider buffers; the last one dense

    def rnd(*shape):
        return (torch.rand(shape, generator=g) * 8 - 4).to(dtype).to(backend)
    curs, wide = [], []
    for (H, W, C), (ld, off) in zip(shapes, ld_off):
        w = rnd(B, H, W, ld)
        wide.append(w)
        curs.append(ops.View(w, B, H, W, ld).slice(off, C))
    kinds = ("first", "cont", "off")
    for mix in itertools.product(kinds, repeat=B):
        slots = [4, 0, 2]
        row_slot = torch.tensor([-1 if m == "off" else s for m, s in zip(mix, slots)], dtype=torch.int32, device=backend)
        row_first = torch.tensor([1 if m == "first" else 0 for m in mix], dtype=torch.uint8, device=backend)
        if mix[2] == "off":
            row_first[2] = 1                                     # a first flag on a row without a slot changes nothing
        pools = [rnd(Sn, H, W, C) for H, W, C in shapes]
        before = [p.clone() for p in pools]
        for k, ((H, W, C), (ld, off)) in enumerate(zip(shapes, ld_off)):
            supw = rnd(B, H, W, ld)
            keep = supw.clone()
            sup = ops.View(supw, B, H, W, ld).slice(off, C)
            ops.stream_state_gather(curs[k], pools[k], sup, row_slot, row_first)
            want = keep.clone()
            for b, m in enumerate(mix):
                want[b, :, :, off:off + C] = pools[k][slots[b]] if m == "cont" else wide[k][b, :, :, off:off + C]
            assert torch.equal(supw, want), (mix, k)             # the channels outside the slice included
        ops.stream_state_scatter(curs, pools, row_slot)
        for k, ((H, W, C), (ld, off)) in enumerate(zip(shapes, ld_off)):
            want = before[k].clone()
            for b, m in enumerate(mix):
                if m != "off":
                    want[slots[b]] = wide[k][b, :, :, off:off + C]
            assert torch.equal(pools[k], want), (mix, k)
    assert all(torch.equal(c.buf, w) for c, w in zip(curs, wide))


def test_state_kernels_reject_bad_arguments(backend):
    """Status codes only: misaligned 16-byte pieces and null pointers are SY_ERR_ARG."""
    from streamyolo_amd import _lib
    B, H, W, C = 2, 2, 2, 8
    cur = ops.View.alloc(B, H, W, C + 4, torch.float32, backend)                # fp32: ld = 12 elements = 48 bytes is fine ...
    pool = torch.zeros((3, H, W, 4), dtype=torch.float32, device=backend)
    sup = ops.View.alloc(B, H, W, 4, torch.float32, backend)
    row_slot = torch.zeros(B, dtype=torch.int32, device=backend)
    row_first = torch.zeros(B, dtype=torch.uint8, device=backend)
    ops.stream_state_gather(cur.slice(4, 4), pool, sup, row_slot, row_first)
    with pytest.raises(_lib.HipLibraryError, match="bad argument"):             # ... a slice starting 8 bytes in is not
        ops.stream_state_gather(cur.slice(2, 4), pool, sup, row_slot, row_first)
    with pytest.raises(_lib.HipLibraryError, match="bad argument"):
        ops.stream_state_scatter([cur.slice(2, 4)], [pool], row_slot)
    lib = _lib.lib()
    assert lib.sy_stream_state_gather(None, 4, 16, pool.data_ptr(), 3, sup.ptr(), 4, 16, B, H, W, 4, row_slot.data_ptr(),
                                      row_first.data_ptr(), _lib.DT_F32, ops.stream_of(pool)) == 1
    assert lib.sy_stream_state_scatter(None, 1, 3, B, row_slot.data_ptr(), _lib.DT_F32, ops.stream_of(pool)) == 1


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_lockstep_equals_the_facade(backend):
    """batch = 3, three streams, every stream in every tick, four ticks, fp32 == the facade at batch 3 with `buf` carried."""
    from oracle import input_oracle as IO
    model, ref = _models(backend, "fp32")
    det = S.MultiStreamDetector(model, HW, max_streams=3, batch=3, dtype="fp32", device=backend)
    det.warm_up(2)
    sids = [det.open() for _ in range(3)]
    frames = [_frames(10 + t, 3) for t in range(4)]
    got = [det(f, sids) for f in frames]
    buf = None
    with torch.no_grad():
        for t, f in enumerate(frames):
            x = IO.pair_tensor(np.stack(f), None, CANVAS, 2).to(backend)
            out, buf = ref(x, buffer=buf, mode="on_pipe")
            for b in range(3):
                assert _same(got[t][b], S.inference(out[b], 8, 0.01, 0.65, 0.5)), (t, b)
    assert sum(len(r[0]) for tick in got for r in tick) > 0


# ---- 3 + 6 --------------------------------------------------------------------------------------------------------------------
def test_interleaved_streams_resets_and_errors(backend):
    """Streams that tick in different subsets and orders, a reset, a close-and-reopen that reuses a slot, and the documented
    errors in between (none of which may leave a slot half-written): every active row of every tick == the facade at batch 3
    over buffers assembled per row."""
    model, ref = _models(backend, "fp32")
    det = S.MultiStreamDetector(model, HW, max_streams=3, batch=3, dtype="fp32", device=backend)
    fac = _Facade(ref, backend, 3)
    det.warm_up(2)
    sid = [det.open() for _ in range(3)]
    for s in sid:
        fac.start(s)
    with pytest.raises(RuntimeError):
        det.open()                                               # max_streams are open
    seed = [100]

    def tick(order):
        seed[0] += 1
        f = _frames(seed[0], len(order))
        ids = [sid[i] for i in order]
        got, want = det(f, ids), fac.tick(f, ids)
        assert len(got) == len(order)
        for b in range(len(order)):
            assert _same(got[b], want[b]), (seed[0], order, b)
        return got
    tick([0, 1, 2])
    tick([2, 0])
    with pytest.raises(ValueError):
        det(_frames(1, 2), [sid[1], sid[1]])                     # a stream id twice in one tick
    tick([1])
    det.reset(sid[1]); fac.start(sid[1])                         # a new sequence on stream 1 between ticks 3 and 4
    with pytest.raises(ValueError):
        det([np.zeros((64, 96, 3), np.uint8)], [sid[0]])         # wrong frame shape
    with pytest.raises(ValueError):
        det([_frames(1, 1)[0], np.zeros((64, 96, 3), np.uint8)], [sid[2], sid[0]])   # ... behind a good frame: nothing staged
    tick([1, 0, 2])
    old = sid[2]
    det.close(old)
    with pytest.raises(ValueError):
        det(_frames(2, 1), [old])                                # closed id
    with pytest.raises(ValueError):
        det(_frames(2, 2), [sid[0], 12345])                      # unknown id beside a valid one
    sid[2] = det.open(); fac.start(sid[2])                       # reuses the slot; the stale state in it must not be read
    assert sid[2] != old and det._slot_of[sid[2]] == 2
    tick([2])
    got = tick([2, 1, 0])
    assert sum(len(r[0]) for r in got) > 0
    # n > batch: consecutive ticks, results in the order given (stream 0 has two frames: they land in different ticks)
    f = _frames(777, 4)
    ids = [sid[0], sid[1], sid[2], sid[0]]
    got = det(f, ids)
    want = fac.tick(f[:3], ids[:3]) + fac.tick(f[3:], ids[3:])
    assert len(got) == 4 and all(_same(a, b) for a, b in zip(got, want))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_rows_are_independent(backend, dtype, monkeypatch):
    """Stream A's detections over five frames are bit-identical whether A runs alone (other rows inactive), beside two other
    streams, or in another batch row — one detector object; fp16 with split-K on."""
    from streamyolo_amd import engine
    if dtype == "fp16":
        monkeypatch.setenv("STREAMYOLO_STREAM_SPLITK", "1")
        if backend.type == "cpu":
            monkeypatch.setattr(engine, "FORCE_SPLIT_K", (2, 118))               # the emulator has no tuner
    model, _ = _models(backend, dtype)
    det = S.MultiStreamDetector(model, HW, max_streams=4, batch=3, dtype=dtype, device=backend)
    det.warm_up(2)
    if dtype == "fp16":
        assert det.plan.allow_split_k
        if backend.type == "cpu":
            assert sum(1 for op in det.plan.ops if op.kind == "conv" and op._tiles.get("splitk", (1,))[0] > 1) >= 1
    a, b, c = det.open(), det.open(), det.open()
    fa, fb, fc = _frames(21, 5), _frames(22, 5), _frames(23, 5)
    alone = [det([fa[t]], [a])[0] for t in range(5)]
    for s in (a, b, c):
        det.reset(s)
    beside = [det([fa[t], fb[t], fc[t]], [a, b, c])[0] for t in range(5)]
    for s in (a, b, c):
        det.reset(s)
    moved = [det([fc[t], fb[4 - t], fa[t]], [b, c, a])[2] for t in range(5)]
    assert sum(len(r[0]) for r in alone) > 0
    for t in range(5):
        assert _same(alone[t], beside[t]) and _same(alone[t], moved[t]), t
    # the state matters: the same frame with another history gives another answer somewhere
    det.reset(a)
    fresh = det([fa[4]], [a])[0]
    assert not (np.array_equal(fresh[0], alone[4][0]) and np.array_equal(fresh[1], alone[4][1]))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_every_tick_is_one_replay_of_one_tape(backend):
    """After warm_up every tick — ticks with first rows included — replays the same tape object; the launch list has the three
    gathers and the one scatter, no sy_view_copy.  On the GPU: detect_device with changing stream ids makes no host read."""
    from streamyolo_amd import _lib
    model, _ = _models(backend, "fp32")
    det = S.MultiStreamDetector(model, HW, max_streams=4, batch=3, dtype="fp32", device=backend)
    assert det.plan._slots_tape is None
    det.warm_up(2)
    tape = det.plan._slots_tape[2]
    n_launch = tape.size()
    sid = [det.open() for _ in range(3)]
    for t, order in enumerate(([0, 1, 2], [1], [2, 0], [0, 1, 2])):
        if t == 3:
            det.reset(sid[0])
        det(_frames(40 + t, len(order)), [sid[i] for i in order])
        assert det.plan._slots_tape[2] is tape and tape.size() == n_launch
    with _lib.record() as calls, torch.no_grad():                # the C-ABI calls of one tick through the wrappers
        det.plan.run_stream_slots(det._in, det.state)
    names = [c[2] for c in calls]
    assert "sy_view_copy" not in names
    assert names.count("sy_stream_state_gather") == 3 and names.count("sy_stream_state_scatter") == 1
    assert names[-1] == "sy_stream_state_scatter"
    at = [i for i, n in enumerate(names) if n == "sy_stream_state_gather"]
    assert all(names[i + 1] == "sy_conv2d" and names[i + 2] == "sy_conv2d" for i in at)   # directly in front of the fusion convs
    if backend.type != "cuda":
        return
    frames = [[torch.from_numpy(f).pin_memory() for f in _frames(60 + t, 2)] for t in range(3)]
    want = []
    for s in sid:
        det.reset(s)
    for t, order in enumerate(([0, 1], [2, 0], [1, 2])):
        d, c, n = det.detect_device(frames[t], [sid[i] for i in order])
        want.append((d[:n].clone(), c[:n].clone()))
    for s in sid:
        det.reset(s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    got = []
    try:
        for t, order in enumerate(([0, 1], [2, 0], [1, 2])):
            d, c, n = det.detect_device(frames[t], [sid[i] for i in order])
            got.append((d[:n].clone(), c[:n].clone()))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert det.plan._slots_tape[2] is tape
    for (d0, c0), (d1, c1) in zip(want, got):
        assert torch.equal(c0, c1) and int(c0.max()) > 0
        for b in range(c0.numel()):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c0[b])])

"""Cameras of different resolutions in one batched on_pipe plan: the per-row pack kernel (sy_frames_u8_pack_rows,
csrc/input_pipeline.hip), data.FrameRowsU8 and MultiStreamDetector's mixed mode (max_frame_hw).

The kernel's yardsticks are sy_frames_u8_pack on each frame alone (bit for bit: both kernels call the same per-pixel
functions) and oracle/input_oracle.py; the detector's is the facade called the reference's way at the same batch over
per-stream buffers the test keeps itself, as in tests/test_multistream.py — same plan shape, same kernels, so detections
must be bit-identical."""
import numpy as np
import pytest
import torch

from oracle import input_oracle as IO
from streamyolo_amd import _lib, ops
from streamyolo_amd import streaming as S
from streamyolo_amd.data import FramePairsU8, FrameRowsU8, row_geometry
from streamyolo_amd.ops import View

HW, CANVAS = (128, 192), (64, 96)                                # the detector tests: tests/test_multistream.py's sizes
OTHER = (90, 150)                                                # neither the canvas nor twice it: r = 0.64, a 57 x 96 image


# ---- 1: the kernel ------------------------------------------------------------------------------------------------------------
K_CANVAS = (32, 64)
# (Hs, Ws, decimate, mirror) of rows 0..4; row 5 has no frame
K_ROWS = [(32, 64, 1, 0),                                        # the canvas itself: copy
          (64, 128, 2, 0),                                       # exactly twice the canvas: 2x decimation
          (40, 72, 0, 0),                                        # r = 0.8 set by the height: 32 x 57, padding on the right
          (50, 20, 0, 0),                                        # tall: r = 0.64, 32 x 12, wide padding
          (33, 70, -1, 1)]                                       # per-axis stretch to the canvas, mirrored
K_B = len(K_ROWS) + 1


def _k_frames():
    rng = np.random.RandomState(7)
    return [rng.randint(0, 256, (hs, ws, 3)).astype(np.uint8) for hs, ws, _, _ in K_ROWS]


def _oracle_row(frame, dec, mirror):
    """fp32 [3, H, W] of one frame on the canvas, from the oracle's own functions."""
    if frame is None:
        return np.full((3,) + K_CANVAS, 114.0, dtype=np.float32)
    if dec == -1:
        img = IO.cv2_resize_linear_u8(frame, (K_CANVAS[1], K_CANVAS[0]))
        return IO.preproc(IO.mirror_image(img, bool(mirror)), K_CANVAS)
    return IO.pair_tensor(frame[None], None, K_CANVAS, dec, np.array([mirror], dtype=np.uint8))[0].numpy()


@pytest.mark.parametrize("out_size", [(32, 64), (16, 32)])
def test_rows_kernel_is_bit_exact(backend, out_size):
    """One call, six rows of five geometries and an empty row: every row == sy_frames_u8_pack on that frame alone (torch.equal;
    NCHW fp32 and Focus fp32 / fp16 / bf16) and == the oracle (bit-exact at the canvas size; through F.interpolate within the
    bound below at 16 x 32, where the canvas-resize stage runs); the empty row is all 114; a second call of the SAME launch
    (identical C-ABI arguments) over permuted rows gives the permuted outputs.
    Oracle bound at 16 x 32: fp32 1e-5 * 255 (tests/test_data.py's bound for this bilinear stage against F.interpolate); 16-bit
    storage adds at most one unit in the last place at values <= 255 (two fp32 values that close round to the same or to
    neighbouring numbers): 0.125 for fp16, 1.0 for bf16."""
    frames = _k_frames()
    resize = out_size != K_CANVAS
    rows = FrameRowsU8(K_B, (64, 128), K_CANVAS, backend, out_size=out_size)
    assert tuple(rows.shape) == (K_B, 3) + out_size and rows.size(0) == K_B and rows.dtype == torch.float32
    assert rows.device == backend and rows.float() is rows and rows.contiguous() is rows

    def fill(order):
        for b, k in enumerate(order):
            if k is None:
                rows.set_row(b, None)
            else:
                _, _, dec, mir = K_ROWS[k]
                rows.set_row(b, frames[k], mirror=bool(mir), decimate=dec, divisor=1.0)
        rows.upload()

    def alone(k, view=None):
        """sy_frames_u8_pack on frame k alone (k None: nothing to run, the plain canvas)."""
        hs, ws, dec, mir = K_ROWS[k]
        one = FramePairsU8(torch.from_numpy(frames[k]).unsqueeze(0).to(backend), None, K_CANVAS, dec,
                           torch.tensor([mir], dtype=torch.uint8, device=backend), out_size)
        if view is None:
            return one.to_nchw()[0]
        one.pack_focus(view)
        return view.buf.reshape(out_size[0] // 2, out_size[1] // 2, 16).clone()

    order = [0, 1, 2, 3, 4, None]
    want_nchw = torch.from_numpy(np.stack([_oracle_row(None if k is None else frames[k], *(K_ROWS[k][2:] if k is not None else (1, 0)))
                                           for k in order]))
    if resize:
        want_nchw, _ = IO.exp_preprocess(want_nchw, (torch.zeros(K_B, 1, 5), torch.zeros(K_B, 1, 5)), out_size, K_CANVAS)
    fill(order)
    with _lib.record() as first_calls:
        got = rows.to_nchw()
    nchw = got.cpu()
    for b, k in enumerate(order):
        if k is None:
            assert torch.equal(nchw[b], torch.full_like(nchw[b], 114.0))
        else:
            assert torch.equal(got[b], alone(k)), ("nchw", b)
    if resize:
        assert float((nchw - want_nchw).abs().max()) <= 1e-5 * 255.0
    else:
        assert torch.equal(nchw, want_nchw)
    focus = {}
    for dt, ulp in (("fp32", 0.0), ("fp16", 0.125), ("bf16", 1.0)):
        v = View.alloc(K_B, out_size[0] // 2, out_size[1] // 2, 16, dt, backend)
        rows.pack_focus(v)
        f = v.buf.reshape(K_B, out_size[0] // 2, out_size[1] // 2, 16).clone()
        focus[dt] = f
        one = View.alloc(1, out_size[0] // 2, out_size[1] // 2, 16, dt, backend)
        for b, k in enumerate(order):
            if k is not None:
                assert torch.equal(f[b], alone(k, one)), (dt, b)
        tdt = ops.TORCH_DTYPE[ops.dtype_code(dt)]
        want = IO.focus_pack(want_nchw)
        assert torch.equal(f[..., 12:], torch.zeros_like(f[..., 12:]))
        assert torch.equal(f[5, ..., :12].cpu().float(), torch.full((out_size[0] // 2, out_size[1] // 2, 12), 114.0))
        if resize:
            assert float((f[..., :12].cpu().float() - want.to(tdt).float()).abs().max()) <= ulp + 1e-5 * 255.0, dt
        else:
            assert torch.equal(f[..., :12].cpu().float(), want.to(tdt).float()), dt
    # the same launch, the rows somewhere else: nothing of a geometry is in the launch
    perm = [3, None, 4, 0, 2, 1]
    fill(perm)
    with _lib.record() as second_calls:
        got2 = rows.to_nchw()
    (_, a1, name1), (_, a2, name2) = first_calls[0], second_calls[0]
    assert len(first_calls) == len(second_calls) == 1 and name1 == name2 == "sy_frames_u8_pack_rows"
    assert a1[:7] + a1[8:] == a2[:7] + a2[8:]                    # (all but the freshly allocated output)
    v = View.alloc(K_B, out_size[0] // 2, out_size[1] // 2, 16, "fp16", backend)
    rows.pack_focus(v)
    f2 = v.buf.reshape(K_B, out_size[0] // 2, out_size[1] // 2, 16)
    for b2, k in enumerate(perm):
        b = order.index(k)
        assert torch.equal(got2[b2], got[b]) and torch.equal(f2[b2], focus["fp16"][b]), (b2, k)


# ---- 2: rejections ------------------------------------------------------------------------------------------------------------
def test_rows_entry_point_rejects_bad_arguments(backend):
    """Status codes only (SY_ERR_ARG = 1): null table, null output, B = 0, odd Ho with the Focus layout, unknown layout / dtype."""
    lib = _lib.lib()
    rows = FrameRowsU8(2, (8, 8), (8, 8), backend)
    out = torch.zeros((2, 3, 8, 8), dtype=torch.float32, device=backend)
    t, o, st = rows.table.data_ptr(), out.data_ptr(), ops.stream_of(out)
    assert lib.sy_frames_u8_pack_rows(t, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 0
    assert lib.sy_frames_u8_pack_rows(None, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 1
    assert lib.sy_frames_u8_pack_rows(t, 2, 8, 8, 8, 8, ops.FRAMES_NCHW, None, _lib.DT_F32, st) == 1
    assert lib.sy_frames_u8_pack_rows(t, 0, 8, 8, 8, 8, ops.FRAMES_NCHW, o, _lib.DT_F32, st) == 1
    assert lib.sy_frames_u8_pack_rows(t, 2, 8, 8, 7, 8, ops.FRAMES_FOCUS, o, _lib.DT_F32, st) == 1
    assert lib.sy_frames_u8_pack_rows(t, 2, 8, 8, 8, 7, ops.FRAMES_FOCUS, o, _lib.DT_F32, st) == 1
    assert lib.sy_frames_u8_pack_rows(t, 2, 8, 8, 8, 8, 2, o, _lib.DT_F32, st) == 1
    assert lib.sy_frames_u8_pack_rows(t, 2, 8, 8, 8, 8, ops.FRAMES_FOCUS, o, 7, st) == 1
    assert torch.equal(out.cpu(), torch.full((2, 3, 8, 8), 114.0))               # (only the good call wrote)
    # the Python layer validates what the host side of the C entry point cannot see
    with pytest.raises(ValueError):
        rows.set_row(0, np.zeros((9, 8, 3), np.uint8))                           # above max_frame_hw
    with pytest.raises(ValueError):
        rows.set_row(0, np.zeros((8, 8), np.uint8))                              # not [Hs, Ws, 3]
    with pytest.raises(ValueError):
        rows.set_row(0, np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        rows.set_row(0, np.zeros((6, 6, 3), np.uint8), decimate=1)               # ratio 1 does not letterbox 6x6 onto 8x8
    with pytest.raises(ValueError):
        rows.set_row(2, None)
    with pytest.raises(ValueError):
        row_geometry((400, 2), (8, 8))                                           # int(ws * r) < 1
    assert row_geometry((8, 8), (8, 8)) == (1, 1.0) and row_geometry((16, 16), (8, 8)) == (2, 0.5)
    assert row_geometry((10, 20), (8, 8)) == (0, 0.4) and row_geometry((10, 20), (8, 8), -1) == (-1, None)


def _models(backend, dtype):
    import streamyolo_amd as sy
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, load_bn_stats
    cfg = O.OracleConfig.named("nano")
    sd = synth_state_dict(O.param_shapes(cfg), seed=0, bn_stats=load_bn_stats("nano"))
    model = sy.build_model("nano"); model.load_state_dict(sd, strict=True)
    ref = sy.build_model("nano"); ref.load_state_dict(sd, strict=True)
    return model, ref.to(backend).eval().set_compute_dtype(dtype)


def _frames(seed, hw, n=1):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, tuple(hw) + (3,)).astype(np.uint8) for _ in range(n)]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] is None


def test_python_layer_rejects_and_leaves_the_state_alone(backend):
    """ValueError for a frame that is not of its stream's size, a geometry above max_frame_hw, a geometry that leaves no pixels
    and open(frame_hw=...) on a uniform detector — each found before anything is written: stream A's detections over the ticks
    around the errors equal those of an undisturbed run."""
    model, _ = _models(backend, "fp32")
    uniform = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend)
    with pytest.raises(ValueError):
        uniform.open(frame_hw=CANVAS)
    assert uniform.open() == 0 and uniform._free == [1]                          # the failed open took neither a slot nor an id
    fa, fb = _frames(31, OTHER, 4), _frames(32, CANVAS, 4)

    def run(disturb):
        det = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend, max_frame_hw=HW)
        det.warm_up(2)
        a, b = det.open(frame_hw=OTHER), det.open(frame_hw=CANVAS)
        got = []
        for t in range(4):
            if disturb and t == 1:
                with pytest.raises(ValueError):
                    det.open(frame_hw=(129, 192))                                # above max_frame_hw
                with pytest.raises(ValueError):
                    det.open(frame_hw=(128, 1))                                  # int(ws * r) < 1
                with pytest.raises(RuntimeError):
                    det.open(frame_hw=CANVAS)                                    # (both streams are open)
            if disturb and t == 2:
                with pytest.raises(ValueError):
                    det([fa[t], fa[t]], [a, b])                                  # b's frames are canvas-sized: behind a good frame
                with pytest.raises(ValueError):
                    det([fb[t]], [a])
                with pytest.raises(ValueError):
                    det.detect_device([fa[t], fb[t], fb[t]], [a, b, b])          # more rows than the batch
            got.append(det([fa[t], fb[t]], [a, b]))
        assert det._next_id == 2
        return got
    want, got = run(False), run(True)
    assert sum(len(r[0]) for tick in want for r in tick) > 0
    for t in range(4):
        assert _same(got[t][0], want[t][0]) and _same(got[t][1], want[t][1]), t


# ---- 3: the detector against the facade --------------------------------------------------------------------------------------------
class _Facade:
    """The reference's loop for several cameras on a batch-`B` facade (tests/test_multistream.py's, with a size per stream):
    per-stream buffers kept by the test, every frame through the oracle's `preproc` of its own size."""

    def __init__(self, ref, backend, B):
        self.ref, self.backend, self.B = ref, backend, B
        self.buf, self.mode, self.div = {}, {}, {}

    def start(self, key, mode=None, div=None):
        self.buf[key] = None
        if mode is not None:
            self.mode[key], self.div[key] = mode, div

    def tick(self, frames, keys):
        n = len(keys)
        x = [IO.pair_tensor(f[None], None, CANVAS, self.mode[k]) for f, k in zip(frames, keys)]
        x += [torch.full((1, 3) + CANVAS, 114.0)] * (self.B - n)  # rows without a frame: the plain canvas
        x = torch.cat(x).to(self.backend)
        with torch.no_grad():
            _, own = self.ref(x, buffer=None, mode="on_pipe")    # buffer_ = this frame's pre-fusion PAN outputs, per row
            buf = []
            for k in range(3):
                lvl = [own[k][b] if b >= n or self.buf[keys[b]] is None else self.buf[keys[b]][k] for b in range(self.B)]
                buf.append(torch.stack(lvl))
            out, _ = self.ref(x, buffer=tuple(buf), mode="on_pipe")
        for b, key in enumerate(keys):
            self.buf[key] = tuple(own[k][b].clone() for k in range(3))
        return [S.inference(out[b], 8, 0.01, 0.65, self.div[keys[b]]) for b in range(n)]


def test_mixed_detector_equals_the_facade(backend):
    """Streams of the canvas size, twice the canvas and an unrelated size (and one opened without a size: the detector's own
    camera) interleaved over ticks with absent streams and a reset mid-way, fp32: every active row == the facade at batch 3
    over `preproc`'s letterbox of that camera, boxes / r (bit-identical, as tests/test_multistream.py demands of the uniform
    detector)."""
    model, ref = _models(backend, "fp32")
    det = S.MultiStreamDetector(model, HW, max_streams=4, batch=3, dtype="fp32", device=backend, max_frame_hw=(128, 192))
    fac = _Facade(ref, backend, 3)
    det.warm_up(2)
    sizes = [CANVAS, HW, OTHER, HW]
    sid = [det.open(frame_hw=CANVAS), det.open(frame_hw=HW), det.open(frame_hw=OTHER), det.open()]
    r_other = min(CANVAS[0] / OTHER[0], CANVAS[1] / OTHER[1])
    for s, mode, div in zip(sid, (1, 2, 0, 2), (1.0, 0.5, r_other, 0.5)):
        fac.start(s, mode, div)
    assert [det._geom[s][1:] for s in sid] == [(1, 1.0), (2, 0.5), (0, r_other), (2, 0.5)]
    seed = [200]

    def tick(order):
        seed[0] += 1
        f = [_frames(seed[0] * 10 + i, sizes[i])[0] for i in order]
        ids = [sid[i] for i in order]
        got, want = det(f, ids), fac.tick(f, ids)
        assert len(got) == len(order)
        for b in range(len(order)):
            assert _same(got[b], want[b]), (seed[0], order, b)
        return got
    tick([0, 1, 2])
    tick([2, 0])                                                 # stream 1 absent, the others in other rows
    tick([1, 3])
    det.reset(sid[2]); fac.start(sid[2])                         # a new sequence on the letterboxed stream
    tick([2, 1, 0])
    got = tick([3, 2, 1])
    assert sum(len(r[0]) for r in got) > 0
    # a slot reopened with another geometry: the pools are canvas-sized, the stale state in it is not read
    old = sid[0]
    det.close(old)
    sid[0], sizes[0] = det.open(frame_hw=OTHER), OTHER
    fac.start(sid[0], 0, r_other)
    assert sid[0] != old and det._slot_of[sid[0]] == 0
    tick([0, 2])
    # n > batch: consecutive ticks, results in the order given
    order = [0, 1, 2, 3]
    f = [_frames(900 + i, sizes[i])[0] for i in order]
    got = det(f, sid)
    want = fac.tick(f[:3], sid[:3]) + fac.tick(f[3:], sid[3:])
    assert len(got) == 4 and all(_same(a, b) for a, b in zip(got, want))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_rows_are_independent_of_other_cameras(backend, dtype, monkeypatch):
    """Stream A's detections over five frames are bit-identical whether the other rows of its ticks are empty, carry cameras of
    other sizes, or A sits in another batch row — one detector object; fp16 with split-K on."""
    from streamyolo_amd import engine
    if dtype == "fp16":
        monkeypatch.setenv("STREAMYOLO_STREAM_SPLITK", "1")
        if backend.type == "cpu":
            monkeypatch.setattr(engine, "FORCE_SPLIT_K", (2, 118))               # the emulator has no tuner
    model, _ = _models(backend, dtype)
    det = S.MultiStreamDetector(model, HW, max_streams=4, batch=3, dtype=dtype, device=backend, max_frame_hw=HW)
    det.warm_up(2)
    if dtype == "fp16":
        assert det.plan.allow_split_k
        if backend.type == "cpu":
            assert sum(1 for op in det.plan.ops if op.kind == "conv" and op._tiles.get("splitk", (1,))[0] > 1) >= 1
    a, b, c = det.open(frame_hw=OTHER), det.open(frame_hw=HW), det.open(frame_hw=CANVAS)
    fa, fb, fc = _frames(21, OTHER, 5), _frames(22, HW, 5), _frames(23, CANVAS, 5)
    alone = [det([fa[t]], [a])[0] for t in range(5)]
    for s in (a, b, c):
        det.reset(s)
    beside = [det([fa[t], fb[t], fc[t]], [a, b, c])[0] for t in range(5)]
    for s in (a, b, c):
        det.reset(s)
    moved = [det([fc[t], fb[4 - t], fa[t]], [c, b, a])[2] for t in range(5)]
    assert sum(len(r[0]) for r in alone) > 0
    for t in range(5):
        assert _same(alone[t], beside[t]) and _same(alone[t], moved[t]), t
    # the state matters: the same frame with another history gives another answer somewhere
    det.reset(a)
    fresh = det([fa[4]], [a])[0]
    assert not (np.array_equal(fresh[0], alone[4][0]) and np.array_equal(fresh[1], alone[4][1]))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_every_mixed_tick_is_one_replay_of_one_tape(backend):
    """After warm_up every tick — whatever sizes its rows have, first rows included — replays the same tape object, and no new
    tape is recorded; the launch list starts with the ONE rows pack launch.  detect_device returns the per-row divisors."""
    model, _ = _models(backend, "fp32")
    det = S.MultiStreamDetector(model, HW, max_streams=4, batch=3, dtype="fp32", device=backend, max_frame_hw=HW)
    assert det.plan._slots_tape is None
    det.warm_up(2)
    tape = det.plan._slots_tape[2]
    n_launch = tape.size()
    sizes = [CANVAS, HW, OTHER]
    sid = [det.open(frame_hw=hw) for hw in sizes]
    for t, order in enumerate(([0, 1, 2], [2], [1, 0], [2, 1, 0], [0, 2])):
        if t == 3:
            det.reset(sid[0])
        det([_frames(40 + 3 * t + i, sizes[i])[0] for i in order], [sid[i] for i in order])
        assert det.plan._slots_tape[2] is tape and tape.size() == n_launch
    d, c, n, div = det.detect_device([_frames(70, OTHER)[0], _frames(71, HW)[0]], [sid[2], sid[1]])
    assert det.plan._slots_tape[2] is tape and tape.size() == n_launch
    assert n == 2 and d.shape[0] == 3 and div.device == d.device
    r_other = min(CANVAS[0] / OTHER[0], CANVAS[1] / OTHER[1])
    assert torch.equal(div.cpu(), torch.tensor([r_other, 0.5, 1.0], dtype=torch.float32))
    with _lib.record() as calls, torch.no_grad():                # the C-ABI calls of one tick through the wrappers
        det.plan.run_stream_slots(det._in, det.state)
    names = [c[2] for c in calls]
    assert names[0] == "sy_frames_u8_pack_rows" and names.count("sy_frames_u8_pack_rows") == 1
    assert "sy_frames_u8_pack" not in names and "sy_focus_pack" not in names and "sy_view_copy" not in names


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_uniform_detector_still_packs_with_the_batch_kernel(backend):
    """A detector built without max_frame_hw is the detector it was: FramePairsU8 staging, sy_frames_u8_pack in its launch list
    (and no rows launch), detect_device's three results."""
    model, _ = _models(backend, "fp32")
    det = S.MultiStreamDetector(model, HW, max_streams=2, batch=2, dtype="fp32", device=backend)
    det.warm_up(2)
    assert type(det._in) is FramePairsU8 and det._in.decimate == 2 and tuple(det._stage.shape) == (2,) + HW + (3,)
    with _lib.record() as calls, torch.no_grad():
        det.plan.run_stream_slots(det._in, det.state)
    names = [c[2] for c in calls]
    assert names[0] == "sy_frames_u8_pack" and "sy_frames_u8_pack_rows" not in names
    a = det.open()
    assert len(det.detect_device(_frames(5, HW), [a])) == 3

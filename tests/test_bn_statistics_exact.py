"""The BatchNorm statistics path on INTEGER-VALUED operands: every product, accumulator and partial sum is an integer below 2^24,
so fp32 addition is exact in any order and grouping, and the kernels must equal a float64 reference with ZERO tolerance — on the
emulator and on the GPU, whatever the arrival order of the atomics.

  1. sy_conv2d's statistics epilogue of every forward tile code: per-segment sums / sums of squares, guards around the
     [S][copies][C] arrays, the `+=` contract;
  2. one workgroup per replica row under the training plan's own row formula (train_engine.exact_stat_rows);
  3. fold_rows_kernel / sy_bn_finalize / sy_bn_finalize_apply / sy_bn_running_update over integer rows (fp32-ulp bounds against float64,
     measured against torch's own fp32 BatchNorm);
  4. the backward sums: sy_bn_silu_bwd_reduce under every workgroup cap, sy_bn_silu_bwd_apply (folded and raw-moment rows), and the
     fused SY_EPI_BNR epilogue of the 3x3 data gradient.

A scheme that replaces these sums has to pass this module unchanged."""
import functools
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from streamyolo_amd import ops
from streamyolo_amd.ops import View
from streamyolo_amd.model.packing import pack_conv_weight, pack_conv_weight_frag
from streamyolo_amd.train_engine import exact_stat_rows

DTYPES = ["bf16", "fp16", "fp32"]
SENTINEL = -98765.0            # fill of the guard bands around the statistics arrays (exact in fp32, never a sum of these tests)
LIMIT = float(2 ** 24)         # integers up to here are exact in fp32

# ---- the forward tile codes --------------------------------------------------------------------------------------------------------
IGEMM_TILES = [1, 2, 3, 4, 5, 6, 7, 17, 18, 19, 20, 21, 22, 23, 35, 36, 38, 39, 51, 52, 54, 55, 83, 84, 85, 86, 87, 24, 88, 89, 99, 102, 103]
HALO_S1_TILES = [96, 97, 98, 100, 101, 104, 106, 107, 109, 111, 112, 113, 114, 115, 116, 117, 118]
HALO_S2_TILES = [110, 105]
K1_TILES = [121, 122, 123, 124]

# family = the kernel source; xpad / ypad: the views sit behind that many channels of a wider buffer (ld / channel offsets)
Case = namedtuple("Case", "family tile N cin cout k stride H W xpad ypad")


def _igemm_case(tile, N):            # the shape of test_conv_every_tile_configuration, one and two images
    return Case("igemm", tile, N, 24 if tile < 80 else 32, 264 if tile < 80 else 288, 3, 2, 21, 27, 0, 0)


CASES = [_igemm_case(t, N) for t in IGEMM_TILES for N in (1, 2)]
CASES += [Case("halo", t, 2, 64, 72, 3, 1, 11, 37, 32, 8) for t in HALO_S1_TILES]                       # test_conv3x3_halo_kernel
CASES += [Case("halo_s2", t, N, cin, cout, 3, 2, H, W, 32, 8) for t in HALO_S2_TILES                   # test_conv3x3_stride2_halo_kernel
          for (N, cin, cout, H, W) in [(2, 64, 72, 11, 37), (1, 32, 160, 8, 66), (2, 64, 128, 5, 130)]]
CASES += [Case("k1", t, N, cin, cout, 1, 1, H, W, 8, 16) for t in K1_TILES                              # test_conv1x1_tile_kernel
          for (cin, cout, N, H, W) in [(64, 72, 2, 7, 9), (128, 160, 4, 5, 13), (256, 128, 2, 9, 11), (512, 64, 2, 6, 13),
                                       (1024, 128, 2, 5, 9), (2048, 64, 2, 4, 9)]]

# (tile, dtype, shape) combinations the library refuses BY DESIGN: (tile codes, what, predicate(case, dt), refusing site).  Nothing else is
# left out; test_refused_combinations_are_refused launches each of them and expects SY_ERR_UNSUPPORTED (status 3).
REFUSED = [
    (K1_TILES, "fp32 operands", lambda c, dt: dt == "fp32",
     "csrc/conv1x1_tile.h launch_1x1_tile: `if constexpr (T::kEPC != 8) return SY_ERR_UNSUPPORTED` (16-bit kernel)"),
    ([123], "Cin = 512 (16 slabs) on the 128 ch x 128 px tile", lambda c, dt: c.cin == 512,
     "csrc/conv1x1_tile.h launch_1x1_tile_cfg `case 16`: TC * TP <= 2 or SY_ERR_UNSUPPORTED (weight registers)"),
    ([122, 123], "Cin = 1024 / 2048 (chunked K)", lambda c, dt: c.cin >= 1024,
     "csrc/conv1x1_tile.h launch_1x1_tile_cfg `case 32` / `case 64`: (WC == 4 || TC * TP == 1) && TC * TP <= 2 or SY_ERR_UNSUPPORTED"),
]


def _refusal(case, dt):
    for tiles, what, pred, site in REFUSED:
        if case.tile in tiles and pred(case, dt):
            return "%s: %s" % (what, site)
    return None


def _case_id(c):
    return "%s-t%d-n%d-%dx%d-%dx%d" % (c.family, c.tile, c.N, c.cin, c.cout, c.H, c.W)


def _params(cases):
    out = []
    for c in cases:
        for dt in DTYPES:
            why = _refusal(c, dt)
            out.append(pytest.param(c, dt, id=_case_id(c) + "-" + dt, marks=[pytest.mark.skip(reason=why)] if why else []))
    return out


# ---- operands and references (computed once per shape, shared by every tile / dtype / backend) ---------------------------------------
@functools.lru_cache(maxsize=None)
def _ternary_conv(N, cin, cout, k, stride, H, W):
    """x, w drawn from {-1, 0, 1} (exact in bf16 / fp16 / fp32) and acc = conv2d(x, w) in float64 — with the three conditions that
    make "exact" a theorem asserted by the callers through _assert_exact."""
    g = torch.Generator().manual_seed(N * 7 + cin * 1000 + cout + k * 13 + stride + H * 31 + W)
    x = torch.randint(-1, 2, (N, cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, k, k), generator=g).float()
    acc = F.conv2d(x.double(), w.double(), None, stride, (k - 1) // 2)
    return x, w, acc


def _assert_exact(acc, segs):
    """acc integral; |acc| <= 256 (the stored 16-bit output is exact: bf16 holds integers up to 256); per channel and statistics
    segment sum acc^2 < 2^24 (bounds every partial sum of acc and of acc^2: |a| <= a^2 for integers)."""
    assert torch.equal(acc, acc.round())
    assert float(acc.abs().max()) <= 256.0
    per = acc.shape[0] // segs
    for s in range(segs):
        assert float((acc[s * per:(s + 1) * per] ** 2).sum((0, 2, 3)).max()) < LIMIT


def _guarded(n, guard, dev):
    """n zeroed floats between two guard bands of `guard` sentinel floats: (whole allocation, the n floats)"""
    full = torch.full((n + 2 * guard,), SENTINEL, device=dev)
    body = full[guard:guard + n]
    body.zero_()
    return full, body


def _guards_untouched(full, guard):
    return bool((full[:guard] == SENTINEL).all()) and bool((full[full.numel() - guard:] == SENTINEL).all())


class _StatsLaunch:
    """One training-forward launch of sy_conv2d (raw output + statistics) on a forced tile, into guarded statistics arrays."""

    def __init__(self, dev, case, dt, x, w, segs, copies):
        c = case
        code = ops.dtype_code(dt)
        self.c, self.segs, self.copies = c, segs, copies
        self.Ho, self.Wo = ops.conv_out_size(c.H, c.k, c.stride), ops.conv_out_size(c.W, c.k, c.stride)
        self.xv = View.alloc(c.N, c.H, c.W, c.cin + c.xpad, dt, dev, zero=True).slice(c.xpad, c.cin)
        self.xv.set_nchw(x.to(dev))
        self.yv = View.alloc(c.N, self.Ho, self.Wo, c.cout + c.ypad, dt, dev, zero=True).slice(c.ypad, c.cout)
        self.wp = pack_conv_weight(w, code).to(dev)
        self.wf = pack_conv_weight_frag(self.wp, c.k)
        self.guard = 2 * copies * c.cout
        n = segs * copies * c.cout
        self.sum_all, self.ssum = _guarded(n, self.guard, dev)
        self.sq_all, self.ssq = _guarded(n, self.guard, dev)

    def launch(self):
        c = self.c
        ops.conv2d(self.xv, self.wp, self.yv, c.k, c.stride, stats=(self.ssum, self.ssq), tile=c.tile, wfrag=self.wf, segments=self.segs)

    def rows(self):
        """([segs][copies][Cout] sums, sums of squares) on the host, in float64"""
        shape = (self.segs, self.copies, self.c.cout)
        return self.ssum.view(shape).double().cpu(), self.ssq.view(shape).double().cpu()

    def guards_untouched(self):
        return _guards_untouched(self.sum_all, self.guard) and _guards_untouched(self.sq_all, self.guard)


# ======================================================================================================================================
# 1. convolution-epilogue statistics of every kernel that can produce them
# ======================================================================================================================================
@pytest.mark.parametrize("case,dt", _params(CASES))
def test_conv_epilogue_statistics_are_exact(backend, case, dt):
    """Every forward tile code with `stats`, ternary operands, copies = 4, one statistics segment per half of the batch when N is
    even: the raw output equals conv2d in float64, the replica rows of every segment add up to the float64 per-channel sum and sum
    of squares EXACTLY (a pixel of a ragged tile edge counted twice, dropped, or credited to the other segment changes an integer),
    nothing is written outside [S][copies][C], and a second launch into the same arrays doubles them (`+=`)."""
    c = case
    x, w, acc = _ternary_conv(c.N, c.cin, c.cout, c.k, c.stride, c.H, c.W)
    segs = 2 if c.N % 2 == 0 else 1
    _assert_exact(acc, segs)
    run = _StatsLaunch(backend, c, dt, x, w, segs, copies=4)
    run.launch()
    assert torch.equal(run.yv.nchw().cpu().double(), acc)
    if c.ypad:
        assert float(run.yv.buf[..., :c.ypad].float().abs().max()) == 0.0
    per = c.N // segs
    want_s = torch.stack([acc[s * per:(s + 1) * per].sum((0, 2, 3)) for s in range(segs)])
    want_q = torch.stack([(acc[s * per:(s + 1) * per] ** 2).sum((0, 2, 3)) for s in range(segs)])
    assert torch.equal(want_s.float().double(), want_s) and torch.equal(want_q.float().double(), want_q)     # the fp32 cast is lossless
    rs, rq = run.rows()
    assert torch.equal(rs.sum(1), want_s), "sum: worst channel off by %g" % float((rs.sum(1) - want_s).abs().max())
    assert torch.equal(rq.sum(1), want_q), "sum of squares: worst channel off by %g" % float((rq.sum(1) - want_q).abs().max())
    assert run.guards_untouched()
    run.launch()
    rs2, rq2 = run.rows()
    assert torch.equal(rs2, 2 * rs) and torch.equal(rq2, 2 * rq)
    assert torch.equal(run.yv.nchw().cpu().double(), acc)
    assert run.guards_untouched()


def _refused_params():
    return [p for p in _params(CASES) if p.marks]


@pytest.mark.parametrize("case,dt", [pytest.param(*p.values, id=p.id) for p in _refused_params()])
def test_refused_combinations_are_refused(backend, case, dt):
    """The skip table holds only what the library turns away itself: each entry returns SY_ERR_UNSUPPORTED before any kernel runs."""
    c = case
    x, w, _ = _ternary_conv(c.N, c.cin, c.cout, c.k, c.stride, c.H, c.W)
    run = _StatsLaunch(backend, c, dt, x, w, 1, copies=4)
    assert run.wf is not None
    with pytest.raises(ops._lib.HipLibraryError, match=r"status 3"):
        run.launch()
    assert float(run.ssum.abs().max()) == 0.0 and run.guards_untouched()


# ======================================================================================================================================
# 2. one workgroup per replica row under the plan's own formula
# ======================================================================================================================================
def _ownership_cases():
    out = []
    # the output maps: part 1's shape of the family, a narrow image (W = 5) and one just above the 32-pixel tile (W = 37)
    for t in IGEMM_TILES:
        cin = 24 if t < 80 else 32
        out += [Case("igemm", t, 2, cin, 264 if t < 80 else 288, 3, 2, 21, 27, 0, 0),
                Case("igemm", t, 2, cin, 40, 3, 2, 13, 9, 0, 0),           # -> 7 x 5
                Case("igemm", t, 2, cin, 40, 3, 2, 21, 73, 0, 0)]          # -> 11 x 37
    for t in HALO_S1_TILES:
        out += [Case("halo", t, 2, 64, 72, 3, 1, 11, 37, 32, 8), Case("halo", t, 2, 32, 40, 3, 1, 7, 5, 0, 0),
                Case("halo", t, 4, 32, 40, 3, 1, 6, 70, 0, 0)]
    for t in HALO_S2_TILES:
        out += [Case("halo_s2", t, 2, 64, 72, 3, 2, 11, 37, 32, 8), Case("halo_s2", t, 2, 32, 40, 3, 2, 13, 9, 0, 0),
                Case("halo_s2", t, 2, 32, 40, 3, 2, 21, 73, 0, 0)]
    for t in K1_TILES:
        out += [Case("k1", t, 2, 64, 72, 1, 1, 7, 9, 8, 16), Case("k1", t, 2, 64, 40, 1, 1, 7, 5, 0, 0),
                Case("k1", t, 2, 64, 40, 1, 1, 11, 37, 0, 0)]
    return out


OWNERSHIP_CASES = _ownership_cases()


def _ownership_params():
    out = []
    for c in OWNERSHIP_CASES:
        for dt in (["bf16", "fp32"] if c.family != "k1" else ["bf16", "fp16"]):      # (the 1x1 tile kernel is 16-bit only: REFUSED)
            assert _refusal(c, dt) is None
            out.append(pytest.param(c, dt, id=_case_id(c) + "-" + dt))
    return out


@pytest.mark.parametrize("case,dt", _ownership_params())
def test_every_workgroup_owns_a_replica_row(backend, case, dt):
    """Every output = 1 (x[:, 0] = 1, the centre tap of w[:, 0] = 1: in bounds at every output pixel, stride 1 and 2), so
    ssum[row, c] COUNTS the pixels the row received.  With copies = exact_stat_rows(...) — the training plan's own figure — and with 8x
    that, the non-zero row counts of a segment are the same multiset: a wrap `tile % copies` that merged two workgroups into one row
    would change it, on the emulator as on the GPU and whatever the order of the atomics.  The counts add up to the segment's
    pixels, and every channel of a row reports the same count."""
    c = case
    x = torch.zeros(c.N, c.cin, c.H, c.W)
    x[:, 0] = 1.0
    w = torch.zeros(c.cout, c.cin, c.k, c.k)
    w[:, 0, c.k // 2, c.k // 2] = 1.0
    segs = 2
    counts = []
    for mult in (1, 8):
        Ho, Wo = ops.conv_out_size(c.H, c.k, c.stride), ops.conv_out_size(c.W, c.k, c.stride)
        copies = mult * exact_stat_rows(c.N // segs, Ho, Wo)
        run = _StatsLaunch(backend, c, dt, x, w, segs, copies)
        run.launch()
        assert torch.equal(run.yv.nchw().cpu(), torch.ones(c.N, c.cout, Ho, Wo))
        rs, rq = run.rows()
        assert run.guards_untouched()
        assert torch.equal(rs, rq)                                     # 1 * 1 = 1
        assert torch.equal(rs, rs[:, :, :1].expand_as(rs))             # every channel of a row: the same count
        per_seg = []
        for s in range(segs):
            n = rs[s, :, 0]
            assert float(n.sum()) == (c.N // segs) * Ho * Wo
            per_seg.append(sorted(int(v) for v in n[n != 0].tolist()))
        counts.append(per_seg)
    assert counts[0] == counts[1]


# ======================================================================================================================================
# 3. fold, finalize and running statistics over integer rows
# ======================================================================================================================================
ROW_COUNTS = [1, 31, 32, 33, 64, 65, 777, 4096]       # both sides of kFoldAbove = 64 / kFoldTo = 32, the 8 replica groups, thousands
EPS, MOMENTUM = 1e-3, 0.03


def _ulps(got, ref64):
    """max |got - ref| in units of the fp32 spacing at |ref| (ref in float64)"""
    a = ref64.abs().float()
    a = torch.where(a.double() > ref64.abs(), torch.nextafter(a, torch.zeros_like(a)), a)        # the fp32 number at or below |ref|
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
    return float(((got.double() - ref64).abs() / ulp).max())


@functools.lru_cache(maxsize=None)
def _integer_rows(R, nseg, C):
    """Integer pixels x [nseg][R][3][C] (three pixels per replica row) and their per-row sums / sums of squares.  Every pixel of a channel
    has the sign of the channel's offset (|offset| 3..8, noise -2..2), and beta / the running mean get the opposite / the same sign
    below, so that neither shift = beta - mean * scale nor the running-mean update cancels: an ulp of the RESULT then measures the
    arithmetic, not the conditioning of the data.  Per-channel totals: <= 4096 * 3 * 100 < 2^24."""
    g = torch.Generator().manual_seed(R * 10 + nseg + C)
    off = torch.randint(3, 9, (C,), generator=g) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    x = (torch.randint(-2, 3, (nseg, R, 3, C), generator=g) + off).double()
    gamma = (torch.rand(C, generator=g) + 0.5)
    beta = -(torch.rand(C, generator=g) + 0.5) * off.sign()
    rm0 = (torch.rand(C, generator=g) + 0.1) * off.sign()
    rv0 = torch.rand(C, generator=g) + 0.5
    rows, sq = x.sum(2), (x ** 2).sum(2)
    assert float(sq.sum(1).max()) < LIMIT
    return x, rows.float(), sq.float(), gamma, beta, rm0, rv0


def _finalize_reference(x, gamma, beta):
    """(mean, invstd, scale, shift) [nseg][C] of sy_bn_finalize's formulas in float64, and the same four from torch's own fp32
    BatchNorm on the same pixels (save_mean / save_invstd of the training-mode batch_norm, scale and shift formed from them in fp32)."""
    nseg, C = x.shape[0], x.shape[-1]
    px = x.reshape(nseg, -1, C)
    count = px.shape[1]
    mean = px.sum(1) / count
    var = ((px ** 2).sum(1) / count - mean ** 2).clamp_min(0.0)
    invstd = 1.0 / (var + EPS).sqrt()
    scale = gamma.double() * invstd
    ref = (mean, invstd, scale, beta.double() - mean * scale)
    t_mean, t_inv = [], []
    for s in range(nseg):
        _, m, i = torch.native_batch_norm(px[s].float(), gamma, beta, None, None, True, MOMENTUM, EPS)
        t_mean.append(m); t_inv.append(i)
    t_mean, t_inv = torch.stack(t_mean), torch.stack(t_inv)
    t_scale = gamma * t_inv
    return ref, (t_mean, t_inv, t_scale, beta - t_mean * t_scale), count


@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("R", ROW_COUNTS)
def test_finalize_over_integer_rows(backend, R, nseg):
    """sy_bn_finalize (fold_rows_kernel above 64 rows) over integer replica rows whose per-channel totals stay below 2^24: the fold is
    exact in any order, so mean / invstd / scale / shift differ from a float64 evaluation of the same formulas only by the final
    roundings.  Bound, per quantity, in fp32 ulps of the float64 value: twice what torch's own fp32 batch_norm shows on the same
    pixels, at least 1 ulp.  Measured (max over the 16 cases, emulator):
        ours   mean 0.33  invstd 0.50  scale   1.19  shift  2.03 ulp
        torch  mean 0.33  invstd 119.5  scale 128.2  shift 97.3  ulp   (its fp32 variance cancels on these offset pixels)
    closest case: shift at R = 1, nseg = 2 — ours 1.99 against torch's 1.61 ulp, bound 3.22.
    Two calls over the same rows are bit-equal, and sy_bn_finalize_apply — which adds the rows in another order — equals
    sy_bn_finalize bit for bit at every row count (test_bn_finalize_apply_fused_equals_the_two_launches' definition)."""
    C = 96
    x, rows, sq, gamma, beta, _, _ = _integer_rows(R, nseg, C)
    ref, tref, count = _finalize_reference(x, gamma, beta)
    dev = backend
    gd, bd = gamma.to(dev), beta.to(dev)
    outs = []
    for _ in range(2):
        ssum, ssq = rows.clone().to(dev).reshape(-1), sq.clone().to(dev).reshape(-1)       # (the fold writes into its arrays)
        o = [torch.empty(nseg * C, device=dev) for _ in range(4)]                            # scale, shift, mean, invstd
        ops.bn_finalize(ssum, ssq, count, gd, bd, EPS, MOMENTUM, None, None, *o, nseg=nseg)
        outs.append([t.cpu().view(nseg, C) for t in o])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    scale, shift, mean, invstd = outs[0]
    for name, got, r64, t32 in zip(("mean", "invstd", "scale", "shift"), (mean, invstd, scale, shift), ref, tref):
        ours, torchs = _ulps(got, r64), _ulps(t32, r64)
        print("finalize R=%d nseg=%d %s: ours %.3f ulp, torch fp32 %.3f ulp" % (R, nseg, name, ours, torchs))
        assert ours <= max(1.0, 2.0 * torchs), name
    # the fused launch, over fresh copies of the same rows
    yv = View.alloc(nseg, 1, 4, C, "fp32", dev, zero=True)
    ov = View.alloc(nseg, 1, 4, C, "fp32", dev)
    f = [torch.empty(nseg * C, device=dev) for _ in range(4)]
    ops.bn_finalize_apply(rows.clone().to(dev).reshape(-1), sq.clone().to(dev).reshape(-1), count, gd, bd, EPS, *f, yv, ov, nseg=nseg)
    for a, b in zip(outs[0], f):
        assert torch.equal(a, b.cpu().view(nseg, C))


def test_running_update_over_integer_rows(backend):
    """sy_bn_running_update driven by the same integer rows: one module per row count (1 ... 4096) in ONE launch, two calls per
    module (the two segments' rows, in call order), the rows a channel slice of a wider statistics array (ld > C) whose other columns
    are NaN — they must not reach the result.  Same bound as the finalize test: twice torch's own fp32 error against float64 on
    the same pixels, at least 1 ulp.  Measured (max over the modules, emulator): ours running_mean 1.82 / running_var 2.18 ulp, torch
    fp32 1.82 / 19.2 ulp (the same two fp32 operations per call for the mean: equal figures)."""
    import torch.nn as nn
    dev = backend
    mods, refs = [], []
    for i, R in enumerate(ROW_COUNTS):
        C = 40 if i % 2 else 96
        x, rows, sq, _, _, rm0, rv0 = _integer_rows(R, 2, C)
        c_off, ld = 8, C + 24
        bn = nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM)
        bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
        r32 = nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM).train(); r32.load_state_dict(bn.state_dict())
        r64 = nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM).double().train()
        r64.running_mean.copy_(rm0.double()); r64.running_var.copy_(rv0.double())
        bn = bn.to(dev)
        calls = []
        for s in range(2):
            px = x[s].reshape(-1, C)
            r32(px.float()); r64(px)
            wide_s = torch.full((R, ld), float("nan")); wide_q = torch.full((R, ld), float("nan"))
            wide_s[:, c_off:c_off + C] = rows[s]; wide_q[:, c_off:c_off + C] = sq[s]
            wide_s, wide_q = wide_s.to(dev), wide_q.to(dev)
            calls.append((wide_s.view(-1)[c_off:], wide_q.view(-1)[c_off:], px.shape[0], R, ld))
        mods.append((bn, calls)); refs.append((r32, r64))
    tab = ops.BnRunningTable(mods, dev)
    tab.run()
    for (bn, _), (r32, r64), R in zip(mods, refs, ROW_COUNTS):
        for name in ("running_mean", "running_var"):
            got, t32, want = getattr(bn, name).cpu(), getattr(r32, name), getattr(r64, name)
            assert bool(torch.isfinite(got).all()), "%s R=%d: a NaN column outside the slice was read" % (name, R)
            ours, torchs = _ulps(got, want), _ulps(t32, want)
            print("running update R=%d %s: ours %.3f ulp, torch fp32 %.3f ulp" % (R, name, ours, torchs))
            assert ours <= max(1.0, 2.0 * torchs), "%s R=%d" % (name, R)


# ======================================================================================================================================
# 4. the backward sums
# ======================================================================================================================================
@functools.lru_cache(maxsize=None)
def _bwd_operands(C, nseg):
    """Integer y (|y| <= 6) and EVEN integer da (|da| <= 8) [nseg, C, 13, 37]: with scale = shift = 0, silu'(0) = 1/2 and dz = da / 2 is an
    integer; with mean = 0, invstd = 1, xhat = y."""
    g = torch.Generator().manual_seed(C + nseg)
    y = torch.randint(-6, 7, (nseg, C, 13, 37), generator=g).float()
    da = (torch.randint(-4, 5, (nseg, C, 13, 37), generator=g) * 2).float()
    dz = da.double() * 0.5
    s0, s1 = dz.sum((2, 3)), (dz * y.double()).sum((2, 3))                       # [nseg][C]
    assert torch.equal(dz, dz.round())
    assert float(dz.abs().sum((2, 3)).max()) < LIMIT and float((dz * y.double()).abs().sum((2, 3)).max()) < LIMIT
    return y, da, s0, s1


@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("C", [16, 96, 192])           # 96 / 192: channel slices of 48 / 64 (blockIdx.z)
@pytest.mark.parametrize("dt", DTYPES)
def test_bwd_reduce_is_exact_under_every_workgroup_cap(backend, dt, C, nseg):
    """sy_bn_silu_bwd_reduce on integer operands, copies = the workgroup cap (the exact mode's sizing): the replica rows add up to the
    float64 sum dz and sum dz * xhat exactly — under the default cap and under caps of 1, 3 and 8 workgroups, i.e. the folded result
    does not depend on the cap (include/streamyolo_hip.h, sy_bn_grid_caps)."""
    y, da, s0, s1 = _bwd_operands(C, nseg)
    dev = backend
    yv = View.alloc(nseg, 13, 37, C, dt, dev); yv.set_nchw(y.to(dev))
    dav = View.alloc(nseg, 13, 37, C, dt, dev); dav.set_nchw(da.to(dev))
    zeros, ones = torch.zeros(nseg * C, device=dev), torch.ones(nseg * C, device=dev)
    default = ops.bn_grid_caps()["bwd_reduce"]
    try:
        for cap in (default, 1, 3, 8):
            assert ops.bn_grid_caps(bwd_reduce=cap)["bwd_reduce"] == cap
            guard = 2 * cap * C
            full, sums = _guarded(nseg * cap * 2 * C, guard, dev)
            ops.bn_silu_bwd_reduce(yv, dav, zeros, zeros, zeros, ones, sums, nseg=nseg)
            got = sums.view(nseg, cap, 2, C).double().cpu().sum(1)
            assert torch.equal(got[:, 0], s0) and torch.equal(got[:, 1], s1), "cap %d" % cap
            assert _guards_untouched(full, guard)
    finally:
        ops.bn_grid_caps(bwd_reduce=default)


@pytest.mark.parametrize("copies", [2, 8, 768])         # folded by every workgroup (<= 2) | by fold_replicas_kernel
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_bwd_apply_parameter_gradients_are_the_folded_rows(backend, dt, nseg, copies):
    """sy_bn_silu_bwd_apply fed the reduce pass's own integer rows (768 of them: the exact mode) and two or eight synthetic ones:
    dbeta = S0 and dgamma = S1 exactly, the segments added into the shared parameters."""
    C = 96
    y, da, s0, s1 = _bwd_operands(C, nseg)
    dev = backend
    yv = View.alloc(nseg, 13, 37, C, dt, dev); yv.set_nchw(y.to(dev))
    dav = View.alloc(nseg, 13, 37, C, dt, dev); dav.set_nchw(da.to(dev))
    zeros, ones = torch.zeros(nseg * C, device=dev), torch.ones(nseg * C, device=dev)
    if copies == 768:
        default = ops.bn_grid_caps()["bwd_reduce"]
        try:
            assert ops.bn_grid_caps(bwd_reduce=768)["bwd_reduce"] == 768
            sums = torch.zeros(nseg * copies * 2 * C, device=dev)
            ops.bn_silu_bwd_reduce(yv, dav, zeros, zeros, zeros, ones, sums, nseg=nseg)
        finally:
            ops.bn_grid_caps(bwd_reduce=default)
    else:                                               # the totals spread over the rows as integers: row 0 takes the remainder
        g = torch.Generator().manual_seed(copies)
        part = torch.randint(-50, 51, (nseg, copies, 2, C), generator=g).double()
        part[:, 0] = torch.stack([s0, s1], 1) - part[:, 1:].sum(1)
        assert float(part.abs().sum(1).max()) < LIMIT
        sums = part.float().to(dev).reshape(-1)
    dyv = View.alloc(nseg, 13, 37, C, dt, dev)
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ops.bn_silu_bwd_apply(yv, dav, zeros, zeros, zeros, ones, torch.ones(C, device=dev), sums, dyv, dgam, dbet, nseg=nseg)
    assert torch.equal(dbet.double().cpu(), s0.sum(0)) and torch.equal(dgam.double().cpu(), s1.sum(0))


@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_bwd_apply_raw_moment_rows_equal_centred_rows(backend, dt, nseg):
    """Raw-moment mode (dres_accumulate & 4, the rows a fused SY_EPI_BNR reduce leaves): with an integer mean and a power-of-two invstd
    the conversion invstd * (sum dz*y - mean * sum dz) is exact, so dy / dgamma / dbeta are bit-equal to the run fed the
    already-centred rows (768 rows each: the same fold)."""
    C, copies = 96, 768
    g = torch.Generator().manual_seed(11 + nseg)
    dev = backend
    y = torch.randint(-6, 7, (nseg, C, 13, 37), generator=g).float()
    da = torch.randn(nseg, C, 13, 37, generator=g)
    mean = torch.randint(-3, 4, (nseg, C), generator=g).float()
    invstd = 2.0 ** torch.randint(-2, 2, (nseg, C), generator=g).float()
    gamma = torch.rand(C, generator=g) + 0.5
    scale = (gamma[None] * invstd).reshape(-1)
    shift = (torch.randn(nseg, C, generator=g) * 0.2).reshape(-1)
    raw = torch.randint(-40, 41, (nseg, copies, 2, C), generator=g).double()                  # [.., 0, :] = sum dz, [.., 1, :] = sum dz*y
    cen = raw.clone()
    cen[:, :, 1] = invstd.double()[:, None] * (raw[:, :, 1] - mean.double()[:, None] * raw[:, :, 0])
    assert float(raw.abs().sum(1).max()) < LIMIT and float(cen.abs().sum(1).max()) * 4 < LIMIT   # (x 4: in units of the smallest invstd)
    assert torch.equal(cen.float().double(), cen)
    yv = View.alloc(nseg, 13, 37, C, dt, dev); yv.set_nchw(y.to(dev))
    dav = View.alloc(nseg, 13, 37, C, dt, dev); dav.set_nchw(da.to(dev))
    args = [t.to(dev) for t in (scale, shift, mean.reshape(-1), invstd.reshape(-1), gamma)]
    outs = []
    for rows, raw_moment in ((raw, True), (cen, False)):
        dyv = View.alloc(nseg, 13, 37, C, dt, dev)
        dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        ops.bn_silu_bwd_apply(yv, dav, *args, rows.float().to(dev).reshape(-1), dyv, dgam, dbet, nseg=nseg, raw_moment=raw_moment)
        outs.append((dyv.buf.cpu(), dgam.cpu(), dbet.cpu()))
    assert torch.isfinite(outs[0][0].float()).all()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][1].double(), cen[:, :, 1].sum((0, 1))) and torch.equal(outs[0][2].double(), cen[:, :, 0].sum((0, 1)))


@functools.lru_cache(maxsize=None)
def _bnr_operands():
    N, C, cout, H, W = 2, 64, 96, 9, 37              # the shape of test_dgrad_carries_the_producers_bn_backward_reduce
    g = torch.Generator().manual_seed(98)
    dy = torch.randint(-1, 2, (N, cout, H, W), generator=g).float()
    w = torch.randint(-1, 2, (cout, C, 3, 3), generator=g).float()
    z = torch.randint(-4, 5, (N, C, H, W), generator=g).float()
    acc = F.conv_transpose2d(dy.double(), w.double(), None, 1, 1)                # the data gradient of conv2d(a, w, stride 1, pad 1)
    return dy, w, z, acc


@pytest.mark.parametrize("tile", [98, 100, 101, 104, 109, 117])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_fused_bnr_epilogue_sums_are_exact(backend, tile, dt):
    """SY_EPI_BNR with ternary dy and w, integer z and scale = shift = 0: g = acc / 2, so the fused rows add up to sum acc / 2 and
    sum acc * z / 2 of the float64 data gradient exactly (the comparison with the separate reduce launch sees rounded gradients and
    cannot tell a 1 % error), da = acc exactly, and nothing is written outside [copies][2][C]."""
    dy, w, z, acc = _bnr_operands()
    N, C, H, W = z.shape
    cout, copies = dy.shape[1], 4
    g64 = acc * 0.5
    assert torch.equal(acc, acc.round()) and float(acc.abs().max()) <= 256.0
    assert float(g64.abs().sum((0, 2, 3)).max()) < LIMIT and float((g64 * z.double()).abs().sum((0, 2, 3)).max()) < LIMIT
    dev = backend
    code = ops.dtype_code(dt)
    zv = View.alloc(N, H, W, C, dt, dev); zv.set_nchw(z.to(dev))
    dyp = View.alloc(N, H, W, cout, dt, dev); dyp.set_nchw(dy.to(dev))
    wt = pack_conv_weight(w, code, transpose=True).to(dev)
    wf = pack_conv_weight_frag(wt, 3)
    dav = View.alloc(N, H, W, C, dt, dev)
    guard = 2 * copies * C
    full, sums = _guarded(copies * 2 * C, guard, dev)
    zeros = torch.zeros(C, device=dev)
    ops.conv2d(dyp, wt, dav, 3, 1, mode=ops.CONV_DGRAD, tile=tile, wfrag=wf, bn_reduce=(zv, zeros, zeros, sums))
    assert torch.equal(dav.nchw().cpu().double(), acc)
    got = sums.view(copies, 2, C).double().cpu().sum(0)
    assert torch.equal(got[0], g64.sum((0, 2, 3)))
    assert torch.equal(got[1], (g64 * z.double()).sum((0, 2, 3)))
    assert _guards_untouched(full, guard)

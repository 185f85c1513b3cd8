"""The small BatchNorm kernels on the step's frame chains — fold_rows_kernel, bn_finalize_kernel, the backward folds and the
head of bn_silu_bwd_apply_kernel (idle tail threads, a full s_fold) — against NumPy restatements of their DOCUMENTED order of operations, bit for bit, on real-valued rows
(on integers every order gives the same sum: tests/test_bn_statistics_exact.py covers that side; here the order is the subject).

  1. sy_bn_finalize above kFoldAbove = 64 rows: rows [0, 32) of sum / sqsum after the call are the fixed tree of the comment above
     fold_rows_kernel (class r = the rows r, r + 32, ...; four partial sums over the rows j = q mod 4 of that list, each added in index
     order onto +0.0f in float32; combined ((p0 + p1) + p2) + p3), rows >= 32 are left as they were, and the outputs are the direct
     path's over those 32 rows;
  2. sy_bn_finalize up to 64 rows: eight float32 partials per channel (rows k = rg, rg + 8, ... in order), summed in double in order
     0 ... 7, then the double formulas of bn_finalize_kernel, rounded to float where the kernel rounds;
  3. sy_bn_silu_bwd_apply / _live: dy in the float32 operation order of the kernel, dres written or accumulated, dgamma / dbeta +=
     the folded rows — with integer-valued rows, scale = shift = 0 (silu'(0) = 1/2 exactly) and even integer da, so dz and every
     folded sum is exact whatever the fold order and the restatement needs no model of the sigmoid.

Every array the kernels write lies between two bands of sentinels that must come back untouched.

Bit equality of part 2's outputs on the GPU rests on correctly rounded float64 division and square root in the device library;
the parent build (before the loads of these kernels were reordered) was run through this file on the MI355X and is bit-equal to
the restatement there as well (profiles/r18/README.md), so no comparison is relaxed to 1 ulp."""
import functools

import numpy as np
import pytest
import torch

from streamyolo_amd import ops
from streamyolo_amd.ops import View

f32 = np.float32
SENTINEL = -98765.0
EPS, MOMENTUM = 1e-3, 0.03
GUARD = 64                      # elements; a multiple of the 16-byte chunk in every dtype
FOLD_TO, FOLD_ABOVE = 32, 64    # kFoldTo, kFoldAbove (csrc/train_ops.hip)

FOLDED_COPIES = [65, 66, 95, 96, 97, 128, 129, 577, 2251]       # J = 3 | every remainder of the 16-wide rounds | unequal classes
DIRECT_COPIES = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64]
CHANNELS = [8, 40, 64, 72, 256]                                  # C < 32 | partial 32-channel block | partial 64-channel workgroup


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


class _Guarded:
    """n elements between two bands of GUARD sentinels; `body` is what the kernels are given"""

    def __init__(self, init, dev, dtype=torch.float32):
        init = torch.from_numpy(np.array(init, dtype=f32)).reshape(-1).to(dtype)          # (a copy: the operands are shared)
        self.full = torch.full((init.numel() + 2 * GUARD,), SENTINEL, dtype=dtype)
        self.full[GUARD:GUARD + init.numel()] = init
        self.full = self.full.to(dev)
        self.band = self.full[:GUARD].cpu().clone()
        self.body = self.full[GUARD:GUARD + init.numel()]

    def intact(self):
        f = self.full.cpu()
        return torch.equal(f[:GUARD], self.band) and torch.equal(f[f.numel() - GUARD:], self.band)

    def numpy(self):
        return self.body.cpu().float().numpy().copy()


# ---- restatements ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(copies, C, nseg):
    """Real-valued statistic rows [nseg][copies][C] of four "pixels" each: sum s, sum of squares q >= s^2 / 4 + 0.5 (so the batch
    variance is positive), a per-channel offset so that mean^2 is not small against E[x^2]; gamma, beta, running statistics."""
    rng = np.random.default_rng(copies * 1000 + C * 10 + nseg)
    off = rng.uniform(-2.0, 2.0, C)
    s = (rng.normal(size=(nseg, copies, C)) * 2.0 + 4.0 * off).astype(f32)
    q = (s.astype(np.float64) ** 2 / 4.0 + rng.uniform(0.5, 8.0, (nseg, copies, C))).astype(f32)
    gamma = rng.uniform(0.5, 1.5, C).astype(f32)
    beta = rng.normal(size=C).astype(f32)
    rm, rv = rng.normal(size=C).astype(f32), rng.uniform(0.5, 1.5, C).astype(f32)
    for a in (s, q, gamma, beta, rm, rv):
        a.setflags(write=False)
    return s, q, gamma, beta, rm, rv, 4.0 * copies


def _fold_restated(a):
    """[nseg][copies][C] float32 -> [nseg][32][C]: the tree of the comment above fold_rows_kernel, vectorised over segments and C"""
    nseg, copies, C = a.shape
    out = np.zeros((nseg, FOLD_TO, C), f32)
    for r in range(FOLD_TO):
        J = (copies - r + FOLD_TO - 1) // FOLD_TO
        p = [np.zeros((nseg, C), f32) for _ in range(4)]
        for j in range(J):
            p[j % 4] = p[j % 4] + a[:, r + FOLD_TO * j]
        out[:, r] = ((p[0] + p[1]) + p[2]) + p[3]
    assert out.dtype == f32
    return out


@functools.lru_cache(maxsize=None)
def _folded(copies, C, nseg):
    s, q = _rows(copies, C, nseg)[:2]
    return _fold_restated(s), _fold_restated(q)


def _finalize_restated(s, q, count, gamma, beta, rm, rv):
    """bn_finalize_kernel over the rows s, q [nseg][copies][C]: (scale, shift, mean, invstd) [nseg][C], (running_mean, running_var)
    of segment 0"""
    nseg, copies, C = s.shape
    ds, dq = np.zeros((nseg, C)), np.zeros((nseg, C))
    for rg in range(8):
        ps, pq = np.zeros((nseg, C), f32), np.zeros((nseg, C), f32)
        for k in range(rg, copies, 8):
            ps = ps + s[:, k]
            pq = pq + q[:, k]
        ds = ds + ps.astype(np.float64)
        dq = dq + pq.astype(np.float64)
    mean = ds / count
    var = np.maximum(dq / count - mean * mean, 0.0)
    invstd = (1.0 / np.sqrt(var + np.float64(f32(EPS)))).astype(f32)
    mean32 = mean.astype(f32)
    scale = gamma[None] * invstd
    shift = beta[None] - mean32 * scale
    unbiased = (var * count / (count - 1.0) if count > 1.0 else var).astype(f32)
    mom = f32(MOMENTUM)
    new_rm = (f32(1.0) - mom) * rm + mom * mean32[0]
    new_rv = (f32(1.0) - mom) * rv + mom * unbiased[0]
    for a in (scale, shift, new_rm, new_rv):
        assert a.dtype == f32
    return (scale, shift, mean32, invstd), (new_rm, new_rv)


def _pointer_combinations(nseg):
    """(mean / invstd given, running statistics given); the library takes running statistics with one segment only"""
    return [(mi, run) for mi in (True, False) for run in ((True, False) if nseg == 1 else (False,))]


def _run_finalize(dev, copies, C, nseg, with_mi, with_run):
    s, q, gamma, beta, rm, rv, count = _rows(copies, C, nseg)
    gs, gq = _Guarded(s, dev), _Guarded(q, dev)
    outs = [_Guarded(np.full(nseg * C, 7.0, f32), dev) for _ in range(4)]          # scale, shift, mean, invstd
    grm, grv = _Guarded(rm, dev), _Guarded(rv, dev)
    gg, gb = _Guarded(gamma, dev), _Guarded(beta, dev)
    ops.bn_finalize(gs.body, gq.body, count, gg.body, gb.body, EPS, MOMENTUM, grm.body if with_run else None,
                    grv.body if with_run else None, outs[0].body, outs[1].body, outs[2].body if with_mi else None,
                    outs[3].body if with_mi else None, nseg=nseg)
    for g in [gs, gq, grm, grv, gg, gb] + outs:
        assert g.intact()
    assert _same_bits(gg.numpy(), gamma) and _same_bits(gb.numpy(), beta)
    return gs.numpy().reshape(s.shape), gq.numpy().reshape(q.shape), [o.numpy().reshape(nseg, C) for o in outs], grm.numpy(), grv.numpy()


def _check_outputs(outs, got_rm, got_rv, want, want_run, rm, rv, with_mi, with_run, what):
    for name, got, ref, given in zip(("scale", "shift", "mean", "invstd"), outs, want, (True, True, with_mi, with_mi)):
        if given:
            assert _same_bits(got, ref), "%s %s: %d of %d elements differ, worst by %g" % (
                what, name, int((_bits(got) != _bits(ref)).sum()), ref.size, float(np.abs(got - ref).max()))
        else:
            assert np.all(got == f32(7.0)), "%s %s: written through a null pointer's neighbour" % (what, name)
    if with_run:
        assert _same_bits(got_rm, want_run[0]) and _same_bits(got_rv, want_run[1]), what + " running statistics"
    else:
        assert _same_bits(got_rm, rm) and _same_bits(got_rv, rv), what + " running statistics touched"


# ======================================================================================================================================
# 1. above kFoldAbove rows: the fold's tree, then the finalize over the 32 folded rows
# ======================================================================================================================================
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("copies", FOLDED_COPIES)
def test_finalize_folded_rows_are_the_documented_tree(backend, copies, C, nseg):
    """Rows [0, 32) of sum / sqsum after sy_bn_finalize are bit-equal to the restated tree, rows >= 32 keep their bits, nothing
    outside the arrays is written, and scale / shift / mean / invstd / running statistics are the direct path's over the 32 folded
    rows (segments `copies` rows apart) — for every combination of mean / invstd and running statistics given or null."""
    assert copies > FOLD_ABOVE
    s, q, gamma, beta, rm, rv, count = _rows(copies, C, nseg)
    fs, fq = _folded(copies, C, nseg)
    want, want_run = _finalize_restated(fs, fq, count, gamma, beta, rm, rv)
    for with_mi, with_run in _pointer_combinations(nseg):
        what = "copies=%d C=%d nseg=%d mean/invstd=%s running=%s:" % (copies, C, nseg, with_mi, with_run)
        got_s, got_q, outs, got_rm, got_rv = _run_finalize(backend, copies, C, nseg, with_mi, with_run)
        assert _same_bits(got_s[:, :FOLD_TO], fs), what + " folded sum rows"
        assert _same_bits(got_q[:, :FOLD_TO], fq), what + " folded sqsum rows"
        assert _same_bits(got_s[:, FOLD_TO:], s[:, FOLD_TO:]) and _same_bits(got_q[:, FOLD_TO:], q[:, FOLD_TO:]), what + " rows >= 32 written"
        _check_outputs(outs, got_rm, got_rv, want, want_run, rm, rv, with_mi, with_run, what)


# ======================================================================================================================================
# 2. up to kFoldAbove rows: the direct path
# ======================================================================================================================================
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("copies", DIRECT_COPIES)
def test_finalize_direct_path_is_the_documented_order(backend, copies, C, nseg):
    """scale / shift / mean / invstd / running statistics bit-equal to the restatement (per-rg float32 partials, a double sum in
    order, the kernel's double formulas rounded to float as the kernel rounds); the statistic rows are read-only on this path."""
    assert copies <= FOLD_ABOVE
    s, q, gamma, beta, rm, rv, count = _rows(copies, C, nseg)
    want, want_run = _finalize_restated(s, q, count, gamma, beta, rm, rv)
    for with_mi, with_run in _pointer_combinations(nseg):
        what = "copies=%d C=%d nseg=%d mean/invstd=%s running=%s:" % (copies, C, nseg, with_mi, with_run)
        got_s, got_q, outs, got_rm, got_rv = _run_finalize(backend, copies, C, nseg, with_mi, with_run)
        assert _same_bits(got_s, s) and _same_bits(got_q, q), what + " statistic rows written"
        _check_outputs(outs, got_rm, got_rv, want, want_run, rm, rv, with_mi, with_run, what)


# ======================================================================================================================================
# 3. the backward apply pass
# ======================================================================================================================================
# (rows allocated per segment, rows written since the clear or None = sy_bn_silu_bwd_apply): one row | folded by every workgroup |
# fold_replicas_kernel | one live row (no fold launch) | fold_replicas_live_kernel, short and across a 16-row round
FOLDS = [(1, None), (2, None), (8, None), (8, 1), (8, 3), (40, 37)]


@functools.lru_cache(maxsize=None)
def _bwd_operands(C, pixels, nseg):
    rng = np.random.default_rng(C * 100 + pixels * 3 + nseg)
    y = rng.integers(-6, 7, (nseg, pixels, C)).astype(f32)
    da = (rng.integers(-4, 5, (nseg, pixels, C)) * 2).astype(f32)
    prev = rng.integers(-9, 10, (nseg, pixels, C)).astype(f32)              # what dres holds before an accumulating call
    mean = rng.integers(-3, 4, (nseg, C)).astype(f32)
    invstd = (2.0 ** rng.integers(-2, 2, (nseg, C))).astype(f32)
    gamma = rng.uniform(0.5, 1.5, C).astype(f32)
    rows = {}
    for copies, live in FOLDS:
        r = rng.integers(-50, 51, (nseg, copies, 2, C)).astype(f32)
        if live is not None:
            r[:, live:] = 0.0                                               # never written since the clear: +0.0f
        rows[(copies, live)] = r
    dg0, db0 = rng.integers(-20, 21, C).astype(f32), rng.integers(-20, 21, C).astype(f32)
    return y, da, prev, mean, invstd, gamma, rows, dg0, db0


def _bwd_restated(y, da, mean, invstd, gamma, rows, pixels):
    """dy [nseg][pixels][C] in the kernel's float32 order — gi * ((dz - m0) - ((y - mean) * invstd) * m1), dz = da / 2 — and the
    folded totals [nseg][2][C] (integers below 2^24: exact in any order)"""
    tot = rows.astype(np.float64).sum(1)
    assert float(np.abs(rows).astype(np.float64).sum(1).max()) < 2.0 ** 24
    fold = tot.astype(f32)
    inv_m = f32(1.0) / f32(pixels)
    m0, m1 = fold[:, 0] * inv_m, fold[:, 1] * inv_m
    gi = gamma[None] * invstd
    dz = da * f32(0.5)
    dy = gi[:, None] * ((dz - m0[:, None]) - ((y - mean[:, None]) * invstd[:, None]) * m1[:, None])
    assert dy.dtype == f32
    return dy, tot


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("pixels", [1, 5, 257])
@pytest.mark.parametrize("C", [8, 24, 72, 256, 1024])       # 24: an idle tail thread per workgroup (bf16) | 1024: s_fold full
def test_bwd_apply_is_the_documented_formula(backend, C, pixels, nseg, dt):
    """sy_bn_silu_bwd_apply / _live over every fold route (FOLDS), without dres, with dres as first write and with `+=`: dy is
    bit-equal to the float32 restatement rounded to the storage type, dres = da (or da + what it held: small integers, exact),
    dgamma / dbeta grow by the folded totals of all segments exactly, and the guard bands around dy, dres, dgamma and dbeta stay as
    they were."""
    y, da, prev, mean, invstd, gamma, all_rows, dg0, db0 = _bwd_operands(C, pixels, nseg)
    dev = backend
    tdt = ops.TORCH_DTYPE[ops.dtype_code(dt)]

    def view(g):
        return View(g.body.view(nseg, 1, pixels, C), nseg, 1, pixels, C)

    yv, dav = view(_Guarded(y, dev, tdt)), view(_Guarded(da, dev, tdt))
    zeros = torch.zeros(nseg * C, device=dev)
    md, isd, gd = (torch.from_numpy(a.copy()).reshape(-1).to(dev) for a in (mean, invstd, gamma))
    for (copies, live), rows in all_rows.items():
        want_dy, tot = _bwd_restated(y, da, mean, invstd, gamma, rows, pixels)
        want_dy = torch.from_numpy(want_dy).to(tdt).float().numpy()
        for mode in ("none", "write", "accumulate"):
            what = "C=%d pixels=%d nseg=%d %s copies=%d live=%s dres=%s:" % (C, pixels, nseg, dt, copies, live, mode)
            gdy = _Guarded(np.full(y.shape, 3.0, f32), dev, tdt)
            gdr = _Guarded(prev, dev, tdt)
            gdg, gdb = _Guarded(dg0, dev), _Guarded(db0, dev)
            sums = torch.from_numpy(rows.copy()).reshape(-1).to(dev)            # (a fold launch writes into its rows)
            ops.bn_silu_bwd_apply(yv, dav, zeros, zeros, md, isd, gd, sums, view(gdy), gdg.body, gdb.body, nseg=nseg,
                                  dres=None if mode == "none" else view(gdr), dres_accumulate=mode == "accumulate", live=live)
            for g in (gdy, gdr, gdg, gdb):
                assert g.intact(), what + " guard band"
            assert _same_bits(gdy.numpy().reshape(y.shape), want_dy), what + " dy: worst off by %g" % float(
                np.abs(gdy.numpy().reshape(y.shape) - want_dy).max())
            want_res = {"none": prev, "write": da, "accumulate": da + prev}[mode]
            assert _same_bits(gdr.numpy().reshape(y.shape), want_res), what + " dres"
            assert np.array_equal(gdb.numpy().astype(np.float64), db0 + tot[:, 0].sum(0)), what + " dbeta"
            assert np.array_equal(gdg.numpy().astype(np.float64), dg0 + tot[:, 1].sum(0)), what + " dgamma"

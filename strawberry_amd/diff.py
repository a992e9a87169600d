"""Differential isoform usage: did the isoform usage of a locus change between two samples?  Each sample is solved, both are
solved under one shared theta (the pooled problem, its columns scaled so that the shared theta is the joint maximum-likelihood
one), and the likelihoods are compared (include/sbgpu.h states the rule).

em_diff_host       the three host calls around a solver the caller brings (the library has no CPU EM)
em_diff_device     sbgpu_em_diff_device: built in HBM for two batches of one annotation
model_diff_device  sbgpu_model_diff_device: from what two resident calls kept for the bootstrap on two contexts of one device
                   (ChainQuantifier / FrontQuantifier(keep_bootstrap=True).differential_usage(other))
model_diff_merged_device  sbgpu_model_diff_merged_device: the same two retained samples on ONE bin table, the union of their bins by
                   key (differential_usage(other, shared_bins=True); merge.py)

All return a DifferentialUsage.  The per-isoform arrays are laid out as theta is.

model_diff_device tests each sample on the bins it observed, so part of a reported difference is that difference of conditioning
(the CAVEAT of include/sbgpu.h's differential-usage block); model_diff_merged_device removes it for bins a sample did not observe.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

NAMES = _lib.sbgpu_em_diff_t._NAMES
PER_ISO = ("theta_a", "theta_b", "theta_pooled", "usage_a", "usage_b", "usage_pooled", "delta_usage")
FLOAT64 = PER_ISO + ("lr_stat", "loglik_a", "loglik_b", "loglik_a_pooled", "loglik_b_pooled")
INT64 = ("n_a", "n_b", "lost_shift")
DTYPES = {k: np.float64 if k in FLOAT64 else np.int64 if k in INT64 else np.int32 for k in NAMES}
LIMIT_NAMES = ("max_kept", "max_pooled_bins", "tile_vals", "tile_rows", "group_max_kept", "threads", "grid_per_cu", "default_bytes")
OK, EMPTY, SOLE, TOO_WIDE, TOO_DEEP, ONE_SAMPLE, UNSOLVED = range(7)
STATUS_NAMES = ("OK", "EMPTY", "SOLE", "TOO_WIDE", "TOO_DEEP", "ONE_SAMPLE", "UNSOLVED")
KIND_A, KIND_B, KIND_POOLED = range(3)


def limits():
    """The thresholds (csrc/diff_rules.h, csrc/diff_device.h) by name: see sbgpu_em_diff_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_em_diff_limits(out), "sbgpu_em_diff_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def params(max_bytes=0):
    """max_bytes: the device scratch one chunk of sub-problems may take (0: 1 GiB)"""
    return _lib.sbgpu_diff_params_t(int(max_bytes), 0)


def _gamma_q(a, x):
    """The regularised upper incomplete gamma function Q(a, x), a > 0, x >= 0: the series of P below x < a + 1, Lentz's
    continued fraction of Q beyond (both to 1e-16 relative or 500 terms)."""
    if x <= 0.0:
        return 1.0
    if math.isinf(x):
        return 0.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        for n in range(1, 500):
            term *= x / (a + n)
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return min(1.0, max(0.0, 1.0 - total * lead))
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for n in range(1, 500):
        an = -n * (n - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        step = d * c
        h *= step
        if abs(step - 1.0) < 1e-16:
            break
    return min(1.0, max(0.0, lead * h))


def chi2_sf(x, dof):
    """The survival function of chi-squared with dof >= 1 degrees of freedom at x (max(x, 0) is taken)."""
    return _gamma_q(0.5 * dof, 0.5 * max(float(x), 0.0))


class DifferentialUsage(Results):
    """theta_a, theta_b, theta_pooled, usage_a, usage_b, usage_pooled, delta_usage (float64) [n_iso]; lr_stat, loglik_a, loglik_b,
    loglik_a_pooled, loglik_b_pooled (float64), n_a, n_b, lost_shift (int64), dof, diff_status, top_iso, status_a, status_b,
    status_pooled, iters_a, iters_b, iters_pooled (int32) [n_loci].
    want: the names to bring to the host (None: all) -- the device forms copy nothing else over PCIe; the others are None.
    .device: name -> device address of the context's copy (device forms; valid until its next quantify / diff call)."""
    STRUCT = _lib.sbgpu_em_diff_t

    def __init__(self, iso_off, want=None):
        self.iso_off = np.ascontiguousarray(iso_off, np.int64)
        self.n_loci, self.n_iso = len(self.iso_off) - 1, int(self.iso_off[-1])
        self._arrays({k: (self.n_iso if k in PER_ISO else self.n_loci, DTYPES[k]) for k in NAMES}, want)

    def p_value(self):
        """Per locus: the chi-squared survival function with dof degrees of freedom at max(lr_stat, 0); NaN where lost_shift != 0
        (the statistic does not compare like with like) or the status is neither OK nor SOLE; 1.0 for SOLE."""
        p = np.full(self.n_loci, np.nan)
        for l in range(self.n_loci):
            st = int(self.diff_status[l])
            if st == SOLE:
                p[l] = 1.0
            elif st == OK and int(self.lost_shift[l]) == 0 and int(self.dof[l]) >= 1:
                p[l] = chi2_sf(self.lr_stat[l], int(self.dof[l]))
        return p

    def significant(self, alpha=0.05):
        """The loci whose p-value is below alpha, ascending (a NaN is never significant)."""
        p = self.p_value()
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(p < alpha)

    def rows(self, names=None):
        """-> (locus, status, lr_stat, dof, p_value, n_a, n_b, lost_shift, top_iso, top delta_usage, loglik_a, loglik_b, loglik_a_pooled,
        loglik_b_pooled) per locus, for a TSV: the locus as its index, or -- names = locus names -- by name; top_iso locus-local."""
        p = self.p_value()
        for l in range(self.n_loci):
            top = int(self.top_iso[l])
            yield (names[l] if names else l, STATUS_NAMES[int(self.diff_status[l])], float(self.lr_stat[l]), int(self.dof[l]), float(p[l]),
                   int(self.n_a[l]), int(self.n_b[l]), int(self.lost_shift[l]), top,
                   float(self.delta_usage[int(self.iso_off[l]) + top]) if top >= 0 else 0.0, float(self.loglik_a[l]), float(self.loglik_b[l]),
                   float(self.loglik_a_pooled[l]), float(self.loglik_b_pooled[l]))


def _offsets(batch_a, batch_b, who):
    ra, rb = np.ascontiguousarray(batch_a.row_off, np.int64), np.ascontiguousarray(batch_b.row_off, np.int64)
    ia, ib = np.ascontiguousarray(batch_a.iso_off, np.int64), np.ascontiguousarray(batch_b.iso_off, np.int64)
    if ia.size < 1 or ra.size != ia.size or rb.size != ib.size:
        raise ValueError("%s: row_off and iso_off hold n_loci + 1 entries" % who)
    if ia.size != ib.size or (ia != ib).any():
        raise _lib.SbgpuError("%s: the two batches differ in n_loci or iso_off: they are not over one annotation" % who)
    return ra, rb, ia


def shapes_host(row_off_a, row_off_b, iso_off, keep_a=None, keep_b=None):
    """Rules 1 and 2 -> dict: diff_status [n_loci] (before the solves); sub_locus, sub_kind [n_sub]; row_off, iso_off, f_off
    [n_sub + 1] of the sub-batch."""
    L = _lib.load()
    row_off_a, row_off_b, iso_off = (np.ascontiguousarray(a, np.int64) for a in (row_off_a, row_off_b, iso_off))
    keep_a, keep_b = as_array(keep_a, np.int32), as_array(keep_b, np.int32)
    if row_off_a.size != iso_off.size or row_off_b.size != iso_off.size or iso_off.size < 1:
        raise ValueError("shapes_host: row_off_a, row_off_b and iso_off hold n_loci + 1 entries")
    n_loci = iso_off.size - 1
    check_lengths("shapes_host", ("keep_a", keep_a, int(iso_off[-1])), ("keep_b", keep_b, int(iso_off[-1])))
    sizes = (C.c_int64 * 4)()
    args = (n_loci, row_off_a.ctypes.data, row_off_b.ctypes.data, iso_off.ctypes.data, ptr(keep_a), ptr(keep_b), sizes)
    _lib.check(L.sbgpu_em_diff_shapes_host(*args, *([None] * 6)), "sbgpu_em_diff_shapes_host")
    n_sub = int(sizes[0])
    out = dict(diff_status=np.zeros(max(n_loci, 1), np.int32), sub_locus=np.zeros(max(n_sub, 1), np.int32), sub_kind=np.zeros(max(n_sub, 1), np.int32),
               row_off=np.zeros(n_sub + 1, np.int64), iso_off=np.zeros(n_sub + 1, np.int64), f_off=np.zeros(n_sub + 1, np.int64))
    _lib.check(L.sbgpu_em_diff_shapes_host(*args, *(out[k].ctypes.data for k in ("diff_status", "sub_locus", "sub_kind", "row_off", "iso_off", "f_off"))),
               "sbgpu_em_diff_shapes_host")
    out["diff_status"], out["sub_locus"], out["sub_kind"] = out["diff_status"][:n_loci], out["sub_locus"][:n_sub], out["sub_kind"][:n_sub]
    return out


def _batch_struct(batch, who, weights=True):
    """-> (sbgpu_batch_t, the arrays it points into)"""
    row_off, iso_off, f_off = (np.ascontiguousarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    count = np.ascontiguousarray(batch.count, np.int32)
    F = np.ascontiguousarray(batch.F, np.float64) if weights else None
    check_lengths(who, ("count", count, int(row_off[-1])), ("F", F, int(f_off[-1])))
    return _lib.sbgpu_batch_t(len(row_off) - 1, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, ptr(count), ptr(F)), (row_off, iso_off, f_off, count, F)


def expand_host(batch_a, batch_b, keep_a=None, keep_b=None, shapes=None):
    """The sub-batch's (count, F) for two batches (row_off, iso_off, f_off, count, F each) and their keeps; shapes: shapes_host's, or None."""
    L = _lib.load()
    ra, rb, iso_off = _offsets(batch_a, batch_b, "expand_host")
    keep_a, keep_b = as_array(keep_a, np.int32), as_array(keep_b, np.int32)
    check_lengths("expand_host", ("keep_a", keep_a, int(iso_off[-1])), ("keep_b", keep_b, int(iso_off[-1])))
    sh = shapes or shapes_host(ra, rb, iso_off, keep_a, keep_b)
    sub_count, sub_F = np.zeros(max(int(sh["row_off"][-1]), 1), np.int32), np.zeros(max(int(sh["f_off"][-1]), 1), np.float64)
    (a, hold_a), (b, hold_b) = _batch_struct(batch_a, "expand_host"), _batch_struct(batch_b, "expand_host")
    _lib.check(L.sbgpu_em_diff_expand_host(C.byref(a), C.byref(b), ptr(keep_a), ptr(keep_b), sub_count.ctypes.data, sub_F.ctypes.data),
               "sbgpu_em_diff_expand_host")
    del hold_a, hold_b
    return sub_count[:int(sh["row_off"][-1])], sub_F[:int(sh["f_off"][-1])]


def cross_inputs(sub_iso_off, theta, status):
    """The cross fit's (theta, status) for a sub-batch of triples A, B, POOLED: the pooled sub-problem's onto its siblings."""
    sub_iso_off = np.asarray(sub_iso_off, np.int64)
    x_theta, x_status = np.array(theta, np.float64), np.array(status, np.int32)
    for q in range(0, len(sub_iso_off) - 1, 3):
        p0, p1 = int(sub_iso_off[q + 2]), int(sub_iso_off[q + 3])
        for k in (0, 1):
            x_theta[int(sub_iso_off[q + k]):int(sub_iso_off[q + k + 1])] = theta[p0:p1]
            x_status[q + k] = status[q + 2]
    return x_theta, x_status


def em_diff_host(batch_a, batch_b, keep_a, keep_b, solve, want=None):
    """batch_a, batch_b: row_off, iso_off, f_off, count, F (synth.LocusBatch) over one annotation; keep_a, keep_b [n_iso] or None;
    solve: a callable (row_off, iso_off, f_off, count, F) -> (theta, status, iters) that solves a batch as sbgpu_em_run_device
    does.  The sub-batch is made (shapes, expansion), solved by `solve`, fitted twice by sbgpu_em_fit_host with nothing erased
    (own; A and B at the pooled theta), and reduced to the statistics."""
    from . import fit as _fit
    L = _lib.load()
    keep_a, keep_b = as_array(keep_a, np.int32), as_array(keep_b, np.int32)
    ra, rb, iso_off = _offsets(batch_a, batch_b, "em_diff_host")
    sh = shapes_host(ra, rb, iso_off, keep_a, keep_b)
    sub_count, sub_F = expand_host(batch_a, batch_b, keep_a, keep_b, sh)
    n_sub = len(sh["sub_locus"])
    theta, status, iters = solve(sh["row_off"], sh["iso_off"], sh["f_off"], sub_count, sub_F)
    theta, status, iters = np.ascontiguousarray(theta, np.float64), np.ascontiguousarray(status, np.int32), np.ascontiguousarray(iters, np.int32)
    check_lengths("em_diff_host", ("theta", theta, int(sh["iso_off"][-1])), ("status", status, n_sub), ("iters", iters, n_sub))
    x_theta, x_status = cross_inputs(sh["iso_off"], theta, status)

    class _Sub:
        row_off, iso_off, f_off, count, F = sh["row_off"], sh["iso_off"], sh["f_off"], sub_count, sub_F
    fits = [_fit.em_fit_host(_Sub, t if t.size else np.zeros(1), None, s if n_sub else None, want=("loglik", "n_live", "n_dropped", "n_impossible"))
            for t, s in ((theta, status), (x_theta, x_status))]
    own, cross = fits
    t = DifferentialUsage(iso_off, want)
    s = t._struct()
    (a, hold_a), (b, hold_b) = _batch_struct(batch_a, "em_diff_host", False), _batch_struct(batch_b, "em_diff_host", False)
    _lib.check(L.sbgpu_em_diff_stat_host(C.byref(a), C.byref(b), ptr(keep_a), ptr(keep_b), ptr(theta), ptr(status), ptr(iters), ptr(own.loglik),
                                         ptr(own.n_live), ptr(own.n_dropped), ptr(own.n_impossible), ptr(cross.loglik), ptr(cross.n_dropped),
                                         ptr(cross.n_impossible), C.byref(s)), "sbgpu_em_diff_stat_host")
    del hold_a, hold_b
    t.sub = dict(sh, count=sub_count, F=sub_F, theta=theta, status=status, iters=iters, fit=own, cross=cross)
    return t._finish(s)


def _keep_host(keep, d_keep):
    """keep on the host, for the shapes of with_sub_batch: given, or read back from a tensor"""
    if keep is not None or d_keep is None:
        return keep
    if not hasattr(d_keep, "cpu"):
        raise ValueError("diff: d_keep is a device address: give keep (the same values on the host) too")
    return d_keep.cpu().numpy()


def em_diff_device(ctx, plan_a, d_count_a, d_F_a, plan_b, d_count_b, d_F_b, d_keep_a=None, d_keep_b=None, keep_a=None, keep_b=None, max_bytes=0,
                   stream=None, want=None, with_sub_batch=False):
    """plan_a, plan_b: em.Plan of the two batches; d_count_* (int32), d_F_* (float64), d_keep_* (int32): torch tensors on the
    context's device, or device addresses; max_bytes: the scratch budget of one chunk (0: 1 GiB); with_sub_batch: the expanded
    sub-batch comes back too, as .sub = dict(shapes_host's arrays, count, F) -- for a caller that checks the expansion (keep_*:
    the keeps on the host, where d_keep_* are addresses)."""
    check_tensors("em_diff_device", d_count_a=(d_count_a, "torch.int32"), d_F_a=(d_F_a, "torch.float64"), d_keep_a=(d_keep_a, "torch.int32"),
                  d_count_b=(d_count_b, "torch.int32"), d_F_b=(d_F_b, "torch.float64"), d_keep_b=(d_keep_b, "torch.int32"))
    t = DifferentialUsage(plan_a.iso_off, want)
    s, p = t._struct(), params(max_bytes)
    if with_sub_batch:
        _offsets(plan_a, plan_b, "em_diff_device")
        sh = shapes_host(plan_a.row_off, plan_b.row_off, plan_a.iso_off, _keep_host(keep_a, d_keep_a), _keep_host(keep_b, d_keep_b))
        sub_count, sub_F = np.zeros(int(sh["row_off"][-1]) + 1, np.int32), np.zeros(int(sh["f_off"][-1]) + 1)
        s.sub_count, s.sub_F = sub_count.ctypes.data, sub_F.ctypes.data
        t.sub = dict(sh, count=sub_count[:-1], F=sub_F[:-1])
    _lib.check(ctx.L.sbgpu_em_diff_device(ctx.h, plan_a.h, addr(d_count_a), addr(d_F_a), plan_b.h, addr(d_count_b), addr(d_F_b), addr(d_keep_a),
                                          addr(d_keep_b), C.byref(p), stream, C.byref(s)), "sbgpu_em_diff_device")
    return t._finish(s)


def model_diff_device(ctx_a, handle_a, ctx_b, handle_b, d_keep_a=None, d_keep_b=None, keep_a=None, keep_b=None, max_bytes=0, stream=None, want=None,
                      with_sub_batch=False):
    """Right after two resident calls made with bootstrap_keep on, on their handles, before either context's next quantify call:
    sample A is ctx_a's, sample B ctx_b's (contexts of one device).  d_keep_*: each call's keep (int32 tensor or device
    address), or None: everything kept.  The work and the results' device copies are ctx_a's.  with_sub_batch: as em_diff_device's
    (keep_*: the keeps on the host, where d_keep_* are addresses)."""
    L = ctx_a.L
    handle_a, handle_b = getattr(handle_a, "h", handle_a), getattr(handle_b, "h", handle_b)
    if handle_a is None or handle_b is None:
        raise _lib.SbgpuError("model_diff_device: null argument (a handle is None)")
    check_tensors("model_diff_device", d_keep_a=(d_keep_a, "torch.int32"), d_keep_b=(d_keep_b, "torch.int32"))
    n_loci = bins_info(L, handle_a)[0]
    row_off, iso_off = np.zeros(n_loci + 1, np.int64), np.zeros(n_loci + 1, np.int64)
    _lib.check(L.sbgpu_bins_export(handle_a, row_off.ctypes.data, iso_off.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
    t = DifferentialUsage(iso_off, want)
    s, p = t._struct(), params(max_bytes)
    if with_sub_batch:
        row_off_b, iso_off_b = np.zeros(bins_info(L, handle_b)[0] + 1, np.int64), np.zeros(bins_info(L, handle_b)[0] + 1, np.int64)
        _lib.check(L.sbgpu_bins_export(handle_b, row_off_b.ctypes.data, iso_off_b.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
        sh = shapes_host(row_off, row_off_b, iso_off, _keep_host(keep_a, d_keep_a), _keep_host(keep_b, d_keep_b))
        sub_count, sub_F = np.zeros(int(sh["row_off"][-1]) + 1, np.int32), np.zeros(int(sh["f_off"][-1]) + 1)
        s.sub_count, s.sub_F = sub_count.ctypes.data, sub_F.ctypes.data
        t.sub = dict(sh, count=sub_count[:-1], F=sub_F[:-1])
    _lib.check(L.sbgpu_model_diff_device(ctx_a.h, handle_a, ctx_b.h, handle_b, addr(d_keep_a), addr(d_keep_b), C.byref(p), stream, C.byref(s)),
               "sbgpu_model_diff_device")
    return t._finish(s)


def model_diff_merged_device(ctx_a, handle_a, ctx_b, handle_b, d_keep_a=None, d_keep_b=None, max_bytes=0, stream=None, want=None, merged_want=(),
                             merge_only=False):
    """As model_diff_device, on ONE bin table for both samples: the union of their bins by key, zero counts where a sample saw
    nothing, a missing bin's weights from the other sample's bin under this sample's insert-size law (sbgpu_model_diff_merged_device;
    DESIGN 3.29).  Needs handles whose bins were grouped on the device.  The result carries the merge.MergedBins as .merged:
    offsets, device addresses, and on the host the arrays merged_want names (None: all).  merge_only: no test -- the MergedBins
    alone is returned (and the context's stage times are the merge's)."""
    from . import merge as _merge
    L = ctx_a.L
    handle_a, handle_b = getattr(handle_a, "h", handle_a), getattr(handle_b, "h", handle_b)
    if handle_a is None or handle_b is None:
        raise _lib.SbgpuError("model_diff_merged_device: null argument (a handle is None)")
    check_tensors("model_diff_merged_device", d_keep_a=(d_keep_a, "torch.int32"), d_keep_b=(d_keep_b, "torch.int32"))
    n_loci = bins_info(L, handle_a)[0]
    row_off, iso_off = np.zeros(n_loci + 1, np.int64), np.zeros(n_loci + 1, np.int64)
    _lib.check(L.sbgpu_bins_export(handle_a, row_off.ctypes.data, iso_off.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
    t, m = DifferentialUsage(iso_off, want), _merge.MergedBins(iso_off, merged_want)
    s, ms, p = t._struct(), m._struct(), params(max_bytes)
    _lib.check(L.sbgpu_model_diff_merged_device(ctx_a.h, handle_a, ctx_b.h, handle_b, addr(d_keep_a), addr(d_keep_b), C.byref(p), stream,
                                                None if merge_only else C.byref(s), C.byref(ms)), "sbgpu_model_diff_merged_device")
    m.fetch(ctx_a, ms, stream)
    if merge_only:
        return m
    t.merged = m
    return t._finish(s)

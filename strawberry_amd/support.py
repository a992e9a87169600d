"""Isoform support: do the fragments of a locus need this isoform, or do its neighbours explain them as well?  Every kept
isoform of a locus of 2..64 kept isoforms is dropped in turn, the locus is solved again, and the two likelihoods are compared
(include/sbgpu.h states the rule).

em_loo_host       the three host calls around a solver the caller brings (the library has no CPU EM)
em_loo_device     sbgpu_em_loo_device: built in HBM for a batch an em.EmBatchSolver holds (EmBatchSolver.run_loo())
model_loo_device  sbgpu_model_loo_device: from what a resident call kept for the bootstrap (sbgpu_bootstrap_keep;
                  quantify_resident(with_support=True), ChainQuantifier / FrontQuantifier(...).isoform_support())

All return an IsoformSupport.  The per-isoform arrays are laid out as theta is; theta_without is packed by without_off.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

NAMES = tuple(n for n in _lib.sbgpu_em_loo_t._NAMES if n not in ("theta_without", "without_off"))
PER_ISO = ("lr_stat", "heir_gain", "theta_refit", "n_unique", "heir", "status_without", "iters_without", "support")
PER_LOCUS = ("loglik_base", "loo_status", "status_base", "iters_base")
DTYPES = dict({k: np.int32 for k in NAMES}, lr_stat=np.float64, heir_gain=np.float64, theta_refit=np.float64, n_unique=np.int64,
              loglik_base=np.float64, theta_without=np.float64)
LIMIT_NAMES = ("max_kept", "tile_vals", "tile_rows", "threads", "grid_per_cu", "default_bytes", "max_bins", "max_iso")
NOT_KEPT, TESTED, SOLE, LOCUS_SKIPPED = range(4)
SUPPORT_NAMES = ("NOT_KEPT", "TESTED", "SOLE", "LOCUS_SKIPPED")
OK, EMPTY, TOO_WIDE = range(3)
STATUS_NAMES = ("OK", "EMPTY", "TOO_WIDE")


def limits():
    """The thresholds (csrc/loo_rules.h, csrc/loo_device.h) by name: see sbgpu_em_loo_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_em_loo_limits(out), "sbgpu_em_loo_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def offsets(iso_off, keep=None):
    """without_off [n_iso + 1] of the packed theta_without for a batch's iso_off and keep (sbgpu_em_loo_offsets)."""
    iso_off, keep = np.ascontiguousarray(iso_off, np.int64), as_array(keep, np.int32)
    if iso_off.ndim != 1 or iso_off.size < 1:
        raise ValueError("offsets: iso_off holds n_loci + 1 entries")
    check_lengths("offsets", ("keep", keep, int(iso_off[-1])))
    out = np.zeros(int(max(iso_off[-1], 0)) + 1, np.int64)
    _lib.check(_lib.load().sbgpu_em_loo_offsets(iso_off.ctypes.data, ptr(keep), iso_off.size - 1, out.ctypes.data), "sbgpu_em_loo_offsets")
    return out


def params(max_bytes=0):
    """max_bytes: the device scratch one chunk of sub-problems may take (0: 1 GiB)"""
    return _lib.sbgpu_loo_params_t(int(max_bytes), 0)


class IsoformSupport(Results):
    """lr_stat, heir_gain, theta_refit (float64), n_unique (int64), heir, status_without, iters_without, support (int32) [n_iso];
    loglik_base (float64), loo_status, status_base, iters_base (int32) [n_loci]; without (float64) [without_off[-1]]: theta_without,
    packed (want: "theta_without"; theta_without(l, j) reads it).
    want: the names to bring to the host (None: all) -- the device forms copy nothing else over PCIe; the others are None.
    iso_off, keep: the batch's (keep None: everything kept), for the packed offsets and the per-locus views.
    .device: name -> device address of the context's copy (device forms; valid until its next quantify / support call)."""
    STRUCT = _lib.sbgpu_em_loo_t

    def __init__(self, iso_off, keep=None, want=None):
        self.iso_off = np.ascontiguousarray(iso_off, np.int64)
        self.n_loci, self.n_iso = len(self.iso_off) - 1, int(self.iso_off[-1])
        self.keep = as_array(keep, np.int32)
        self.without_off = offsets(self.iso_off, self.keep)
        # (the packed array is .without: theta_without is the per-isoform view below)
        packed = want is None or "theta_without" in want
        self.without = np.zeros(max(int(self.without_off[-1]), 1)) if packed else None
        self._arrays({k: (self.n_iso if k in PER_ISO else self.n_loci, DTYPES[k]) for k in NAMES},
                     None if want is None else [k for k in want if k != "theta_without"])

    def _struct(self):
        s = super()._struct()
        s.theta_without = None if self.without is None else self.without.ctypes.data
        s.without_off = self.without_off.ctypes.data
        return s

    def _finish(self, s):
        super()._finish(s)
        if self.without is not None:
            self.without = self.without[:int(self.without_off[-1])]
        if s.d_theta_without:
            self.device["theta_without"] = int(s.d_theta_without)
        if s.d_without_off:
            self.device["without_off"] = int(s.d_without_off)
        return self

    def theta_without(self, l, j):
        """theta of locus l solved without its isoform j (locus-local), over all of the locus' isoforms: 0 for j itself and
        for an isoform that is not kept; None where j was not TESTED."""
        i0, i1 = int(self.iso_off[l]), int(self.iso_off[l + 1])
        w0, w1 = int(self.without_off[i0 + j]), int(self.without_off[i0 + j + 1])
        if w1 == w0 or self.without is None:
            return None
        packed = self.without
        kept = np.ones(i1 - i0, bool) if self.keep is None else self.keep[i0:i1] != 0
        kept[j] = False
        out = np.zeros(i1 - i0)
        out[kept] = packed[w0:w1]
        return out

    def p_value(self):
        """Per isoform, under the boundary mixture 1/2 chi2_0 + 1/2 chi2_1 (the null theta_j = 0 lies on the edge of the
        parameter space): 0.5 * erfc(sqrt(max(stat, 0) / 2)); 0 for +inf, 1 for a statistic <= 0 -- also for the isoforms that
        were not tested, whose statistic is 0."""
        stat = np.maximum(np.nan_to_num(self.lr_stat, nan=0.0, posinf=np.inf), 0.0)
        p = np.array([0.0 if math.isinf(x) else 0.5 * math.erfc(math.sqrt(x / 2.0)) for x in stat])
        p[stat <= 0.0] = 1.0
        return p

    def rows(self, names=None):
        """-> (locus, isoform, support, lr_stat, p_value, n_unique, heir, heir_gain, theta_refit, status_without, iters_without) per
        isoform, for a TSV: the locus as its index, or -- names = locus names -- by name; the isoform and its heir locus-local."""
        p = self.p_value()
        for l in range(self.n_loci):
            for i in range(int(self.iso_off[l]), int(self.iso_off[l + 1])):
                yield (names[l] if names else l, i - int(self.iso_off[l]), SUPPORT_NAMES[int(self.support[i])], float(self.lr_stat[i]), float(p[i]),
                       int(self.n_unique[i]), int(self.heir[i]), float(self.heir_gain[i]), float(self.theta_refit[i]), int(self.status_without[i]),
                       int(self.iters_without[i]))


def shapes_host(row_off, iso_off, keep=None):
    """Rules 1 and 2 -> dict: loo_status [n_loci]; sub_locus, sub_drop [n_sub]; row_off, iso_off, f_off [n_sub + 1] of the sub-batch."""
    L = _lib.load()
    row_off, iso_off, keep = np.ascontiguousarray(row_off, np.int64), np.ascontiguousarray(iso_off, np.int64), as_array(keep, np.int32)
    if row_off.size != iso_off.size or iso_off.size < 1:
        raise ValueError("shapes_host: row_off and iso_off hold n_loci + 1 entries")
    n_loci = iso_off.size - 1
    check_lengths("shapes_host", ("keep", keep, int(iso_off[-1])))
    sizes = (C.c_int64 * 4)()
    args = (n_loci, row_off.ctypes.data, iso_off.ctypes.data, ptr(keep), sizes)
    _lib.check(L.sbgpu_em_loo_shapes_host(*args, *([None] * 6)), "sbgpu_em_loo_shapes_host")
    n_sub = int(sizes[0])
    out = dict(loo_status=np.zeros(max(n_loci, 1), np.int32), sub_locus=np.zeros(max(n_sub, 1), np.int32), sub_drop=np.zeros(max(n_sub, 1), np.int32),
               row_off=np.zeros(n_sub + 1, np.int64), iso_off=np.zeros(n_sub + 1, np.int64), f_off=np.zeros(n_sub + 1, np.int64))
    _lib.check(L.sbgpu_em_loo_shapes_host(*args, *(out[k].ctypes.data for k in ("loo_status", "sub_locus", "sub_drop", "row_off", "iso_off", "f_off"))),
               "sbgpu_em_loo_shapes_host")
    out["loo_status"], out["sub_locus"], out["sub_drop"] = out["loo_status"][:n_loci], out["sub_locus"][:n_sub], out["sub_drop"][:n_sub]
    return out


def expand_host(batch, keep=None, shapes=None):
    """The sub-batch's (count, F) for a batch (row_off, iso_off, f_off, count, F) and keep; shapes: shapes_host's, or None."""
    L = _lib.load()
    row_off, iso_off, f_off = (np.ascontiguousarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    count, F, keep = np.ascontiguousarray(batch.count, np.int32), np.ascontiguousarray(batch.F, np.float64), as_array(keep, np.int32)
    check_lengths("expand_host", ("keep", keep, int(iso_off[-1])), ("count", count, int(row_off[-1])), ("F", F, int(f_off[-1])))
    sh = shapes or shapes_host(row_off, iso_off, keep)
    sub_count, sub_F = np.zeros(max(int(sh["row_off"][-1]), 1), np.int32), np.zeros(max(int(sh["f_off"][-1]), 1), np.float64)
    b = _lib.sbgpu_batch_t(len(row_off) - 1, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, ptr(count), ptr(F))
    _lib.check(L.sbgpu_em_loo_expand_host(C.byref(b), ptr(keep), sub_count.ctypes.data, sub_F.ctypes.data), "sbgpu_em_loo_expand_host")
    return sub_count[:int(sh["row_off"][-1])], sub_F[:int(sh["f_off"][-1])]


def em_loo_host(batch, keep, solve, want=None):
    """batch: row_off, iso_off, f_off, count, F (synth.LocusBatch); keep [n_iso] or None; solve: a callable
    (row_off, iso_off, f_off, count, F) -> (theta, status, iters) that solves a batch as sbgpu_em_run_device does.  The sub-batch
    is made (shapes, expansion), solved by `solve`, fitted by sbgpu_em_fit_host with nothing erased, and reduced to the statistics."""
    from . import fit as _fit
    L = _lib.load()
    keep = as_array(keep, np.int32)
    iso_off = np.ascontiguousarray(batch.iso_off, np.int64)
    sh = shapes_host(batch.row_off, iso_off, keep)
    sub_count, sub_F = expand_host(batch, keep, sh)
    n_sub = len(sh["sub_locus"])
    theta, status, iters = solve(sh["row_off"], sh["iso_off"], sh["f_off"], sub_count, sub_F)
    theta, status, iters = np.ascontiguousarray(theta, np.float64), np.ascontiguousarray(status, np.int32), np.ascontiguousarray(iters, np.int32)
    check_lengths("em_loo_host", ("theta", theta, int(sh["iso_off"][-1])), ("status", status, n_sub), ("iters", iters, n_sub))

    class _Sub:
        row_off, iso_off, f_off, count, F = sh["row_off"], sh["iso_off"], sh["f_off"], sub_count, sub_F
    f = _fit.em_fit_host(_Sub, theta if theta.size else np.zeros(1), None, status if n_sub else None,
                         want=("loglik", "n_live", "n_dropped", "n_impossible"))
    t = IsoformSupport(iso_off, keep, want)
    s = t._struct()
    _lib.check(L.sbgpu_em_loo_stat_host(t.n_loci, iso_off.ctypes.data, ptr(keep), ptr(theta), ptr(status), ptr(iters), ptr(f.loglik),
                                        ptr(f.n_live), ptr(f.n_dropped), ptr(f.n_impossible), C.byref(s)), "sbgpu_em_loo_stat_host")
    t.sub = dict(sh, count=sub_count, F=sub_F, theta=theta, status=status, iters=iters, fit=f)
    return t._finish(s)


def _keep_host(keep, d_keep):
    """keep on the host, for the packed offsets: given, or read back from a tensor"""
    if keep is not None or d_keep is None:
        return keep
    if not hasattr(d_keep, "cpu"):
        raise ValueError("support: d_keep is a device address: give keep (the same values on the host) too, for the packed offsets")
    return d_keep.cpu().numpy()


def em_loo_device(ctx, plan, d_count, d_F, d_keep=None, keep=None, max_bytes=0, stream=None, want=None, with_sub_batch=False):
    """plan: an em.Plan; d_count (int32), d_F (float64), d_keep (int32): torch tensors on the context's device, or device
    addresses (then keep: the same on the host); max_bytes: the scratch budget of one chunk (0: 1 GiB); with_sub_batch: the
    expanded sub-batch comes back too, as .sub = dict(shapes_host's arrays, count, F) -- for a caller that checks the expansion."""
    check_tensors("em_loo_device", d_count=(d_count, "torch.int32"), d_F=(d_F, "torch.float64"), d_keep=(d_keep, "torch.int32"))
    t = IsoformSupport(plan.iso_off, _keep_host(keep, d_keep), want)
    s, p = t._struct(), params(max_bytes)
    if with_sub_batch:
        sh = shapes_host(plan.row_off, plan.iso_off, t.keep)
        sub_count, sub_F = np.zeros(int(sh["row_off"][-1]) + 1, np.int32), np.zeros(int(sh["f_off"][-1]) + 1)
        s.sub_count, s.sub_F = sub_count.ctypes.data, sub_F.ctypes.data
        t.sub = dict(sh, count=sub_count[:-1], F=sub_F[:-1])
    _lib.check(ctx.L.sbgpu_em_loo_device(ctx.h, plan.h, addr(d_count), addr(d_F), addr(d_keep), C.byref(p), stream, C.byref(s)), "sbgpu_em_loo_device")
    return t._finish(s)


def model_loo_device(ctx, handle, d_keep=None, keep=None, max_bytes=0, stream=None, want=None):
    """Right after a resident call made with bootstrap_keep on, on its handle, before the context's next quantify call.
    d_keep: the call's (int32 tensor or device address, then keep too), or None: everything kept."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    check_tensors("model_loo_device", d_keep=(d_keep, "torch.int32"))
    n_loci = bins_info(L, handle)[0]
    row_off, iso_off = np.zeros(n_loci + 1, np.int64), np.zeros(n_loci + 1, np.int64)
    _lib.check(L.sbgpu_bins_export(handle, row_off.ctypes.data, iso_off.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
    t = IsoformSupport(iso_off, _keep_host(keep, d_keep), want)
    s, p = t._struct(), params(max_bytes)
    _lib.check(L.sbgpu_model_loo_device(ctx.h, handle, addr(d_keep), C.byref(p), stream, C.byref(s)), "sbgpu_model_loo_device")
    return t._finish(s)

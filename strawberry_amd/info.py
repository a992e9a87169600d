"""Isoform information: which isoforms of a locus the counted bins can tell apart, which are confounded with which, and the
analytic covariance of theta -- from the observed information matrix of the locus' mixture, in one pass where a bootstrap costs
one EM solve per replicate (include/sbgpu.h states the rule).

em_info_host       sbgpu_em_info_host: the plain CPU statement, on a batch (synth.LocusBatch, or anything with its five arrays)
em_info_device     sbgpu_em_info_device: built in HBM for a batch an em.EmBatchSolver holds (EmBatchSolver.run_info())
model_info_device  sbgpu_model_info_device: from what a resident call kept for the bootstrap (sbgpu_bootstrap_keep;
                   quantify_resident(with_info=True), ChainQuantifier / FrontQuantifier(...).isoform_information())

All return an IsoformInfo.  se, partner_corr, ident, alias_of, partner are laid out as theta is; cov is packed by cov_off.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

NAMES = tuple(n for n in _lib.sbgpu_em_info_t._NAMES if n != "cov_off")
PER_ISO, PER_LOCUS = ("se", "partner_corr", "ident", "alias_of", "partner"), ("min_pivot", "rank", "n_free", "info_status")
DTYPES = dict({k: np.int32 for k in NAMES}, se=np.float64, partner_corr=np.float64, min_pivot=np.float64, cov=np.float64)
LIMIT_NAMES = ("max_free", "wave_vals", "wave_iso", "stage_vals", "wave_loci", "grid_per_cu", "max_bins", "max_iso")
IDENTIFIED, ALIASED, UNOBSERVED, NOT_FREE, SKIPPED = range(5)
IDENT_NAMES = ("IDENTIFIED", "ALIASED", "UNOBSERVED", "NOT_FREE", "SKIPPED")
OK, EMPTY, TOO_WIDE = range(3)
STATUS_NAMES = ("OK", "EMPTY", "TOO_WIDE")
PIVOT_EPS = 1e-9


def limits():
    """The thresholds (csrc/info_rules.h, csrc/info_device.h) by name: see sbgpu_em_info_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_em_info_limits(out), "sbgpu_em_info_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def cov_offsets(iso_off):
    """cov_off [n_loci + 1] of the packed covariance for a batch's iso_off (sbgpu_em_info_cov_offsets)."""
    iso_off = np.ascontiguousarray(iso_off, np.int64)
    if iso_off.ndim != 1 or iso_off.size < 1:
        raise ValueError("cov_offsets: iso_off holds n_loci + 1 entries")
    out = np.zeros(iso_off.size, np.int64)
    _lib.check(_lib.load().sbgpu_em_info_cov_offsets(iso_off.ctypes.data, iso_off.size - 1, out.ctypes.data), "sbgpu_em_info_cov_offsets")
    return out


class IsoformInfo(Results):
    """se, partner_corr (float64), ident, alias_of, partner (int32) [n_iso]; min_pivot (float64), rank, n_free, info_status
    (int32) [n_loci]; cov (float64) [cov_off[-1]], packed by locus.  want: the names to bring to the host (None: all) -- the
    device forms copy nothing else over PCIe; the others are None.  iso_off: the batch's, for the per-locus views.
    .device: name -> device address of the context's copy (device forms; valid until its next quantify / info call)."""
    STRUCT = _lib.sbgpu_em_info_t

    def __init__(self, iso_off, want=None):
        self.iso_off = np.ascontiguousarray(iso_off, np.int64)
        self.n_loci, self.n_iso = len(self.iso_off) - 1, int(self.iso_off[-1])
        self.cov_off = cov_offsets(self.iso_off)
        self._arrays({k: (self.n_iso if k in PER_ISO else self.n_loci if k in PER_LOCUS else int(self.cov_off[-1]), DTYPES[k]) for k in NAMES}, want)

    def _struct(self):
        s = super()._struct()
        s.cov_off = self.cov_off.ctypes.data
        return s

    def _finish(self, s):
        super()._finish(s)
        if s.d_cov_off:
            self.device["cov_off"] = int(s.d_cov_off)
        return self

    def covariance(self, l):
        """cov of locus l as a dense symmetric [niso, niso] array (zero rows for isoforms outside R); None where the locus has
        more isoforms than limits()["max_free"] (it has no packed block)."""
        niso = int(self.iso_off[l + 1] - self.iso_off[l])
        if self.cov_off[l + 1] - self.cov_off[l] != niso * (niso + 1) // 2:
            return None
        out = np.zeros((niso, niso))
        out[np.triu_indices(niso)] = self.cov[self.cov_off[l]:self.cov_off[l + 1]]
        return out + np.triu(out, 1).T

    def correlation(self, l):
        """cov_jk / (se_j se_k) of locus l, dense; 0 where either se is 0, 1 on the diagonal of an isoform with se > 0"""
        cov = self.covariance(l)
        if cov is None:
            return None
        se = self.se[self.iso_off[l]:self.iso_off[l + 1]]
        d = np.outer(se, se)
        return np.divide(cov, d, out=np.zeros_like(cov), where=d > 0)

    def cv(self, theta):
        """se / theta where theta > 0, NaN elsewhere"""
        theta = np.asarray(theta, np.float64)[:self.n_iso]
        return np.divide(self.se, theta, out=np.full(self.n_iso, np.nan), where=theta > 0)

    def rows(self, names=None, theta=None):
        """-> (locus, isoform, ident, se, alias_of, partner, partner_corr[, theta, cv]) per isoform, for a TSV: the locus as its
        index, or -- names = locus names -- by name; the isoform, alias_of and partner as locus-local indices."""
        cv = None if theta is None else self.cv(theta)
        for l in range(self.n_loci):
            for i in range(int(self.iso_off[l]), int(self.iso_off[l + 1])):
                row = (names[l] if names else l, i - int(self.iso_off[l]), IDENT_NAMES[int(self.ident[i])], float(self.se[i]), int(self.alias_of[i]),
                       int(self.partner[i]), float(self.partner_corr[i]))
                yield row if cv is None else row + (float(theta[i]), float(cv[i]))


def em_info_host(batch, theta, keep=None, status=None, want=None):
    """batch: row_off, iso_off, f_off, count, F (synth.LocusBatch); theta [n_iso]; keep [n_iso] / status [n_loci] or None."""
    L = _lib.load()
    row_off, iso_off, f_off = (np.ascontiguousarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    count, F = np.ascontiguousarray(batch.count, np.int32), np.ascontiguousarray(batch.F, np.float64)
    theta, keep, status = as_array(theta, np.float64), as_array(keep, np.int32), as_array(status, np.int32)
    t = IsoformInfo(iso_off, want)
    check_lengths("em_info_host", ("theta", theta, t.n_iso), ("keep", keep, t.n_iso), ("status", status, t.n_loci),
                  ("count", count, int(row_off[-1])), ("F", F, int(f_off[-1])))
    b = _lib.sbgpu_batch_t(t.n_loci, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, ptr(count), ptr(F))
    s = t._struct()
    _lib.check(L.sbgpu_em_info_host(C.byref(b), theta.ctypes.data if theta is not None else None, ptr(keep), ptr(status), C.byref(s)),
               "sbgpu_em_info_host")
    return t._finish(s)


def em_info_device(ctx, plan, d_count, d_F, d_theta, d_keep=None, d_status=None, stream=None, want=None):
    """plan: an em.Plan; d_count (int32), d_F, d_theta (float64), d_keep, d_status (int32): torch tensors on the context's
    device, or device addresses; d_theta: the EM's, or any other estimate (a bootstrap mean)."""
    check_tensors("em_info_device", d_count=(d_count, "torch.int32"), d_F=(d_F, "torch.float64"), d_theta=(d_theta, "torch.float64"),
                  d_keep=(d_keep, "torch.int32"), d_status=(d_status, "torch.int32"))
    t = IsoformInfo(plan.iso_off, want)
    s = t._struct()
    _lib.check(ctx.L.sbgpu_em_info_device(ctx.h, plan.h, addr(d_count), addr(d_F), addr(d_theta), addr(d_keep), addr(d_status), stream,
                                          C.byref(s)), "sbgpu_em_info_device")
    return t._finish(s)


def model_info_device(ctx, handle, d_theta, d_keep=None, d_status=None, stream=None, want=None):
    """Right after a resident call made with bootstrap_keep on, on its handle, before the context's next quantify call.
    d_theta: a float64 torch tensor on the context's device, or a device address ([n_iso]; the call's own d_theta, or a bootstrap
    mean); d_keep / d_status: the call's (int32), or None: everything kept / every locus started."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    check_tensors("model_info_device", d_theta=(d_theta, "torch.float64"), d_keep=(d_keep, "torch.int32"), d_status=(d_status, "torch.int32"))
    n_loci = bins_info(L, handle)[0]
    row_off, iso_off = np.zeros(n_loci + 1, np.int64), np.zeros(n_loci + 1, np.int64)
    _lib.check(L.sbgpu_bins_export(handle, row_off.ctypes.data, iso_off.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
    t = IsoformInfo(iso_off, want)
    s = t._struct()
    _lib.check(L.sbgpu_model_info_device(ctx.h, handle, addr(d_theta), addr(d_keep), addr(d_status), stream, C.byref(s)),
               "sbgpu_model_info_device")
    return t._finish(s)

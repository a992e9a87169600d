"""Model fit: how well theta explains every locus' bin counts, and how converged theta is -- expected counts and Pearson
residuals per bin, the EM's score per isoform, likelihood, deviance, Pearson statistic, degrees of freedom, fragment counts and
the worst bin per locus (include/sbgpu.h states the rule).

em_fit_host       sbgpu_em_fit_host: the plain CPU statement, on a batch (synth.LocusBatch, or anything with its five arrays)
em_fit_device     sbgpu_em_fit_device: built in HBM for a batch an em.EmBatchSolver holds (EmBatchSolver.run_fit())
model_fit_device  sbgpu_model_fit_device: from what a resident call kept for the bootstrap (sbgpu_bootstrap_keep;
                  quantify_resident(with_fit=True), ChainQuantifier / FrontQuantifier(...).model_fit())

All return a ModelFit.  expected / resid are laid out as the batch's count is, score as theta is.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

NAMES = _lib.sbgpu_em_fit_t._NAMES
PER_BIN, PER_ISO = ("expected", "resid"), ("score",)
DTYPES = dict({k: np.float64 for k in NAMES}, n_live=np.int64, n_dropped=np.int64, n_impossible=np.int64, dof=np.int32, worst_bin=np.int32)
LIMIT_NAMES = ("wave_vals", "stage_vals", "wave_loci", "grid_per_cu", "threads", "wave", "max_bins", "max_iso")


def limits():
    """The device form's thresholds (csrc/fit_device.h) by name: see sbgpu_em_fit_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_em_fit_limits(out), "sbgpu_em_fit_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


class ModelFit(Results):
    """expected, resid [n_bins]; score [n_iso]; loglik, deviance, pearson (float64), n_live, n_dropped, n_impossible (int64), dof,
    worst_bin (int32) [n_loci].  want: the names to bring to the host (None: all) -- the device forms copy nothing else over
    PCIe; the others are None.  row_off / iso_off: the batch's, for the per-locus views.
    .device: name -> device address of the context's copy (device forms; valid until its next quantify / fit call)."""
    STRUCT = _lib.sbgpu_em_fit_t

    def __init__(self, row_off, iso_off, want=None):
        self.row_off, self.iso_off = np.asarray(row_off, np.int64), np.asarray(iso_off, np.int64)
        self.n_loci, self.n_bins, self.n_iso = len(self.row_off) - 1, int(self.row_off[-1]), int(self.iso_off[-1])
        self._arrays({k: (self.n_bins if k in PER_BIN else self.n_iso if k in PER_ISO else self.n_loci, DTYPES[k]) for k in NAMES}, want)

    def reduced_chi2(self):
        """pearson / dof where dof > 0, NaN elsewhere"""
        dof = self.dof.astype(np.float64)
        return np.divide(self.pearson, dof, out=np.full(self.n_loci, np.nan), where=dof > 0)

    def step_norm(self, theta):
        """per locus || theta o score - theta ||_2: how far theta stands from its own next EM iterate, in read counts (the
        reference stops below SBGPU_EM_THETA_CHANGE_LIMIT)"""
        theta = np.asarray(theta, np.float64)[:self.n_iso]
        sq = np.concatenate([(theta * self.score - theta) ** 2, [0.0]])
        out = np.zeros(self.n_loci)
        for l in range(self.n_loci):
            out[l] = np.sqrt(sq[self.iso_off[l]:self.iso_off[l + 1]].sum())
        return out

    def rows(self, names=None, theta=None):
        """-> (locus, n_live, n_dropped, n_impossible, loglik, deviance, pearson, dof, reduced chi2, worst_bin[, step norm]) per
        locus, for a TSV: the locus as its index, or -- names = locus names -- by name; the step norm where theta is given."""
        chi2 = self.reduced_chi2()
        step = None if theta is None else self.step_norm(theta)
        for l in range(self.n_loci):
            row = (names[l] if names else l, int(self.n_live[l]), int(self.n_dropped[l]), int(self.n_impossible[l]), float(self.loglik[l]),
                   float(self.deviance[l]), float(self.pearson[l]), int(self.dof[l]), float(chi2[l]), int(self.worst_bin[l]))
            yield row if step is None else row + (float(step[l]),)


def em_fit_host(batch, theta, keep=None, status=None, want=None):
    """batch: row_off, iso_off, f_off, count, F (synth.LocusBatch); theta [n_iso]; keep [n_iso] / status [n_loci] or None."""
    L = _lib.load()
    row_off, iso_off, f_off = (np.ascontiguousarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    count, F = np.ascontiguousarray(batch.count, np.int32), np.ascontiguousarray(batch.F, np.float64)
    theta, keep, status = as_array(theta, np.float64), as_array(keep, np.int32), as_array(status, np.int32)
    t = ModelFit(row_off, iso_off, want)
    check_lengths("em_fit_host", ("theta", theta, t.n_iso), ("keep", keep, t.n_iso), ("status", status, t.n_loci), ("count", count, t.n_bins),
                  ("F", F, int(f_off[-1])))
    b = _lib.sbgpu_batch_t(t.n_loci, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, ptr(count), ptr(F))
    s = t._struct()
    _lib.check(L.sbgpu_em_fit_host(C.byref(b), theta.ctypes.data if theta is not None else None, ptr(keep), ptr(status), C.byref(s)),
               "sbgpu_em_fit_host")
    return t._finish(s)


def em_fit_device(ctx, plan, d_count, d_F, d_theta, d_keep=None, d_status=None, stream=None, want=None):
    """plan: an em.Plan; d_count (int32), d_F, d_theta (float64), d_keep, d_status (int32): torch tensors on the context's
    device, or device addresses; d_theta: the EM's, or any other estimate (a bootstrap mean)."""
    check_tensors("em_fit_device", d_count=(d_count, "torch.int32"), d_F=(d_F, "torch.float64"), d_theta=(d_theta, "torch.float64"),
                   d_keep=(d_keep, "torch.int32"), d_status=(d_status, "torch.int32"))
    t = ModelFit(plan.row_off, plan.iso_off, want)
    s = t._struct()
    _lib.check(ctx.L.sbgpu_em_fit_device(ctx.h, plan.h, addr(d_count), addr(d_F), addr(d_theta), addr(d_keep), addr(d_status), stream,
                                         C.byref(s)), "sbgpu_em_fit_device")
    return t._finish(s)


def model_fit_device(ctx, handle, d_theta, d_keep=None, d_status=None, stream=None, want=None):
    """Right after a resident call made with bootstrap_keep on, on its handle, before the context's next quantify call.
    d_theta: a float64 torch tensor on the context's device, or a device address ([n_iso]; the call's own d_theta, or a bootstrap
    mean); d_keep / d_status: the call's (int32), or None: everything kept / every locus started."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    check_tensors("model_fit_device", d_theta=(d_theta, "torch.float64"), d_keep=(d_keep, "torch.int32"), d_status=(d_status, "torch.int32"))
    n_loci = bins_info(L, handle)[0]
    row_off, iso_off = np.zeros(n_loci + 1, np.int64), np.zeros(n_loci + 1, np.int64)
    _lib.check(L.sbgpu_bins_export(handle, row_off.ctypes.data, iso_off.ctypes.data, *([None] * 11)), "sbgpu_bins_export")
    t = ModelFit(row_off, iso_off, want)
    s = t._struct()
    _lib.check(L.sbgpu_model_fit_device(ctx.h, handle, addr(d_theta), addr(d_keep), addr(d_status), stream, C.byref(s)),
               "sbgpu_model_fit_device")
    return t._finish(s)

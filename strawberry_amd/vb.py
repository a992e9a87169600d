"""Variational Bayes solve: a Dirichlet(alpha) prior on the isoform shares of every locus -- the posterior's counts, shares and
their spread per isoform, status, iterations and the evidence bound (ELBO) per locus (include/sbgpu.h states the rule; DESIGN
3.31).  A second solver beside the EM: with alpha < 1 it empties the isoforms the data do not need.

em_vb_host       sbgpu_em_vb_host: the plain CPU statement, on a batch (synth.LocusBatch, or anything with its five arrays)
em_vb_device     sbgpu_em_vb_device: solved in HBM for a batch an em.EmBatchSolver holds (EmBatchSolver.run_vb())
model_vb_device  sbgpu_model_vb_device: from what a resident call kept for the bootstrap (sbgpu_bootstrap_keep;
                 quantify_resident(with_variational=True), ChainQuantifier / FrontQuantifier(...).variational())

All return a VariationalFit.  count, share and share_sd are laid out as theta is.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, bins_info, check_lengths, check_tensors, ptr

NAMES = _lib.sbgpu_em_vb_t._NAMES
PER_ISO = ("count", "share", "share_sd")
DTYPES = dict({k: np.float64 for k in NAMES}, status=np.int32, iters=np.int32, n_active=np.int32, n_frag=np.int64)
LIMIT_NAMES = ("wave_vals", "stage_doubles", "wave_loci", "grid_per_cu", "threads", "wave", "max_bins", "max_iso")


def limits():
    """The device form's thresholds (csrc/vb_device.h) by name: see sbgpu_em_vb_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_em_vb_limits(out), "sbgpu_em_vb_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def _params(alpha, change_limit, max_iter):
    """None for all three: NULL (the library's defaults); else a struct with the defaults where one is None"""
    if alpha is None and change_limit is None and max_iter is None:
        return None
    return C.byref(_lib.sbgpu_vb_params_t(0.01 if alpha is None else float(alpha), 1e-2 if change_limit is None else float(change_limit),
                                          1000 if max_iter is None else int(max_iter), 0))


class VariationalFit(Results):
    """count, share, share_sd (float64) [n_iso]; status, iters, n_active (int32), elbo (float64), n_frag (int64) [n_loci].
    want: the names to bring to the host (None: all) -- the device forms copy nothing else over PCIe; the others are None.
    iso_off: the batch's, for the per-locus views.
    .device: name -> device address of the context's copy (device forms; valid until its next quantify / variational call)."""
    STRUCT = _lib.sbgpu_em_vb_t

    def __init__(self, iso_off, want=None):
        self.iso_off = np.asarray(iso_off, np.int64)
        self.n_loci, self.n_iso = len(self.iso_off) - 1, int(self.iso_off[-1])
        self._arrays({k: (self.n_iso if k in PER_ISO else self.n_loci, DTYPES[k]) for k in NAMES}, want)
        self._epilogue = None

    def supported(self, min_count=1.0):
        """bool [n_iso]: the isoforms the posterior leaves at least min_count fragments"""
        return self.count >= min_count

    def rows(self, names=None, iso_names=None):
        """-> (locus, isoform, count, share, share_sd, status, iters, elbo) per isoform, for a TSV: locus and isoform as their
        indices (the isoform's inside its locus), or by name where names / iso_names are given."""
        for l in range(self.n_loci):
            for i in range(int(self.iso_off[l]), int(self.iso_off[l + 1])):
                yield (names[l] if names else l, iso_names[i] if iso_names else i - int(self.iso_off[l]), float(self.count[i]), float(self.share[i]),
                       float(self.share_sd[i]), int(self.status[l]), int(self.iters[l]), float(self.elbo[l]))

    def abundance(self):
        """FPKM / Frac / TPM under this solve: sbgpu_abundance_device + sbgpu_tpm_device on the device's count with the batch's
        lengths and epilogue parameters, as the abundance bootstrap runs them per replicate.  Device forms only, and before the
        context's next variational call -> dict(fpkm, frac, tpm float64, keep int32 [n_iso], total_fpkm) of host arrays."""
        if self._epilogue is None or "count" not in self.device:
            raise _lib.SbgpuError("VariationalFit.abundance: a device form's result with the batch's lengths is needed")
        ctx, plan, d_length, par, torch, stream = self._epilogue
        dev, n = torch.device("cuda", ctx.device), max(self.n_iso, 1)
        fpkm, frac, tpm = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3))
        keep, tot = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(ctx.L.sbgpu_abundance_device(ctx.h, plan.h, self.device["count"], self.device["status"], addr(d_length), C.byref(par),
                                                fpkm.data_ptr(), frac.data_ptr(), keep.data_ptr(), tot.data_ptr(), stream), "sbgpu_abundance_device")
        _lib.check(ctx.L.sbgpu_tpm_device(ctx.h, self.n_iso, fpkm.data_ptr(), keep.data_ptr(), tot.data_ptr(), tpm.data_ptr(), stream),
                   "sbgpu_tpm_device")
        _lib.check(ctx.L.sbgpu_synchronize(ctx.h, stream), "sbgpu_synchronize")
        k = self.n_iso
        return {"fpkm": fpkm[:k].cpu().numpy(), "frac": frac[:k].cpu().numpy(), "tpm": tpm[:k].cpu().numpy(), "keep": keep[:k].cpu().numpy(),
                "total_fpkm": float(tot.cpu()[0])}


def abundance_params(total_mapped_reads, effective_len_norm=False, insert_mean=0.0, filter_by_expression=True, min_isoform_frac=0.01):
    return _lib.sbgpu_abundance_params_t(int(total_mapped_reads), int(effective_len_norm), int(filter_by_expression), 0, float(insert_mean),
                                         float(min_isoform_frac))


def em_vb_host(batch, alpha=None, change_limit=None, max_iter=None, want=None):
    """batch: row_off, iso_off, f_off, count, F (synth.LocusBatch); alpha, change_limit, max_iter: None: the library's defaults."""
    L = _lib.load()
    row_off, iso_off, f_off = (np.ascontiguousarray(a, np.int64) for a in (batch.row_off, batch.iso_off, batch.f_off))
    count, F = np.ascontiguousarray(batch.count, np.int32), np.ascontiguousarray(batch.F, np.float64)
    t = VariationalFit(iso_off, want)
    check_lengths("em_vb_host", ("count", count, int(row_off[-1])), ("F", F, int(f_off[-1])))
    b = _lib.sbgpu_batch_t(t.n_loci, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, ptr(count), ptr(F))
    s = t._struct()
    _lib.check(L.sbgpu_em_vb_host(C.byref(b), _params(alpha, change_limit, max_iter), C.byref(s)), "sbgpu_em_vb_host")
    return t._finish(s)


def em_vb_device(ctx, plan, d_count, d_F, alpha=None, change_limit=None, max_iter=None, stream=None, want=None):
    """plan: an em.Plan; d_count (int32), d_F (float64): torch tensors on the context's device, or device addresses."""
    check_tensors("em_vb_device", d_count=(d_count, "torch.int32"), d_F=(d_F, "torch.float64"))
    t = VariationalFit(plan.iso_off, want)
    s = t._struct()
    _lib.check(ctx.L.sbgpu_em_vb_device(ctx.h, plan.h, addr(d_count), addr(d_F), _params(alpha, change_limit, max_iter), stream, C.byref(s)),
               "sbgpu_em_vb_device")
    return t._finish(s)


def model_vb_device(ctx, handle, alpha=None, change_limit=None, max_iter=None, stream=None, want=None, abundance=None):
    """Right after a resident call made with bootstrap_keep on, on its handle, before the context's next quantify call.
    abundance: the call's sbgpu_abundance_params_t as its epilogue used them (total_mapped_reads and insert_mean filled in): the
    result can then run abundance() -- the handle's offsets and lengths are exported and planned for it."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    n_loci, n_iso = bins_info(L, handle)[:2]
    row_off, iso_off, f_off = (np.zeros(n_loci + 1, np.int64) for _ in range(3))
    iso_len = np.zeros(max(n_iso, 1), np.int32)
    _lib.check(L.sbgpu_bins_export(handle, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, None, iso_len.ctypes.data, *([None] * 8)),
               "sbgpu_bins_export")
    t = VariationalFit(iso_off, want)
    s = t._struct()
    _lib.check(L.sbgpu_model_vb_device(ctx.h, handle, _params(alpha, change_limit, max_iter), stream, C.byref(s)), "sbgpu_model_vb_device")
    t._finish(s)
    if abundance is not None:
        import torch

        from . import em
        t._epilogue = (ctx, em.Plan(ctx, row_off, iso_off, f_off), torch.from_numpy(iso_len).to(torch.device("cuda", ctx.device)), abundance, torch,
                       stream)
    return t

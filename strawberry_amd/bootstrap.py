"""The bootstrap of the resident path: FPKM / TPM mean, spread and percentile intervals; abundances per locus,
and the bootstrap of Frac and of the loci's FPKM / TPM.

interval_ranks              (n_rep, level) -> the two integer positions of the percentile interval
replicate_stats_host        sbgpu_replicate_stats_host: mean, variance and two order statistics per column, plain CPU
replicate_stats_device      sbgpu_replicate_stats_device: the same from boot_interval_kernel
bootstrap_keep              sbgpu_bootstrap_keep: the context's later resident calls leave what the bootstrap needs
                            (quantify_resident(bootstrap=...); ChainQuantifier / FrontQuantifier(keep_bootstrap=True))
abundance_bootstrap_device  sbgpu_abundance_bootstrap_device on such a call's handle -> dict of host arrays
                            (locus=True: locus_bootstrap_device)
locus_abundance_host        sbgpu_locus_abundance_host: the loci's kept-FPKM sums, kept isoforms and TPM, plain CPU
locus_abundance_device      sbgpu_locus_abundance_device: the same from boot_locus_sum_kernel, on device arrays
locus_bootstrap_device      sbgpu_locus_bootstrap_device: abundance_bootstrap_device's dict with "frac" and "locus" entries
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib
from ._results import bins_info

MAX_DEVICE_REP = 1024     # sbgpu_replicate_stats_device / sbgpu_abundance_bootstrap_device: above it SBGPU_ESHAPE

_LOCUS_STATS = ("frac_mean", "frac_var", "frac_lo", "frac_hi", "locus_fpkm_mean", "locus_fpkm_var", "locus_fpkm_lo", "locus_fpkm_hi",
                "locus_tpm_mean", "locus_tpm_var", "locus_tpm_lo", "locus_tpm_hi")
_STATS = ("theta_mean", "theta_var", "fpkm_mean", "fpkm_var", "fpkm_lo", "fpkm_hi", "tpm_mean", "tpm_var", "tpm_lo", "tpm_hi")


def interval_ranks(n_rep, level):
    """The central `level` interval over n_rep replicates as 0-based positions of the sorted replicates:
    lo = floor(n_rep * (1 - level) / 2) in exact rational arithmetic (level as its decimal digits say), hi = n_rep - 1 - lo."""
    n_rep = int(n_rep)
    if n_rep < 1:
        raise ValueError("interval_ranks: n_rep must be at least 1")
    lev = Fraction(str(level)) if not isinstance(level, Fraction) else level
    if not 0 < lev <= 1:
        raise ValueError("interval_ranks: level must lie in (0, 1]")
    lo = int(n_rep * (1 - lev) / 2)          # (a Fraction >= 0: int() is its floor)
    lo = min(lo, (n_rep - 1) // 2)
    return lo, n_rep - 1 - lo


def replicate_stats_host(x, rank_lo, rank_hi):
    """x [n_rep, n] -> dict(mean, var, lo, hi), each [n]: Welford's recurrence in replicate order; lo / hi the elements at
    positions rank_lo / rank_hi of every column sorted ascending, NaNs last (csrc/bootstrap_rules.h)."""
    L = _lib.load()
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2:
        raise ValueError("replicate_stats_host: x must be [n_rep, n]")
    n_rep, n = x.shape
    out = {k: np.zeros(max(n, 1), np.float64) for k in ("mean", "var", "lo", "hi")}
    _lib.check(L.sbgpu_replicate_stats_host(n_rep, n, x.ctypes.data if x.size else None, int(rank_lo), int(rank_hi),
                                            *(out[k].ctypes.data for k in ("mean", "var", "lo", "hi"))), "sbgpu_replicate_stats_host")
    return {k: v[:n] for k, v in out.items()}


def replicate_stats_device(ctx, x, rank_lo, rank_hi):
    """The same on the device: x is a host array (uploaded here) or a float64 torch tensor on the context's device.
    -> dict of host arrays.  n_rep <= MAX_DEVICE_REP."""
    import torch
    dev = torch.device("cuda", ctx.device)
    d_x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    if d_x.dim() != 2 or d_x.dtype != torch.float64:
        raise ValueError("replicate_stats_device: x must be float64 [n_rep, n]")
    d_x = d_x.contiguous()
    n_rep, n = d_x.shape
    out = {k: torch.zeros(max(n, 1), dtype=torch.float64, device=dev) for k in ("mean", "var", "lo", "hi")}
    stream = torch.cuda.current_stream(dev)
    _lib.check(ctx.L.sbgpu_replicate_stats_device(ctx.h, n_rep, n, d_x.data_ptr() if d_x.numel() else None, int(rank_lo), int(rank_hi),
                                                  *(out[k].data_ptr() for k in ("mean", "var", "lo", "hi")), stream.cuda_stream),
               "sbgpu_replicate_stats_device")
    stream.synchronize()
    return {k: v[:n].cpu().numpy() for k, v in out.items()}


def bootstrap_keep(ctx, on=True):
    """Ask the context's later resident calls (sbgpu_quantify_resident, sbgpu_front_stream_end) to leave what
    sbgpu_abundance_bootstrap_device needs."""
    _lib.check(ctx.L.sbgpu_bootstrap_keep(ctx.h, 1 if on else 0), "sbgpu_bootstrap_keep")


def abundance_bootstrap_device(ctx, handle, n_rep, seed, level=0.95, rep_first=0, locus_id=None, ranks=None, keep_theta_rep=False,
                               comm=None, stream=None, replicates=True, locus=False):
    """Right after a resident call made with bootstrap_keep on, on its handle, before the context's next quantify call.
    ranks: (rank_lo, rank_hi), default interval_ranks(n_rep, level).  locus_id: the loci's global ids where this annotation is
    a shard of a sample; comm: the shards' communicator (one all-reduce of the replicates' FPKM totals).
    -> dict: theta_mean / theta_var / fpkm_mean / fpkm_var / fpkm_lo / fpkm_hi / tpm_mean / tpm_var / tpm_lo / tpm_hi [n_iso],
    keep_count [n_iso], status_count [n_loci, 4], total_fpkm_rep [n_rep], rank_lo, rank_hi, n_rep, device (the device addresses of
    d_fpkm_rep / d_keep_rep, valid until the context's next bootstrap or quantify call); with replicates also
    fpkm_rep / keep_rep [n_rep, n_iso] (and theta_rep with keep_theta_rep).
    locus=True: sbgpu_locus_bootstrap_device instead -- the same entries, bit for bit, and two more:
    "frac": dict(mean, var, lo, hi [n_iso]; with replicates rep [n_rep, n_iso]): the isoforms' share of their locus;
    "locus": dict(fpkm_mean / fpkm_var / fpkm_lo / fpkm_hi / tpm_mean / tpm_var / tpm_lo / tpm_hi [n_loci], kept_count [n_loci]:
    replicates in which the locus kept an isoform; with replicates fpkm_rep / kept_rep [n_rep, n_loci])."""
    L = ctx.L
    handle = getattr(handle, "h", handle)      # (a quantify.BinsHandle, or the raw handle)
    (nl, n_iso), B = bins_info(L, handle)[:2], int(n_rep)
    lo, hi = interval_ranks(B, level) if ranks is None else (int(ranks[0]), int(ranks[1]))
    ids = None if locus_id is None else np.ascontiguousarray(locus_id, np.int64)
    if ids is not None and ids.shape != (nl,):
        raise ValueError("locus_id must have one entry per locus")
    par = _lib.sbgpu_bootstrap_params_t(B, int(rep_first), int(seed), None if ids is None or not nl else ids.ctypes.data)
    res = {k: np.zeros(n_iso + 1, np.float64) for k in _STATS}
    res["keep_count"] = np.zeros(n_iso + 1, np.int32)
    res["status_count"] = np.zeros((nl + 1, 4), np.int32)
    res["total_fpkm_rep"] = np.zeros(max(B, 1), np.float64)
    if replicates:      # (the library downloads what it is given room for)
        res["fpkm_rep"] = np.zeros((max(B, 1), n_iso), np.float64)
        res["keep_rep"] = np.zeros((max(B, 1), n_iso), np.int32)
        if keep_theta_rep:
            res["theta_rep"] = np.zeros((max(B, 1), n_iso), np.float64)
    out = _lib.sbgpu_abundance_bootstrap_t()
    for k, v in res.items():
        setattr(out, k, v.ctypes.data if v.size else None)
    if locus:
        lres = {k: np.zeros((n_iso if k.startswith("frac") else nl) + 1, np.float64) for k in _LOCUS_STATS}
        lres["locus_kept_count"] = np.zeros(nl + 1, np.int32)
        if replicates:
            lres["frac_rep"] = np.zeros((max(B, 1), n_iso), np.float64)
            lres["locus_fpkm_rep"] = np.zeros((max(B, 1), nl), np.float64)
            lres["locus_kept_rep"] = np.zeros((max(B, 1), nl), np.int32)
        lout = _lib.sbgpu_locus_bootstrap_t()
        for k, v in lres.items():
            setattr(lout, k, v.ctypes.data if v.size else None)
        _lib.check(L.sbgpu_locus_bootstrap_device(ctx.h, handle, C.byref(par), lo, hi, 1 if keep_theta_rep else 0,
                                                  comm.h if comm is not None else None, stream, C.byref(out), C.byref(lout)),
                   "sbgpu_locus_bootstrap_device")
    else:
        _lib.check(L.sbgpu_abundance_bootstrap_device(ctx.h, handle, C.byref(par), lo, hi, 1 if keep_theta_rep else 0,
                                                      comm.h if comm is not None else None, stream, C.byref(out)),
                   "sbgpu_abundance_bootstrap_device")
    r = {k: res[k][:n_iso] for k in _STATS + ("keep_count",)}
    r.update(status_count=res["status_count"][:nl], total_fpkm_rep=res["total_fpkm_rep"][:B], rank_lo=lo, rank_hi=hi, n_rep=B)
    # (the replicates' matrices where the call left them: splice.splice_psi reads them before the context's next bootstrap / quantify call)
    r["device"] = {"fpkm_rep": int(out.d_fpkm_rep or 0), "keep_rep": int(out.d_keep_rep or 0)}
    for k in ("fpkm_rep", "keep_rep", "theta_rep"):
        if k in res:
            r[k] = res[k][:B]
    if locus:
        r["frac"] = {k: lres["frac_" + k][:n_iso] for k in ("mean", "var", "lo", "hi")}
        r["locus"] = {k[len("locus_"):]: lres[k][:nl] for k in _LOCUS_STATS[4:] + ("locus_kept_count",)}
        if replicates:
            r["frac"]["rep"] = lres["frac_rep"][:B]
            r["locus"].update(fpkm_rep=lres["locus_fpkm_rep"][:B], kept_rep=lres["locus_kept_rep"][:B])
    return r


def locus_bootstrap_device(ctx, handle, n_rep, seed, **kw):
    """sbgpu_locus_bootstrap_device: abundance_bootstrap_device(..., locus=True)"""
    return abundance_bootstrap_device(ctx, handle, n_rep, seed, locus=True, **kw)


def locus_abundance_host(iso_off, fpkm, keep, total_fpkm):
    """sbgpu_locus_abundance_host (csrc/bootstrap_rules.h: boot_locus_sum) -> dict(fpkm, tpm [n_loci] float64, kept [n_loci] int32):
    per locus the sum of its kept isoforms' FPKM in isoform order, 1e6 * that / total_fpkm (0.0 for a locus with nothing kept),
    and the number of kept isoforms."""
    L = _lib.load()
    iso_off = None if iso_off is None else np.ascontiguousarray(iso_off, np.int64)
    fpkm, keep = np.ascontiguousarray(fpkm, np.float64), np.ascontiguousarray(keep, np.int32)
    nl = 0 if iso_off is None else iso_off.size - 1
    if iso_off is not None and (nl < 0 or (iso_off.size and int(iso_off.max()) > min(fpkm.size, keep.size))):
        raise ValueError("locus_abundance_host: iso_off must hold n_loci + 1 offsets into fpkm / keep")
    out = {"fpkm": np.zeros(nl + 1, np.float64), "tpm": np.zeros(nl + 1, np.float64), "kept": np.zeros(nl + 1, np.int32)}
    _lib.check(L.sbgpu_locus_abundance_host(nl, None if iso_off is None else iso_off.ctypes.data, fpkm.ctypes.data if fpkm.size else None,
                                            keep.ctypes.data if keep.size else None, float(total_fpkm), out["fpkm"].ctypes.data,
                                            out["tpm"].ctypes.data, out["kept"].ctypes.data), "sbgpu_locus_abundance_host")
    return {k: v[:nl] for k, v in out.items()}


def locus_abundance_device(ctx, iso_off, fpkm, keep, total_fpkm, stream=None):
    """sbgpu_locus_abundance_device.  iso_off (int64 [n_loci + 1]), fpkm (float64), keep (int32), total_fpkm (float64 [1], or a
    number): torch tensors on the context's device, or host arrays, uploaded here; fpkm and keep also as plain ints: device
    addresses, the d_fpkm / d_keep of a resident call's sbgpu_abundances_t as they stand.  -> dict(fpkm, tpm, kept) of device tensors [n_loci], queued on `stream` (default: torch's current one)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    dt = {"iso_off": (torch.int64, np.int64), "fpkm": (torch.float64, np.float64), "keep": (torch.int32, np.int32), "total": (torch.float64, np.float64)}

    class Raw:      # a device address the caller vouches for (sbgpu_abundances_t's d_fpkm / d_keep)
        def __init__(self, p):
            self.p = int(p)

        def data_ptr(self):
            return self.p

        def numel(self):
            return 1

    def on_device(x, name):
        if isinstance(x, int) and name in ("fpkm", "keep"):
            return Raw(x)
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.atleast_1d(x), dt[name][1])).to(dev)
        if t.dtype != dt[name][0] or t.device != dev:
            raise ValueError("locus_abundance_device: %s must be %s on the context's device" % (name, dt[name][0]))
        return t.contiguous()
    d_off, d_fpkm, d_keep, d_total = on_device(iso_off, "iso_off"), on_device(fpkm, "fpkm"), on_device(keep, "keep"), on_device(total_fpkm, "total")
    nl = d_off.numel() - 1
    if nl < 0 or d_total.numel() < 1:
        raise ValueError("locus_abundance_device: iso_off holds n_loci + 1 offsets, total_fpkm one number")
    out = {"fpkm": torch.zeros(nl + 1, dtype=torch.float64, device=dev), "tpm": torch.zeros(nl + 1, dtype=torch.float64, device=dev),
           "kept": torch.zeros(nl + 1, dtype=torch.int32, device=dev)}
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(ctx.L.sbgpu_locus_abundance_device(ctx.h, nl, d_off.data_ptr(), d_fpkm.data_ptr() if d_fpkm.numel() else None,
                                                  d_keep.data_ptr() if d_keep.numel() else None, d_total.data_ptr(), out["fpkm"].data_ptr(),
                                                  out["tpm"].data_ptr(), out["kept"].data_ptr(), s), "sbgpu_locus_abundance_device")
    return {k: v[:nl] for k, v in out.items()}

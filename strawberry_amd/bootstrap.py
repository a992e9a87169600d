"""The bootstrap of the resident path: FPKM / TPM mean, spread and percentile intervals.

interval_ranks              (n_rep, level) -> the two integer positions of the percentile interval
replicate_stats_host        sbgpu_replicate_stats_host: mean, variance and two order statistics per column, plain CPU
replicate_stats_device      sbgpu_replicate_stats_device: the same from boot_interval_kernel
bootstrap_keep              sbgpu_bootstrap_keep: the context's later resident calls leave what the bootstrap needs
                            (quantify_resident(bootstrap=...); ChainQuantifier / FrontQuantifier(keep_bootstrap=True))
abundance_bootstrap_device  sbgpu_abundance_bootstrap_device on such a call's handle -> dict of host arrays
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib

MAX_DEVICE_REP = 1024     # sbgpu_replicate_stats_device / sbgpu_abundance_bootstrap_device: above it SBGPU_ESHAPE

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
                               comm=None, stream=None, replicates=True):
    """Right after a resident call made with bootstrap_keep on, on its handle, before the context's next quantify call.
    ranks: (rank_lo, rank_hi), default interval_ranks(n_rep, level).  locus_id: the loci's global ids where this annotation is
    a shard of a sample; comm: the shards' communicator (one all-reduce of the replicates' FPKM totals).
    -> dict: theta_mean / theta_var / fpkm_mean / fpkm_var / fpkm_lo / fpkm_hi / tpm_mean / tpm_var / tpm_lo / tpm_hi [n_iso],
    keep_count [n_iso], status_count [n_loci, 4], total_fpkm_rep [n_rep], rank_lo, rank_hi, n_rep; with replicates also
    fpkm_rep / keep_rep [n_rep, n_iso] (and theta_rep with keep_theta_rep)."""
    L = ctx.L
    handle = getattr(handle, "h", handle)      # (a quantify.BinsHandle, or the raw handle)
    info = (C.c_int64 * 8)()
    _lib.check(L.sbgpu_bins_info(handle, info), "sbgpu_bins_info")
    nl, n_iso, B = int(info[0]), int(info[1]), int(n_rep)
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
    _lib.check(L.sbgpu_abundance_bootstrap_device(ctx.h, handle, C.byref(par), lo, hi, 1 if keep_theta_rep else 0,
                                                  comm.h if comm is not None else None, stream, C.byref(out)),
               "sbgpu_abundance_bootstrap_device")
    r = {k: res[k][:n_iso] for k in _STATS + ("keep_count",)}
    r.update(status_count=res["status_count"][:nl], total_fpkm_rep=res["total_fpkm_rep"][:B], rank_lo=lo, rank_hi=hi, n_rep=B)
    for k in ("fpkm_rep", "keep_rep", "theta_rep"):
        if k in res:
            r[k] = res[k][:B]
    return r

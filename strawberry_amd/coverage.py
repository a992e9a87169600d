"""Isoform-resolved coverage: per-exon bases, per-junction mass, per-isoform bases and the bases of every locus that no kept
isoform explains (include/sbgpu.h states the rule).

isoform_coverage_host    sbgpu_isoform_coverage_host: the plain CPU statement, on a handle that holds hit -> bin
isoform_coverage_device  sbgpu_isoform_coverage_device: built in HBM from what a resident call kept and the hits it was given
                         (sbgpu_context_table_keep; quantify_resident(with_coverage=True), ChainQuantifier / FrontQuantifier(keep_context=True))

Both forms return an IsoformCoverage.  exon_bases and junction_mass are laid out as the annotation's exon_left is, iso_bases
as theta is.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

NAMES = ("exon_bases", "junction_mass", "iso_bases", "unexplained_bases")
LIMIT_NAMES = ("item_hits", "lds_exons", "lds_iso", "narrow_iso", "copy_exons", "copies", "max_bins", "max_iso")


def limits():
    """The device form's thresholds (csrc/coverage_device.h) by name: see sbgpu_isoform_coverage_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_isoform_coverage_limits(out), "sbgpu_isoform_coverage_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


class IsoformCoverage(Results):
    """exon_bases / junction_mass [n_exon]; iso_bases [n_iso]; unexplained_bases [n_loci] (float64).
    want: the names to bring to the host (None: all) -- the device form copies nothing else over PCIe; the others are None.
    .device: name -> device address of the context's copy (device form; valid until its next quantify / coverage call)."""
    STRUCT = _lib.sbgpu_isoform_coverage_t

    def __init__(self, n_exon, n_iso, n_loci, want=None):
        self._arrays({k: (n, np.float64) for k, n in zip(NAMES, (n_exon, n_exon, n_iso, n_loci))}, want)

    def exon_depth(self, annot):
        """exon_bases[e] / (R_e - L_e + 1)"""
        return self.exon_bases / (np.asarray(annot.exon_right, np.float64) - np.asarray(annot.exon_left, np.float64) + 1.0)

    def iso_depth(self, annot):
        """iso_bases[j] / the isoform's exonic length (0.0 for an isoform without exons)"""
        ln = np.asarray(annot.exon_right, np.int64) - np.asarray(annot.exon_left, np.int64) + 1
        off = np.asarray(annot.exon_off, np.int64)
        total = np.concatenate([[0], np.cumsum(ln)])[off]
        length = np.diff(total).astype(np.float64)
        return np.divide(self.iso_bases, length, out=np.zeros_like(self.iso_bases), where=length > 0)

    def rows(self, annot, names=None):
        """-> (locus, isoform, exon, left, right, bases, depth, junction_mass) per annotated exon, for a TSV: locus and isoform as
        indices (isoform inside its locus), or -- names = (locus names, isoform names [n_iso]) -- by name; exon counts from 0
        inside its isoform."""
        depth = self.exon_depth(annot)
        iso_off, exon_off = np.asarray(annot.iso_off, np.int64), np.asarray(annot.exon_off, np.int64)
        for l in range(annot.n_loci):
            for i in range(int(iso_off[l]), int(iso_off[l + 1])):
                for e in range(int(exon_off[i]), int(exon_off[i + 1])):
                    yield (names[0][l] if names else l, names[1][i] if names else i - int(iso_off[l]), e - int(exon_off[i]),
                           int(annot.exon_left[e]), int(annot.exon_right[e]), float(self.exon_bases[e]), float(depth[e]), float(self.junction_mass[e]))


def _sizes(L, handle, annot):
    n_loci, n_iso = bins_info(L, handle)[:2]
    return int(np.asarray(annot.exon_off)[-1]), n_iso, n_loci


def isoform_coverage_host(handle, annot, hits, compat, theta, F=None, keep=None, status=None, hit_mass=None, want=None):
    """handle: an sbgpu_bins_t that holds hit -> bin (sbgpu_bins_create, sbgpu_quantify_host), made from annot (exonbin.Annotation)
    and hits (exonbin.Hits); compat [n_hits, cw], theta [n_iso], F, keep, status, hit_mass: as for assign.fragment_assign_host."""
    L = _lib.load()
    handle = getattr(handle, "h", handle)
    n_exon, n_iso, n_loci = _sizes(L, handle, annot)
    compat = np.ascontiguousarray(compat, np.uint32)
    cw = compat.shape[1] if compat.ndim == 2 else 1
    n_hits = compat.shape[0] if compat.ndim == 2 else compat.size
    theta, F, keep, status = as_array(theta, np.float64), as_array(F, np.float64), as_array(keep, np.int32), as_array(status, np.int32)
    hit_mass = as_array(hit_mass, np.float32)
    check_lengths("isoform_coverage_host", ("theta", theta, n_iso), ("keep", keep, n_iso), ("status", status, n_loci), ("hit_mass", hit_mass, n_hits))
    t = IsoformCoverage(n_exon, n_iso, n_loci, want)
    s, a, h = t._struct(), annot._struct(), hits._struct()
    _lib.check(L.sbgpu_isoform_coverage_host(handle, C.byref(a), C.byref(h), ptr(compat), cw, ptr(F), ptr(theta), ptr(keep), ptr(status),
                                             ptr(hit_mass), C.byref(s)), "sbgpu_isoform_coverage_host")
    return t._finish(s)


def isoform_coverage_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=None, stream=None, want=None):
    """Right after a resident call made with retention on (sbgpu_context_table_keep), on its handle, before the context's next
    quantify call.  annot: the call's exonbin.Annotation (host arrays); d_hits: the _lib.sbgpu_hits_t of DEVICE arrays the call
    was given (or sbgpu_front_stream_hits'); d_theta: a float64 torch tensor on the context's device, or a device address
    ([n_iso]; normally the call's own d_theta); d_hit_mass: float32 tensor / address of the masses the call was given, or None
    for unit masses."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    n_exon, n_iso, n_loci = _sizes(L, handle, annot)
    check_tensors("isoform_coverage_device", d_theta=(d_theta, "torch.float64"), d_hit_mass=(d_hit_mass, "torch.float32"))
    t = IsoformCoverage(n_exon, n_iso, n_loci, want)
    s = t._struct()
    a = annot if isinstance(annot, _lib.sbgpu_annotation_t) else annot._struct()
    _lib.check(L.sbgpu_isoform_coverage_device(ctx.h, handle, C.byref(a), C.byref(d_hits), addr(d_theta), addr(d_hit_mass), stream, C.byref(s)),
               "sbgpu_isoform_coverage_device")
    return t._finish(s)

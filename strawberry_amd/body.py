"""Transcript-body coverage profile: every isoform's posterior-weighted bases by 5' -> 3' positional bin, its total, centre and
coefficient of variation, and the sample's gene-body curve per length class (include/sbgpu.h states the rule).

body_profile_host    sbgpu_body_profile_host: the plain CPU statement, on a handle that holds hit -> bin
body_profile_device  sbgpu_body_profile_device: built in HBM from what a resident call kept and the hits it was given
                     (sbgpu_context_table_keep; quantify_resident(with_body_profile=True), ChainQuantifier / FrontQuantifier(keep_context=True))

Both forms return a BodyProfile.  body_bases is [n_iso, n_pos], laid out as theta is; iso_strand: one of 0 (unknown), 1 (+), 2 (-)
per isoform, or None for all 0.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import Results, addr, as_array, bins_info, check_lengths, check_tensors, ptr

NAMES = ("body_bases", "body_total", "body_center", "body_cv", "class_profile", "class_n")
LIMIT_NAMES = ("item_hits", "lds_exons", "lds_iso", "lds_sums", "narrow_iso", "copies", "max_bins", "max_iso")
MAX_POS = 100           # include/sbgpu.h: SBGPU_BODY_MAX_POS
N_POS = 20
CLASS_EDGES = (1000, 2000, 4000)


def limits():
    """The device form's thresholds (csrc/body_device.h) by name: see sbgpu_body_profile_limits."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_body_profile_limits(out), "sbgpu_body_profile_limits")
    return dict(zip(LIMIT_NAMES, (int(x) for x in out)))


def iso_lengths(annot):
    """L_j [n_iso] (int64): the sum of the isoform's exon lengths"""
    ln = np.asarray(annot.exon_right, np.int64) - np.asarray(annot.exon_left, np.int64) + 1
    return np.diff(np.concatenate([[0], np.cumsum(ln)])[np.asarray(annot.exon_off, np.int64)])


def bin_widths(length, n_pos, strand=None):
    """[n_iso, n_pos] (int64): the bases of every REPORTED bin -- ceil((q + 1) L / P) - ceil(q L / P), mirrored on strand 2"""
    L = np.asarray(length, np.int64)[:, None]
    q = np.arange(n_pos + 1, dtype=np.int64)[None, :]
    wd = np.diff((q * L + (n_pos - 1)) // n_pos, axis=1)
    if strand is not None:
        flip = np.asarray(strand) == 2
        wd[flip] = wd[flip, ::-1]
    return wd


class BodyProfile(Results):
    """body_bases [n_iso, n_pos]; body_total / body_center / body_cv [n_iso]; class_profile [4, n_pos] (float64); class_n [4] (int64).
    want: the names to bring to the host (None: all) -- the device form copies nothing else over PCIe; the others are None.
    .device: name -> device address of the context's copy (device form; valid until its next quantify / body-profile call)."""
    STRUCT = _lib.sbgpu_body_profile_t

    def __init__(self, n_iso, n_pos, want=None, iso_strand=None):
        self.n_iso, self.n_pos, self.iso_strand = n_iso, n_pos, iso_strand
        sizes = dict(body_bases=n_iso * n_pos, body_total=n_iso, body_center=n_iso, body_cv=n_iso, class_profile=4 * n_pos, class_n=4)
        self._arrays({k: (sizes[k], np.int64 if k == "class_n" else np.float64) for k in NAMES}, want)

    def _finish(self, s):
        Results._finish(self, s)
        if self.body_bases is not None:
            self.body_bases = self.body_bases.reshape(self.n_iso, self.n_pos)
        if self.class_profile is not None:
            self.class_profile = self.class_profile.reshape(4, self.n_pos)
        return self

    def depth(self, annot):
        """body_bases[j, p] / the bin's width; 0.0 for a bin of width 0 (L_j < n_pos)"""
        wd = bin_widths(iso_lengths(annot), self.n_pos, self.iso_strand).astype(np.float64)
        return np.divide(self.body_bases, wd, out=np.zeros_like(self.body_bases), where=wd > 0)

    def profile(self, j):
        """isoform j's bins over its total: what it adds to its class (zeros where it holds nothing)"""
        t = float(self.body_total[j]) if self.body_total is not None else float(self.body_bases[j].sum())
        return self.body_bases[j] / t if t > 0.0 else np.zeros(self.n_pos)

    def class_curve(self, c):
        """class_profile[c] / class_n[c]: the mean profile of the expressed isoforms of length class c (zeros for an empty class)"""
        n = int(self.class_n[c])
        return self.class_profile[c] / float(n) if n else np.zeros(self.n_pos)

    def bias_3p(self, c=None):
        """The class mass of the last fifth of the bins over that of the first fifth (c None: all classes together; nan where the
        first fifth holds nothing).  1.0 for uniform coverage, above 1.0 for a 3'-biased sample."""
        curve = self.class_profile.sum(axis=0) if c is None else self.class_profile[c]
        k = max(self.n_pos // 5, 1)
        first, last = float(curve[:k].sum()), float(curve[-k:].sum())
        return last / first if first > 0.0 else float("nan")

    def rows(self, annot, names=None):
        """-> (locus, isoform, length, class, total, center, cv, bases_0 .. bases_{P-1}) per isoform, for a TSV: locus and isoform
        as indices (isoform inside its locus), or -- names = (locus names, isoform names [n_iso]) -- by name."""
        length = iso_lengths(annot)
        iso_off = np.asarray(annot.iso_off, np.int64)
        for l in range(annot.n_loci):
            for i in range(int(iso_off[l]), int(iso_off[l + 1])):
                L = int(length[i])
                yield ((names[0][l] if names else l, names[1][i] if names else i - int(iso_off[l]), L, sum(L >= e for e in CLASS_EDGES),
                        float(self.body_total[i]), float(self.body_center[i]), float(self.body_cv[i])) + tuple(float(x) for x in self.body_bases[i]))


def _strand(who, iso_strand, n_iso):
    iso_strand = as_array(iso_strand, np.uint8)
    check_lengths(who, ("iso_strand", iso_strand, n_iso))
    return iso_strand


def body_profile_host(handle, annot, hits, compat, theta, F=None, keep=None, status=None, hit_mass=None, iso_strand=None, n_pos=N_POS, want=None):
    """handle, annot, hits, compat, theta, F, keep, status, hit_mass: as for coverage.isoform_coverage_host."""
    L = _lib.load()
    handle = getattr(handle, "h", handle)
    n_loci, n_iso = bins_info(L, handle)[:2]
    compat = np.ascontiguousarray(compat, np.uint32)
    cw = compat.shape[1] if compat.ndim == 2 else 1
    n_hits = compat.shape[0] if compat.ndim == 2 else compat.size
    theta, F, keep, status = as_array(theta, np.float64), as_array(F, np.float64), as_array(keep, np.int32), as_array(status, np.int32)
    hit_mass, iso_strand = as_array(hit_mass, np.float32), _strand("body_profile_host", iso_strand, n_iso)
    check_lengths("body_profile_host", ("theta", theta, n_iso), ("keep", keep, n_iso), ("status", status, n_loci), ("hit_mass", hit_mass, n_hits))
    n_pos = int(n_pos)
    t = BodyProfile(n_iso, min(max(n_pos, 1), MAX_POS), want, iso_strand)
    s, a, h = t._struct(), annot._struct(), hits._struct()
    _lib.check(L.sbgpu_body_profile_host(handle, C.byref(a), C.byref(h), ptr(compat), cw, ptr(F), ptr(theta), ptr(keep), ptr(status), ptr(hit_mass),
                                         ptr(iso_strand), n_pos, C.byref(s)), "sbgpu_body_profile_host")
    return t._finish(s)


def body_profile_device(ctx, handle, annot, d_hits, d_theta, d_hit_mass=None, iso_strand=None, n_pos=N_POS, stream=None, want=None):
    """Right after a resident call made with retention on (sbgpu_context_table_keep), on its handle, before the context's next
    quantify call: the arguments of coverage.isoform_coverage_device, and iso_strand (a HOST array) and n_pos."""
    L = ctx.L
    handle = getattr(handle, "h", handle)
    n_iso = bins_info(L, handle)[1]
    check_tensors("body_profile_device", d_theta=(d_theta, "torch.float64"), d_hit_mass=(d_hit_mass, "torch.float32"))
    iso_strand = _strand("body_profile_device", iso_strand, n_iso)
    n_pos = int(n_pos)
    t = BodyProfile(n_iso, min(max(n_pos, 1), MAX_POS), want, iso_strand)
    s = t._struct()
    a = annot if isinstance(annot, _lib.sbgpu_annotation_t) else annot._struct()
    _lib.check(L.sbgpu_body_profile_device(ctx.h, handle, C.byref(a), C.byref(d_hits), addr(d_theta), addr(d_hit_mass), ptr(iso_strand), n_pos,
                                           stream, C.byref(s)), "sbgpu_body_profile_device")
    return t._finish(s)

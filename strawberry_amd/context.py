"""The `-f` fragment-context table (Sample::printContext, /root/reference/src/alignments.cpp:1549-1639) as arrays.

context_table_host    sbgpu_context_table_host: the plain CPU statement, on a handle that holds hit -> bin
context_table_device  sbgpu_context_table_device: built in HBM from what a resident call kept
                      (sbgpu_context_table_keep; ChainQuantifier / FrontQuantifier(keep_context=True))
format_table          the arrays -> the text, through sbgpu_format_context_row / _row_seq

Both forms return a ContextTable; its arrays index the handle's bins (row_bin) and the EM batch's layout (row_prob).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._results import as_array, bins_info, ptr
from .output import CONTEXT_HEADER, context_row


class ContextTable:
    """locus_row_off [n_loci + 1]: rows of locus l are [off[l], off[l + 1]); locus_hits [n_loci]: gene_frag_count;
    row_bin / row_hits [n_rows]: the row's global bin and its path_count; row_prob [n_elem]: row r of locus l holds one
    value per isoform of the locus at f_off[l] + (r - locus_row_off[l]) * niso(l)."""

    def __init__(self, n_loci, n_bins, n_elem):
        self.locus_row_off = np.zeros(n_loci + 1, np.int64)
        self.locus_hits = np.zeros(n_loci, np.uint32)
        self.row_bin = np.zeros(max(n_bins, 1), np.int64)
        self.row_hits = np.zeros(max(n_bins, 1), np.uint32)
        self.row_prob = np.zeros(max(n_elem, 1), np.float64)
        self.n_rows = 0

    def _struct(self):
        s = _lib.sbgpu_context_table_t()
        for k in ("locus_row_off", "locus_hits", "row_bin", "row_hits", "row_prob"):
            setattr(s, k, getattr(self, k).ctypes.data)
        return s

    def _finish(self, s, n_elem):
        self.n_rows = int(s.n_rows)
        self.row_bin, self.row_hits = self.row_bin[:self.n_rows], self.row_hits[:self.n_rows]
        self.row_prob = self.row_prob[:n_elem]
        return self

    def row(self, l, r, iso_off, f_off):
        """the probabilities of row r (global) of locus l, one per isoform of the locus"""
        niso = int(iso_off[l + 1] - iso_off[l])
        at = int(f_off[l]) + (r - int(self.locus_row_off[l])) * niso
        return self.row_prob[at:at + niso]


def _sizes(L, handle):
    n_loci, _, n_bins, n_elem = bins_info(L, handle)[:4]
    return n_loci, n_bins, n_elem


def context_table_host(handle, compat, F=None, keep=None, status=None):
    """handle: an sbgpu_bins_t that holds hit -> bin (sbgpu_bins_create, sbgpu_quantify_host); compat [n_hits, cw]: the hits'
    compat words; F: the bin weights (None: the handle's own); keep [n_iso] / status [n_loci] (None: all kept / all started)."""
    L = _lib.load()
    n_loci, n_bins, n_elem = _sizes(L, handle)
    compat = np.ascontiguousarray(compat, np.uint32)
    cw = compat.shape[1] if compat.ndim == 2 else 1
    F, keep, status = as_array(F, np.float64), as_array(keep, np.int32), as_array(status, np.int32)
    t = ContextTable(n_loci, n_bins, n_elem)
    s = t._struct()
    _lib.check(L.sbgpu_context_table_host(handle, ptr(compat), cw, ptr(F), ptr(keep), ptr(status), C.byref(s)),
               "sbgpu_context_table_host")
    return t._finish(s, n_elem)


def context_table_keep(ctx, on=True):
    """Ask the context's later resident calls (sbgpu_quantify_resident, sbgpu_front_stream_end) to keep the table's inputs."""
    _lib.check(ctx.L.sbgpu_context_table_keep(ctx.h, 1 if on else 0), "sbgpu_context_table_keep")


def context_table_device(ctx, handle, stream=None):
    """Right after a resident call made with retention on, on its handle, before the context's next quantify call."""
    L = ctx.L
    handle = getattr(handle, "h", handle)      # (a quantify.BinsHandle, or the raw handle)
    n_loci, n_bins, n_elem = _sizes(L, handle)
    t = ContextTable(n_loci, n_bins, n_elem)
    s = t._struct()
    _lib.check(L.sbgpu_context_table_device(ctx.h, handle, stream, C.byref(s)), "sbgpu_context_table_device")
    return t._finish(s, n_elem)


def format_table(table, sample, total_mapped, gene_ids, transcript_ids, row_off, iso_off, f_off, bin_segments, fpkm, frac, keep=None,
                 seq_stats=None):
    """The text of the `-f` table.  row_off / iso_off / f_off: the handle's; bin_segments(b) -> [(l, r), ...] of global bin b
    (LocusBins.bin_coords); transcript_ids[l]: the isoform names of locus l; fpkm / frac / keep per isoform (the erased
    isoforms' columns are left out, as printContext runs over the survivors); seq_stats = (gc, entropy, flags) per bin for a
    run with `-b`."""
    out = [CONTEXT_HEADER]
    n_iso = int(iso_off[-1])
    keep = np.ones(n_iso, bool) if keep is None else np.asarray(keep)[:n_iso] != 0
    for l, gene in enumerate(gene_ids):
        r0, r1 = int(table.locus_row_off[l]), int(table.locus_row_off[l + 1])
        if r0 == r1:
            continue
        i0, i1 = int(iso_off[l]), int(iso_off[l + 1])
        kept = [j for j in range(i1 - i0) if keep[i0 + j]]
        names = [transcript_ids[l][j] for j in kept]
        for r in range(r0, r1):
            b = int(table.row_bin[r])
            prob = table.row(l, r, iso_off, f_off)
            out.append(context_row(sample, total_mapped, gene, int(table.locus_hits[l]), names, [fpkm[i0 + j] for j in kept],
                                   [prob[j] for j in kept], [frac[i0 + j] for j in kept], bin_segments(b), int(table.row_hits[r]),
                                   None if seq_stats is None else tuple(x[b] for x in seq_stats)))
    return "".join(out)

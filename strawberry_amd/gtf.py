"""A GTF annotation's bytes -> the annotation's arrays (sbgpu_gtf_*, include/sbgpu.h states the rule): loci, isoforms, exons and
disjoint segments as sbgpu_annotation_t holds them, the clusters, the isoforms' lengths and strands, and the names.

    g = read_gtf("genes.gtf", ref_names=[name for name, length in bam.read_header(bam_bytes)[0]])

ctx=None reads on the host; with a Context the file's bytes are parsed and grouped into transcripts on the device
(sbgpu_gtf_read_upload for host bytes, sbgpu_gtf_read_device for a torch uint8 tensor that is on the device already)."""
import ctypes as C

import numpy as np

from . import _lib


def _array(ptr, n, dtype):
    """A copy of n entries at address `ptr` (the handle owns the memory)."""
    dtype = np.dtype(dtype)
    if not n:
        return np.zeros(0, dtype)
    buf = (C.c_char * (int(n) * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


def _names(off, ptr):
    data = bytes(_array(ptr, int(off[-1]), np.uint8))
    return [data[off[k]:off[k + 1]] for k in range(off.size - 1)]


def limits():
    """sbgpu_gtf_limits as a dict."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_gtf_limits(out), "sbgpu_gtf_limits")
    keys = ("tile_lines", "stage_limit", "max_line", "scan_tile", "index_tile", "grid_cap", "max_name", "max_lines")
    return {k: int(v) for k, v in zip(keys, out)}


class GtfAnnotation:
    """Host copies of what an sbgpu_gtf_t holds.  Names are bytes, as the file has them."""

    def __init__(self, handle):
        L = _lib.load()
        try:
            info = (C.c_int64 * 16)()
            _lib.check(L.sbgpu_gtf_info(handle, info), "sbgpu_gtf_info")
            keys = (["lines"] + ["lines_" + s.lower() for s in _lib.GTF_STATUS_NAMES] +
                    ["transcripts", "loci", "exons", "segments", "chromosomes", "merged_exons", "dropped_transcripts"])
            self.info = {k: int(v) for k, v in zip(keys, info)}
            an, cl = _lib.sbgpu_annotation_t(), _lib.sbgpu_clusters_t()
            p_len, p_strand = C.c_void_p(), C.c_void_p()
            _lib.check(L.sbgpu_gtf_annotation(handle, C.byref(an), C.byref(cl), C.byref(p_len), C.byref(p_strand)), "sbgpu_gtf_annotation")
            nl = self.n_loci = int(an.n_loci)
            self.iso_off = _array(an.iso_off, nl + 1, np.int64)
            n_iso = self.n_iso = int(self.iso_off[-1])
            self.exon_off = _array(an.exon_off, n_iso + 1, np.int64)
            n_exon = int(self.exon_off[-1])
            self.exon_left, self.exon_right = _array(an.exon_left, n_exon, np.uint32), _array(an.exon_right, n_exon, np.uint32)
            self.seg_off = _array(an.seg_off, nl + 1, np.int64)
            n_seg = int(self.seg_off[-1])
            self.seg_left, self.seg_right = _array(an.seg_left, n_seg, np.uint32), _array(an.seg_right, n_seg, np.uint32)
            self.cluster_ref = _array(cl.ref, nl, np.int32)
            self.cluster_left, self.cluster_right = _array(cl.left, nl, np.uint32), _array(cl.right, nl, np.uint32)
            self.cluster_strand = _array(cl.strand, nl, np.uint8)
            self.iso_len, self.iso_strand = _array(p_len.value, n_iso, np.int32), _array(p_strand.value, n_iso, np.uint8)
            nm = _lib.sbgpu_gtf_names_t()
            _lib.check(L.sbgpu_gtf_names(handle, C.byref(nm)), "sbgpu_gtf_names")
            self.gene_id = _names(_array(nm.gene_id_off, nl + 1, np.int64), nm.gene_id)
            self.gene_name = _names(_array(nm.gene_name_off, nl + 1, np.int64), nm.gene_name)
            self.transcript_id = _names(_array(nm.transcript_id_off, n_iso + 1, np.int64), nm.transcript_id)
            self.chrom = _names(_array(nm.chrom_off, self.info["chromosomes"] + 1, np.int64), nm.chrom)
            self.line_status = np.zeros(self.info["lines"], np.uint8)
            _lib.check(L.sbgpu_gtf_line_status(handle, self.line_status.ctypes.data if self.line_status.size else None), "sbgpu_gtf_line_status")
        finally:
            L.sbgpu_gtf_destroy(handle)

    def annotation(self):
        """(sbgpu_annotation_t, sbgpu_clusters_t) over this object's arrays (which must outlive them)."""
        an, cl = _lib.sbgpu_annotation_t(), _lib.sbgpu_clusters_t()
        an.n_loci = cl.n_clusters = self.n_loci
        for name in ("iso_off", "exon_off", "exon_left", "exon_right", "seg_off", "seg_left", "seg_right"):
            setattr(an, name, getattr(self, name).ctypes.data)
        cl.ref, cl.left, cl.right, cl.strand = (getattr(self, "cluster_" + n).ctypes.data for n in ("ref", "left", "right", "strand"))
        return an, cl

    def rows(self):
        """One dict per locus: chrom (id), left, right, strand, gene_id, gene_name and its isoforms -- (transcript_id, strand,
        length, [(left, right), ...]) -- in the annotation's order."""
        out = []
        for l in range(self.n_loci):
            isoforms = []
            for i in range(int(self.iso_off[l]), int(self.iso_off[l + 1])):
                e0, e1 = int(self.exon_off[i]), int(self.exon_off[i + 1])
                isoforms.append((self.transcript_id[i], int(self.iso_strand[i]), int(self.iso_len[i]),
                                 [(int(a), int(b)) for a, b in zip(self.exon_left[e0:e1], self.exon_right[e0:e1])]))
            out.append({"chrom": int(self.cluster_ref[l]), "left": int(self.cluster_left[l]), "right": int(self.cluster_right[l]),
                        "strand": int(self.cluster_strand[l]), "gene_id": self.gene_id[l], "gene_name": self.gene_name[l], "isoforms": isoforms})
        return out


def _opts(ref_names, hash_bits):
    o = _lib.sbgpu_gtf_opts_t()
    names = [n if isinstance(n, bytes) else str(n).encode() for n in (ref_names or [])]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    o.n_ref, o.ref_name, o.hash_bits = len(names), arr, int(hash_bits)
    return o, arr


def read_gtf(path_or_bytes, ref_names=None, ctx=None, hash_bits=0):
    """path_or_bytes: a file's path (str), its bytes (bytes / bytearray / uint8 array), or -- with ctx -- a torch uint8 tensor on
    the context's device.  ref_names: the BAM header's reference names (chromosome ids are then their indices, and transcripts
    on other chromosomes are dropped); None: ids by first appearance.  hash_bits: for tests (sbgpu_gtf_opts_t)."""
    L = _lib.load()
    opts, _keep = _opts(ref_names, hash_bits)
    h = C.c_void_p()
    if ctx is not None and hasattr(path_or_bytes, "data_ptr"):
        import torch
        d = path_or_bytes
        if d.dtype != torch.uint8 or not d.is_cuda or not d.is_contiguous():
            raise ValueError("a device tensor must be contiguous uint8")
        torch.cuda.synchronize(d.device)
        _lib.check(L.sbgpu_gtf_read_device(ctx.h, d.data_ptr() if d.numel() else None, int(d.numel()), C.byref(opts), None, C.byref(h)),
                   "sbgpu_gtf_read_device")
        return GtfAnnotation(h)
    if isinstance(path_or_bytes, str):
        with open(path_or_bytes, "rb") as f:
            path_or_bytes = f.read()
    b = np.frombuffer(path_or_bytes, np.uint8) if isinstance(path_or_bytes, (bytes, bytearray)) else np.ascontiguousarray(path_or_bytes, np.uint8)
    p = b.ctypes.data if b.size else None
    if ctx is None:
        _lib.check(L.sbgpu_gtf_read_host(p, b.size, C.byref(opts), C.byref(h)), "sbgpu_gtf_read_host")
    else:
        _lib.check(L.sbgpu_gtf_read_upload(ctx.h, p, b.size, C.byref(opts), None, C.byref(h)), "sbgpu_gtf_read_upload")
    return GtfAnnotation(h)

"""A genome FASTA's bytes -> the contigs' names, their sequences packed back to back and a .fai index (sbgpu_fasta_*,
include/sbgpu.h states the rule).

    g = read_fasta("genome.fa", device=0)
    gc, entropy, flags = g.bin_sequence_stats(bins, locus_chrom)      # `-b genome.fa` over every chromosome

device=None reads on the host; with a device number the file's bytes are packed on that device and the sequence stays there
(sbgpu_fasta_read_upload for host bytes, sbgpu_fasta_read_device for a torch uint8 tensor that is on the device already)."""
import ctypes as C

import numpy as np

from . import _lib

EMPTY, RAGGED, DUPLICATE, NONAME = 1, 2, 4, 8
INFO_KEYS = ("bytes", "lines", "contigs", "bases", "empty", "ragged", "duplicate", "noname", "longest", "longest_contig", "on_device", "device")


def _array(ptr, n, dtype):
    """A copy of n entries at address `ptr` (the handle owns the memory)."""
    dtype = np.dtype(dtype)
    if not n:
        return np.zeros(0, dtype)
    buf = (C.c_char * (int(n) * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


def limits():
    """sbgpu_fasta_limits as a dict."""
    out = (C.c_int64 * 8)()
    _lib.check(_lib.load().sbgpu_fasta_limits(out), "sbgpu_fasta_limits")
    keys = ("tile", "scan_tile", "grid_cap", "max_header", "max_contigs")
    return {k: int(v) for k, v in zip(keys, out)}


class FastaGenome:
    """An sbgpu_fasta_t and host copies of its per-contig arrays.  Names are bytes, as the file has them."""

    def __init__(self, handle, ctx=None):
        L = _lib.load()
        self._h, self._ctx = handle, ctx
        try:
            info = (C.c_int64 * 16)()
            _lib.check(L.sbgpu_fasta_info(handle, info), "sbgpu_fasta_info")
            self.info = {k: int(v) for k, v in zip(INFO_KEYS, info)}
            n = self.n_contigs = self.info["contigs"]
            p = [C.c_void_p() for _ in range(5)]
            _lib.check(L.sbgpu_fasta_index(handle, *[C.byref(x) for x in p]), "sbgpu_fasta_index")
            self.seq_off = _array(p[0].value, n + 1, np.int64)
            self.offset, self.line_bases, self.line_width = (_array(x.value, n, np.int64) for x in p[1:4])
            self.flags = _array(p[4].value, n, np.uint8)
            self.length = np.diff(self.seq_off)
            p_off, p_names = C.c_void_p(), C.c_void_p()
            _lib.check(L.sbgpu_fasta_names(handle, C.byref(p_off), C.byref(p_names)), "sbgpu_fasta_names")
            off = _array(p_off.value, n + 1, np.int64)
            data = bytes(_array(p_names.value, int(off[-1]), np.uint8))
            self.names = [data[off[k]:off[k + 1]] for k in range(n)]
        except Exception:
            self.close()
            raise

    def close(self):
        if self._h is not None:
            _lib.load().sbgpu_fasta_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def on_device(self):
        return bool(self.info["on_device"])

    @property
    def index(self):
        """One (name, length, offset, line_bases, line_width) per contig: the .fai columns."""
        return [(self.names[c], int(self.length[c]), int(self.offset[c]), int(self.line_bases[c]), int(self.line_width[c])) for c in range(self.n_contigs)]

    def find(self, name):
        """The first contig of that name, compared ASCII-lower-cased; -1 where there is none."""
        name = name if isinstance(name, bytes) else str(name).encode()
        out = C.c_int64(-1)
        _lib.check(_lib.load().sbgpu_fasta_find(self._h, name, len(name), C.byref(out)), "sbgpu_fasta_find")
        return int(out.value)

    def fetch(self, contig, start, length):
        """`length` bases of a contig (an index or a name) from base `start`, 1-based, as bytes."""
        c = contig if isinstance(contig, (int, np.integer)) else self.find(contig)
        out = np.zeros(max(int(length), 1), np.uint8)
        _lib.check(_lib.load().sbgpu_fasta_fetch(self._h, int(c), int(start), int(length), out.ctypes.data), "sbgpu_fasta_fetch")
        return out[:max(int(length), 0)].tobytes()

    def sequence(self, name):
        """A contig's whole sequence as bytes."""
        c = name if isinstance(name, (int, np.integer)) else self.find(name)
        if c < 0:
            raise KeyError(name)
        return self.fetch(c, 1, int(self.length[c]))

    def packed(self):
        """The whole packed sequence as a uint8 array on the host (from a device: one copy per contig)."""
        out = np.zeros(int(self.seq_off[-1]), np.uint8)
        L = _lib.load()
        for c in range(self.n_contigs):
            a, b = int(self.seq_off[c]), int(self.seq_off[c + 1])
            if b > a:
                _lib.check(L.sbgpu_fasta_fetch(self._h, c, 1, b - a, out[a:b].ctypes.data), "sbgpu_fasta_fetch")
        return out

    def fai_text(self):
        L = _lib.load()
        need = C.c_int64()
        _lib.check(L.sbgpu_fasta_fai(self._h, None, 0, C.byref(need)), "sbgpu_fasta_fai")
        buf = C.create_string_buffer(max(int(need.value), 1))
        _lib.check(L.sbgpu_fasta_fai(self._h, buf, int(need.value), C.byref(need)), "sbgpu_fasta_fai")
        return buf.raw[:int(need.value)].decode("latin-1")

    def sequence_pointer(self):
        """(address, on_device) of the packed sequence."""
        p, dev = C.c_void_p(), C.c_int32()
        _lib.check(_lib.load().sbgpu_fasta_sequence(self._h, C.byref(p), C.byref(dev)), "sbgpu_fasta_sequence")
        return p.value, bool(dev.value)

    def runs(self, bins, locus_chrom):
        """(run_off, run_contig) of an exonbin.LocusBins: consecutive loci on one chromosome make a run of bins.  locus_chrom: a
        name per locus of the bins' annotation; a name the genome lacks raises KeyError."""
        row_off = np.asarray(bins.row_off, np.int64)
        contig = []
        for name in locus_chrom:
            c = self.find(name)
            if c < 0:
                raise KeyError(name)
            contig.append(c)
        if len(contig) != row_off.size - 1:
            raise ValueError("a chromosome name per locus is needed")
        run_off, run_contig = [0], []
        for l, c in enumerate(contig):
            if row_off[l + 1] == row_off[l]:
                continue
            if run_contig and run_contig[-1] == c:
                run_off[-1] = int(row_off[l + 1])
            else:
                run_contig.append(c)
                run_off.append(int(row_off[l + 1]))
        return np.asarray(run_off, np.int64), np.asarray(run_contig, np.int32)

    def bin_sequence_stats(self, bins, locus_chrom, ctx=None):
        """(gc, entropy, flags) per bin of an exonbin.LocusBins, in bin order, as output.py's seq_stats= takes them.  With the
        sequence on a device the statistics run there on the resident sequence (sbgpu_binseq_fasta_device); else through the
        host-buffer form."""
        from .binseq import bin_segments
        from .em import default_context
        L = _lib.load()
        ctx = ctx or self._ctx or default_context(max(self.info["device"], 0))
        seg_off, seg_left, seg_right = bin_segments(bins)
        run_off, run_contig = self.runs(bins, locus_chrom)
        return self.run_stats(run_off, run_contig, seg_off, seg_left, seg_right, ctx)

    def run_stats(self, run_off, run_contig, seg_off, seg_left, seg_right, ctx=None, host_form=False):
        """The same for bins given as CSR segment lists and runs."""
        from .em import default_context
        L = _lib.load()
        ctx = ctx or self._ctx or default_context(max(self.info["device"], 0))
        run_off, run_contig = np.ascontiguousarray(run_off, np.int64), np.ascontiguousarray(run_contig, np.int32)
        seg_off = np.ascontiguousarray(seg_off, np.int64)
        seg_left, seg_right = np.ascontiguousarray(seg_left, np.uint32), np.ascontiguousarray(seg_right, np.uint32)
        n, n_runs = seg_off.size - 1, run_contig.size
        ptr = lambda a: a.ctypes.data if a.size else None   # noqa: E731
        if not self.on_device or host_form:
            gc, ent, fl = np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)
            _lib.check(L.sbgpu_binseq_fasta_host(ctx.h, self._h, n_runs, ptr(run_off), ptr(run_contig), n, ptr(seg_off), ptr(seg_left), ptr(seg_right),
                                                 ptr(gc), ptr(ent), ptr(fl)), "sbgpu_binseq_fasta_host")
            return gc, ent, fl
        import torch
        dev = torch.device("cuda", self.info["device"])
        d_off = torch.from_numpy(seg_off).to(dev)
        d_left, d_right = torch.from_numpy(seg_left.view(np.int32)).to(dev), torch.from_numpy(seg_right.view(np.int32)).to(dev)
        gc, ent = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        fl, err = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        dp = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
        _lib.check(L.sbgpu_binseq_fasta_device(ctx.h, self._h, n_runs, ptr(run_off), ptr(run_contig), n, dp(d_off), dp(d_left), dp(d_right), dp(gc), dp(ent),
                                               dp(fl), err.data_ptr(), s), "sbgpu_binseq_fasta_device")
        torch.cuda.synchronize(dev)
        if int(err.item()):
            raise _lib.SbgpuError("sbgpu_binseq_fasta_device: the kernel rejected a bin (segment outside its contig)")
        return gc.cpu().numpy(), ent.cpu().numpy(), fl.cpu().numpy()


def read_fasta(path_or_bytes, device=None, ctx=None):
    """path_or_bytes: a file's path (str), its bytes (bytes / bytearray / uint8 array), or -- with a device -- a torch uint8
    tensor on that device.  device: None reads on the host; a device number packs the sequence there, where it stays."""
    L = _lib.load()
    h = C.c_void_p()
    if device is None and ctx is None and not hasattr(path_or_bytes, "data_ptr"):
        b = _host_bytes(path_or_bytes)
        _lib.check(L.sbgpu_fasta_read_host(b.ctypes.data if b.size else None, b.size, C.byref(h)), "sbgpu_fasta_read_host")
        return FastaGenome(h)
    if ctx is None:
        from .em import default_context
        ctx = default_context(int(device or 0))
    if hasattr(path_or_bytes, "data_ptr"):
        import torch
        d = path_or_bytes
        if d.dtype != torch.uint8 or not d.is_cuda or not d.is_contiguous():
            raise ValueError("a device tensor must be contiguous uint8")
        torch.cuda.synchronize(d.device)
        _lib.check(L.sbgpu_fasta_read_device(ctx.h, d.data_ptr() if d.numel() else None, int(d.numel()), None, C.byref(h)), "sbgpu_fasta_read_device")
        return FastaGenome(h, ctx)
    b = _host_bytes(path_or_bytes)
    _lib.check(L.sbgpu_fasta_read_upload(ctx.h, b.ctypes.data if b.size else None, b.size, None, C.byref(h)), "sbgpu_fasta_read_upload")
    return FastaGenome(h, ctx)


def _host_bytes(path_or_bytes):
    if isinstance(path_or_bytes, str):
        with open(path_or_bytes, "rb") as f:
            path_or_bytes = f.read()
    if isinstance(path_or_bytes, (bytes, bytearray)):
        return np.frombuffer(path_or_bytes, np.uint8)
    return np.ascontiguousarray(path_or_bytes, np.uint8)

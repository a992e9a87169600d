"""BAM alignment records -> the read stream: the host-side mirror of sbgpu_bam_index_host / sbgpu_bam_decode_host /
sbgpu_bam_decode_device (include/sbgpu.h), i.e. of the reference's BAMHitFactory::getHitFromBuf
(/root/reference/src/read.cpp:480-715).

    off = bam.index(rec_bytes)                       # record offsets of the uncompressed record stream
    rd = bam.decode(rec_bytes, off, device=ctx)      # DecodedReads: accepted records as arrays, why the others were refused
    rd.reads()                                       # -> exonbin.Reads-like arguments for pair_mates / assign_reads

The record stream is what follows the BAM header once the BGZF blocks are inflated.  The library inflates them itself
(sbgpu_bgzf_index_host / sbgpu_bgzf_inflate_host / sbgpu_bgzf_inflate_device: no zlib), and finds the records of a stream
that was inflated on the device there (sbgpu_bam_index_device):

    blk_off, out_off = bam.bgzf_index(file_bytes)    # the file's block table
    raw = bam.inflate(file_bytes)                    # the inflated stream (device=ctx: a torch uint8 tensor on the device)
    rd = bam.decode_file(file_bytes, device=ctx)     # file -> inflate -> index -> decode, all on the device"""
import ctypes as C
import struct

import numpy as np

from . import _lib


class BamOptions:
    """The reference's option globals that decide a record's fate (src/common.cpp:19-21,67-69)."""

    def __init__(self, min_intron=20, max_intron=300000, unique_only=True, library=0, n_ref=0):
        self.min_intron, self.max_intron, self.unique_only, self.library, self.n_ref = min_intron, max_intron, unique_only, library, n_ref

    def c(self):
        return _lib.sbgpu_bam_opts_t(int(self.min_intron), int(self.max_intron), int(bool(self.unique_only)), int(self.library), int(self.n_ref))


BGZF_STATUS_NAMES = ("ok", "reserved block type", "stored block LEN/NLEN disagree", "bad code lengths", "invalid symbol",
                     "distance before the member's start", "input ran out", "output is not ISIZE bytes")


def _file_array(file_bytes):
    if isinstance(file_bytes, np.ndarray):
        return np.ascontiguousarray(file_bytes, np.uint8)
    return np.frombuffer(file_bytes, np.uint8)


def bgzf_index(file_bytes):
    """A BGZF file's bytes -> (blk_off, out_off), int64[n + 1] each: where every member starts in the file and where its
    bytes land in the inflated stream."""
    f = _file_array(file_bytes)
    cap = f.size // 26 + 1
    blk, out = np.zeros(cap + 1, np.int64), np.zeros(cap + 1, np.int64)
    n = _lib.load().sbgpu_bgzf_index_host(f.ctypes.data if f.size else None, f.size, blk.ctypes.data, out.ctypes.data, cap)
    if n < 0:
        raise _lib.SbgpuError("sbgpu_bgzf_index_host: " + (_lib.load().sbgpu_last_error() or b"").decode())
    return blk[:n + 1].copy(), out[:n + 1].copy()


def _raise_failed(status, blk_off, first=0):
    bad = np.flatnonzero(status)
    if bad.size:
        b = int(bad[0])
        raise _lib.SbgpuError("BGZF member %d at byte %d of the file: %s (%d of %d members failed)" % (
            first + b, int(blk_off[first + b]), BGZF_STATUS_NAMES[min(int(status[b]), 7)], bad.size, status.size))


def inflate(file_bytes, device=None, table=None, n_blocks=None):
    """The inflated stream of a BGZF file (or of its first n_blocks members).  device None: a uint8 array made by host threads;
    a Context: a torch uint8 tensor made on the device (file and table uploaded through torch).  A member that does not
    inflate to its ISIZE bytes raises."""
    L = _lib.load()
    f = _file_array(file_bytes)
    blk, out = table if table is not None else bgzf_index(f)
    n = blk.size - 1 if n_blocks is None else int(n_blocks)
    total = int(out[n])
    if device is None:
        raw, status = np.zeros(total, np.uint8), np.zeros(max(n, 1), np.uint8)
        _lib.check(L.sbgpu_bgzf_inflate_host(f.ctypes.data if f.size else None, f.size, blk.ctypes.data, out.ctypes.data, 0, n,
                                             raw.ctypes.data if total else status.ctypes.data, status.ctypes.data), "sbgpu_bgzf_inflate_host")
        _raise_failed(status[:n], blk)
        return raw
    import torch
    dev = torch.device("cuda", device.device)
    d_file = torch.from_numpy(f if f.flags.writeable else f.copy()).to(dev) if f.size else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_blk, d_out_off = torch.from_numpy(blk).to(dev), torch.from_numpy(out).to(dev)
    d_raw = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    d_status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    failed = C.c_int64(0)
    torch.cuda.synchronize(dev)
    _lib.check(L.sbgpu_bgzf_inflate_device(device.h, d_file.data_ptr(), f.size, d_blk.data_ptr(), d_out_off.data_ptr(), n, d_raw.data_ptr(),
                                           None, d_status.data_ptr(), C.byref(failed)), "sbgpu_bgzf_inflate_device")
    if failed.value:
        _raise_failed(d_status.cpu().numpy()[:n], blk)
    return d_raw[:total]


def header_length(raw):
    """(references, where record 0 starts) from the head of an inflated BAM stream; raises IndexError / struct.error when
    `raw` is too short to hold the whole header."""
    if bytes(raw[:4]) != b"BAM\1":
        raise ValueError("not a BAM file")
    buf = raw.tobytes() if isinstance(raw, np.ndarray) else bytes(raw)
    l_text, = struct.unpack_from("<i", buf, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", buf, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", buf, p)
        refs.append((buf[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", buf, p + 4 + l_name)[0]))
        p += 8 + l_name
    if p > len(buf):
        raise IndexError("the header is longer than the bytes given")
    return refs, p


def read_header(file_bytes, table=None):
    """(references, the header's length in the inflated stream): inflates members on the host until the header is whole."""
    f = _file_array(file_bytes)
    table = table if table is not None else bgzf_index(f)
    n, k = table[0].size - 1, 1
    while True:
        k = min(k, n)
        try:
            return header_length(inflate(f, table=table, n_blocks=k))
        except (IndexError, struct.error):
            if k >= n:
                raise ValueError("the file ends inside the BAM header")
            k *= 2


def split_header(bam_bytes):
    """A whole (small) BAM file's bytes -> ([(reference name, length)], the record stream as uint8); inflated by the
    library's host form."""
    raw = inflate(bam_bytes)
    try:
        refs, p = header_length(raw)
    except (IndexError, struct.error):
        raise ValueError("the file ends inside the BAM header")
    return refs, raw[p:].copy()


def index(rec_bytes):
    """-> int64[n + 1]: where every record starts (and where the stream ends)."""
    b = np.ascontiguousarray(rec_bytes, np.uint8)
    cap = b.size // 4 + 1      # the indexer accepts any block_size (a malformed stream comes back as TRUNCATED records, not as an error)
    off = np.zeros(cap + 1, np.int64)
    n = _lib.load().sbgpu_bam_index_host(b.ctypes.data if b.size else None, b.size, off.ctypes.data, cap)
    if n < 0:
        raise _lib.SbgpuError("sbgpu_bam_index_host: " + (_lib.load().sbgpu_last_error() or b"").decode())
    return off[:n + 1].copy()


class DecodedReads:
    """Host copies of an sbgpu_bamreads_t."""

    def __init__(self, handle, keep=None):
        L = _lib.load()
        info = (C.c_int64 * 16)()
        _lib.check(L.sbgpu_bamreads_info(handle, info), "sbgpu_bamreads_info")
        self.n_records, self.n_reads, self.n_blocks = int(info[0]), int(info[1]), int(info[2])
        self.any_paired, self.on_device = bool(info[3]), bool(info[4])
        self.by_status = {name: int(info[5 + k]) for k, name in enumerate(_lib.BAM_STATUS_NAMES)}
        n, m, nb = self.n_records, self.n_reads, self.n_blocks
        self.status = np.zeros(n, np.uint8)
        self.record = np.zeros(m, np.int64)
        self.read_id = np.zeros(m, np.uint64)
        self.ref, self.nh, self.nm, self.read_len = (np.zeros(m, np.int32) for _ in range(4))
        self.left, self.right, self.partner_pos, self.sam_flag = (np.zeros(m, np.uint32) for _ in range(4))
        self.flags = np.zeros(m, np.uint8)
        self.block_off = np.zeros(m + 1, np.int64)
        self.block_left, self.block_right = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32)
        p = lambda a: a.ctypes.data if a.size else None
        _lib.check(L.sbgpu_bamreads_export(handle, p(self.status), p(self.record), p(self.read_id), p(self.ref), p(self.left), p(self.right),
                                           p(self.partner_pos), p(self.flags), p(self.nh), p(self.nm), p(self.read_len), p(self.sam_flag),
                                           p(self.block_off), p(self.block_left), p(self.block_right)), "sbgpu_bamreads_export")
        self._handle, self._keep = handle, keep

    def close(self):
        if self._handle is not None:
            _lib.load().sbgpu_bamreads_destroy(self._handle)
            self._handle = None

    __del__ = close

    def device_reads(self):
        """(sbgpu_reads_t, ref ptr, left ptr, right ptr) over the handle's own arrays (device arrays after a device decode)."""
        L = _lib.load()
        rs = _lib.sbgpu_reads_t()
        r, l, rr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(L.sbgpu_bamreads_reads(self._handle, C.byref(rs), C.byref(r), C.byref(l), C.byref(rr)), "sbgpu_bamreads_reads")
        return rs, r.value, l.value, rr.value


def index_device(d_bytes, first_record, d_guess, device, cap=None):
    """sbgpu_bam_index_device over a torch uint8 tensor on the device -> (torch int64[n + 1] offsets relative to first_record,
    info: rounds, segments, walks repeated, first segment of the sequential walker or -1)."""
    import torch
    L = _lib.load()
    n_bytes = int(d_bytes.numel())
    cap = (n_bytes - first_record) // 4 + 1 if cap is None else int(cap)
    d_off = torch.empty(cap + 1, dtype=torch.int64, device=d_bytes.device)
    torch.cuda.synchronize(d_bytes.device)
    n = L.sbgpu_bam_index_device(device.h, d_bytes.data_ptr() if n_bytes else None, n_bytes, int(first_record),
                                 d_guess.data_ptr() if d_guess is not None and d_guess.numel() else None,
                                 int(d_guess.numel()) if d_guess is not None else 0, d_off.data_ptr(), cap, None)
    info = (C.c_int64 * 8)()
    L.sbgpu_bam_index_device_info(info)
    if n < 0:
        raise _lib.SbgpuError("sbgpu_bam_index_device: " + (L.sbgpu_last_error() or b"").decode())
    return d_off[:n + 1], [int(v) for v in info[:4]]


def decode_file(file_bytes, options=None, device=None):
    """A BAM file's bytes -> DecodedReads.  With a Context the file is uploaded as it is, inflated, indexed and decoded on the
    device (only the header's members are also inflated on the host, to learn where record 0 starts); without one the host
    forms do the same."""
    f = _file_array(file_bytes)
    table = bgzf_index(f)
    if device is None:
        refs, rec = split_header(f)
        return decode(rec, None, options, None)
    import torch
    L = _lib.load()
    refs, first = read_header(f, table)
    d_raw = inflate(f, device=device, table=table)
    d_guess = torch.from_numpy(table[1]).to(d_raw.device)
    # (an average record is far longer than 36 bytes -- its fixed part -- but nothing promises it: a stream of shorter ones
    # is indexed again with the cap that always suffices)
    try:
        d_off, _ = index_device(d_raw, first, d_guess, device, cap=(int(d_raw.numel()) - first) // 36 + 1024)
    except _lib.SbgpuError as e:
        if "`cap`" not in str(e):
            raise
        d_off, _ = index_device(d_raw, first, d_guess, device)
    n = int(d_off.numel()) - 1
    opts = (options or BamOptions()).c()
    h = C.c_void_p()
    d_rec = d_raw[first:] if int(d_raw.numel()) > first else torch.zeros(1, dtype=torch.uint8, device=d_raw.device)
    _lib.check(L.sbgpu_bam_decode_device(device.h, d_rec.data_ptr(), int(d_raw.numel()) - first, d_off.data_ptr(), n, C.byref(opts), None, C.byref(h)),
               "sbgpu_bam_decode_device")
    return DecodedReads(h, keep=(d_raw, d_off))


def decode(rec_bytes, rec_off=None, options=None, device=None):
    """Decode an uncompressed record stream.  device: a Context -> sbgpu_bam_decode_device (bytes and offsets uploaded
    through torch), else the host form."""
    L = _lib.load()
    opts = (options or BamOptions()).c()
    b = np.ascontiguousarray(rec_bytes, np.uint8)
    off = index(b) if rec_off is None else np.ascontiguousarray(rec_off, np.int64)
    n = off.size - 1
    h = C.c_void_p()
    if device is None:
        _lib.check(L.sbgpu_bam_decode_host(b.ctypes.data if b.size else None, b.size, off.ctypes.data, n, C.byref(opts), C.byref(h)),
                   "sbgpu_bam_decode_host")
        return DecodedReads(h)
    import torch
    dev = torch.device("cuda", device.device)
    hb = b if b.size else np.zeros(1, np.uint8)
    db = torch.from_numpy(hb if hb.flags.writeable else hb.copy()).to(dev)
    do = torch.from_numpy(off).to(dev)
    _lib.check(L.sbgpu_bam_decode_device(device.h, db.data_ptr(), b.size, do.data_ptr(), n, C.byref(opts), None, C.byref(h)),
               "sbgpu_bam_decode_device")
    return DecodedReads(h, keep=(db, do))

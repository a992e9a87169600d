"""BGZF members made in Python for the inflate tests (tests/test_bgzf.py, tests/test_bgzf_gpu.py): a corpus that reaches every
block type and copy shape of RFC 1951, damaged members, and what zlib -- the library the reference links -- makes of them.

  member(payload, data)     one BGZF member around a raw deflate payload (the framing of bam_util._bgzf_block)
  corpus(rng)               -> [Member]: payload kinds x sizes x levels x strategies, plus a member of many flushed blocks
  damaged(rng, members, n)  -> [Member]: one bit flipped, or the payload one byte shorter / longer; framing and ISIZE valid
  expect(m)                 -> (ok, bytes): zlib's raw inflate reaches the end of the stream and gives exactly ISIZE bytes
"""
import struct
import zlib

import numpy as np

import bam_util as B

LEVELS = (0, 1, 6, 9)
STRATEGIES = (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE))
SIZES = (0, 1, 2, 257, 0xff00, 65535, 65536)
HEAD = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"


class Member:
    def __init__(self, payload, isize, data=None, label=""):
        self.payload, self.isize, self.data, self.label = payload, isize, data, label

    def bytes(self):
        crc = zlib.crc32(self.data) & 0xffffffff if self.data is not None else 0
        return HEAD + struct.pack("<H", len(self.payload) + 25) + self.payload + struct.pack("<II", crc, self.isize)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for i in range(0, len(data), flush_every):
        out += c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def payload_kinds(rng):
    """name -> a function of the size: the bytes to compress"""
    recs = b"".join(B.random_records(rng, 700))
    assert len(recs) >= 65536
    noise = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    skew = rng.choice(16, 32768, p=np.arange(16, 0, -1) / 136.0).astype(np.uint8).tobytes()   # compressible by Huffman alone
    kinds = {"records": lambda n: recs[:n], "noise": lambda n: noise[:n], "period32768": lambda n: (skew * 3)[:n]}
    for p in (1, 2, 3, 4):
        unit = bytes(rng.integers(0, 256, p, dtype=np.uint8).tolist())
        kinds["period%d" % p] = lambda n, unit=unit: (unit * (n // len(unit) + 1))[:n]
    return kinds


def corpus(rng):
    """-> ([Member], skipped labels): a member whose BSIZE would not fit 16 bits cannot exist and is skipped."""
    out, skipped = [], []
    for kind, make in payload_kinds(rng).items():
        for size in SIZES:
            data = make(size)
            for level in LEVELS:
                for sname, strat in STRATEGIES:
                    label = "%s/%d/L%d/%s" % (kind, size, level, sname)
                    comp = deflate(data, level, strat)
                    if len(comp) + 26 > 65536:
                        skipped.append(label)
                        continue
                    out.append(Member(comp, len(data), data, label))
    data = payload_kinds(rng)["records"](0xff00)
    out.append(Member(deflate(data, 6, flush_every=1000), len(data), data, "records/flushed"))
    out.append(Member(deflate(data, 9, mem_level=1), len(data), data, "records/memlevel1"))   # small symbol buffer: many blocks
    return out, skipped


def first_block_type(m):
    return (m.payload[0] >> 1) & 3


def damaged(rng, members, n):
    out = []
    while len(out) < n:
        m = members[int(rng.integers(0, len(members)))]
        p = bytearray(m.payload)
        r = rng.random()
        if r < 0.8 or len(p) < 2:
            k = int(rng.integers(0, len(p) * 8))
            if r < 0.4:
                k = min(k, int(rng.integers(0, 200)))      # half of the flips in the block's header and code lengths
            p[k >> 3] ^= 1 << (k & 7)
            how = "bit %d" % k
        elif r < 0.9:
            del p[-1]
            how = "cut"
        else:
            p.append(int(rng.integers(0, 256)))
            how = "extended"
        if len(p) + 26 > 65536:
            continue
        out.append(Member(bytes(p), m.isize, None, m.label + " " + how))
    return out


def expect(m):
    """(ok, bytes or None) by zlib: the raw inflate reaches the end of the stream and gives exactly ISIZE bytes."""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(m.payload, m.isize + 1)
    except zlib.error:
        return False, None
    ok = d.eof and len(got) == m.isize
    return ok, got if ok else None


def walk(file_bytes):
    """The block table by a Python walk of headers and footers -> (blk_off, out_off)."""
    blk, out, p, o = [0], [0], 0, 0
    while p < len(file_bytes):
        size = struct.unpack_from("<H", file_bytes, p + 16)[0] + 1
        o += struct.unpack_from("<I", file_bytes, p + size - 4)[0]
        p += size
        blk.append(p), out.append(o)
    return np.array(blk, np.int64), np.array(out, np.int64)


GUARD = 4096


def run_host(lib, members, first=None, count=None):
    """sbgpu_bgzf_inflate_host over `members` laid out as one file, the output between guards of 0xA5 -> (status, the
    per-member output bytes, guards intact)."""
    file = np.frombuffer(b"".join(m.bytes() for m in members), np.uint8)
    blk, off = walk(file.tobytes())
    first = 0 if first is None else first
    count = len(members) - first if count is None else count
    buf = np.full(GUARD + int(off[-1]) + GUARD, 0xA5, np.uint8)
    status = np.full(max(count, 1), 0xEE, np.uint8)
    rc = lib.sbgpu_bgzf_inflate_host(file.ctypes.data, file.size, blk.ctypes.data, off.ctypes.data, first, count,
                                     buf.ctypes.data + GUARD, status.ctypes.data)
    assert rc == 0
    return status[:count], split_output(buf, off), guards_intact(buf)


def split_output(buf, off):
    return [buf[GUARD + int(off[k]):GUARD + int(off[k + 1])].tobytes() for k in range(len(off) - 1)]


def guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all())


def interleave(good, bad):
    """good[0] bad[0] good[1] bad[1] ... good[k]: every damaged member between two undamaged ones."""
    out = [good[0]]
    for k, m in enumerate(bad):
        out += [m, good[(k + 1) % len(good)]]
    return out

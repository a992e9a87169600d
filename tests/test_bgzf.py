"""BGZF on the host: the block table (sbgpu_bgzf_index_host) and the inflate (sbgpu_bgzf_inflate_host) against Python's zlib
-- the library the reference links -- on a corpus that holds every block type, and on damaged members, where the library must
refuse exactly what zlib refuses and never write outside the member's own output."""
import os
import struct

import numpy as np
import pytest

import bam_util as B
import bgzf_util as Z


@pytest.fixture(scope="module")
def lib():
    from strawberry_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus(np.random.default_rng(20))


def test_corpus_holds_what_it_says(corpus):
    members, skipped = corpus
    data = b"".join(B.random_records(np.random.default_rng(1), 50))
    assert Z.Member(Z.deflate(data), len(data), data).bytes() == B._bgzf_block(data)            # the framing of bam_util
    assert {Z.first_block_type(m) for m in members} == {0, 1, 2}                                # stored, fixed, dynamic
    for label in skipped:   # BSIZE cannot hold more than 65536 bytes: only what does not compress, at the two largest sizes
        kind, size, level, _ = label.split("/")
        assert int(size) >= 65535 and (level == "L0" or kind == "noise"), label
    assert len(members) + len(skipped) == 7 * 7 * 4 * 4 + 2 and len(skipped) <= 7 * 2 * 4 + 3 * 2 * 4   # level 0; noise at the others
    flushed = [m for m in members if m.label == "records/flushed"][0]
    assert flushed.payload.count(b"\x00\x00\xff\xff") >= 60                                     # many blocks, empty stored ones among them
    assert any(m.isize == 65536 and m.label.startswith("period32768") for m in members)        # the longest distance
    for m in members:
        ok, got = Z.expect(m)
        assert ok and got == m.data, m.label


def test_index_equals_a_walk_of_the_headers(lib, corpus):
    members, _ = corpus
    file = b"".join(m.bytes() for m in members[:300]) + B._bgzf_block(b"")
    blk, off = Z.walk(file)
    n = len(blk) - 1
    f = np.frombuffer(file, np.uint8)

    def index(buf, cap=n):
        a, b = np.full(cap + 2, -7, np.int64), np.full(cap + 2, -7, np.int64)
        arr = np.frombuffer(bytes(buf), np.uint8)
        r = lib.sbgpu_bgzf_index_host(arr.ctypes.data, arr.size, a.ctypes.data, b.ctypes.data, cap)
        return r, a, b
    r, a, b = index(file)
    assert r == n == 301
    np.testing.assert_array_equal(a[:n + 1], blk)
    np.testing.assert_array_equal(b[:n + 1], off)
    assert a[n + 1] == -7 and b[n + 1] == -7
    assert off[-1] == off[-2]                                         # the EOF marker: an ordinary entry without output
    from strawberry_amd import bam
    tb, to = bam.bgzf_index(file)
    np.testing.assert_array_equal(tb, blk), np.testing.assert_array_equal(to, off)
    third = int(blk[3])

    def patched(at, value):
        x = bytearray(file)
        x[at:at + len(value)] = value
        return x
    bad = {"magic": patched(third, b"\x1f\x8c"), "method": patched(third + 2, b"\x07"), "no FEXTRA": patched(third + 3, b"\x00"),
           "XLEN 8": patched(third + 10, b"\x08\x00"), "subfield id": patched(third + 12, b"BD"), "subfield length": patched(third + 14, b"\x03\x00"),
           "cut in a header": file[:third + 10], "cut in a payload": file[:third + 40], "cut in the footer": file[:int(blk[4]) - 2]}
    for why, buf in bad.items():
        assert index(buf)[0] == -1, why
        assert lib.sbgpu_last_error(), why
    assert index(file, cap=n - 1)[0] == -1
    assert index(file, cap=n)[0] == n
    # FLG may carry other bits beside FEXTRA, MTIME / XFL / OS are not looked at: check_header's tests and no others
    assert index(patched(third + 3, b"\x1c"))[0] == n and index(patched(third + 4, b"\x01\x02\x03\x04\x05\x06"))[0] == n
    # an ISIZE word beyond 65536 is refused
    assert index(patched(int(blk[4]) - 4, struct.pack("<I", 65537)))[0] == -1
    assert index(b"")[0] == 0


@pytest.mark.parametrize("threads", ["1", "16"])
def test_inflate_equals_zlib_on_the_corpus(lib, corpus, threads, monkeypatch):
    monkeypatch.setenv("SBGPU_HOST_THREADS", threads)
    members, _ = corpus
    status, got, guards = Z.run_host(lib, members)
    assert guards
    for m, s, g in zip(members, status, got):
        assert s == 0 and g == m.data, (m.label, s)
    # sub-ranges: the members of the call and no others are written, status[0 .. n_blocks) is theirs
    for first, count in ((0, 1), (5, 0), (17, 40), (len(members) - 3, 3), (100, 333)):
        status, got, guards = Z.run_host(lib, members, first, count)
        assert guards and len(status) == count and (status == 0).all()
        for k, (m, g) in enumerate(zip(members, got)):
            assert g == (m.data if first <= k < first + count else b"\xa5" * m.isize), (first, count, m.label)


def test_damaged_members_are_refused_exactly_where_zlib_refuses(lib, corpus):
    rng = np.random.default_rng(21)
    members, _ = corpus
    small = [m for m in members if m.isize <= 257] + [m for m in members if m.isize > 257][::7]
    bad = Z.damaged(rng, small, 2400)
    good = [m for m in members if 0 < m.isize <= 0xff00][::5]
    laid = Z.interleave(good, bad)
    status, got, guards = Z.run_host(lib, laid)
    assert guards
    n_ok = 0
    for k, (m, s, g) in enumerate(zip(laid, status, got)):
        if k % 2 == 0:
            assert s == 0 and g == m.data, ("neighbour", m.label)         # undamaged members on both sides of every damaged one
            continue
        ok, want = Z.expect(m)
        assert (s == 0) == ok, (m.label, int(s), ok)
        assert 0 <= s <= 7
        if ok:
            assert g == want, m.label
            n_ok += 1
    assert 20 < n_ok < 2000 and len(set(status[1::2].tolist())) >= 7, (n_ok, sorted(set(status.tolist())))   # both verdicts, many reasons


def test_an_isize_that_lies_is_refused(lib, corpus):
    members, _ = corpus
    picks = [m for m in members if m.isize in (2, 257, 0xff00)][::9]
    assert len(picks) > 20
    for delta in (-1, 1):
        laid = Z.interleave(picks, [Z.Member(m.payload, m.isize + delta, None, m.label) for m in picks])
        status, got, guards = Z.run_host(lib, laid)
        assert guards and (status[0::2] == 0).all() and (status[1::2] == 7).all()     # SBGPU_BGZF_ESIZE
        assert all(g == m.data for m, g in zip(laid[0::2], got[0::2]))


def test_bad_arguments(lib):
    one = np.zeros(8, np.int64)
    byte = np.zeros(8, np.uint8)
    assert lib.sbgpu_bgzf_inflate_host(None, 0, None, None, 0, 0, None, None) == 0
    assert lib.sbgpu_bgzf_inflate_host(None, 10, one.ctypes.data, one.ctypes.data, 0, 1, byte.ctypes.data, byte.ctypes.data) == -1
    assert lib.sbgpu_bgzf_inflate_host(byte.ctypes.data, 8, one.ctypes.data, one.ctypes.data, -1, 1, byte.ctypes.data, byte.ctypes.data) == -1
    assert lib.sbgpu_bgzf_index_host(byte.ctypes.data, 8, None, one.ctypes.data, 4) == -1
    # a table that points outside the file is a status, not a read
    blk, off = np.array([0, 4000], np.int64), np.array([0, 10], np.int64)
    st = np.zeros(1, np.uint8)
    assert lib.sbgpu_bgzf_inflate_host(byte.ctypes.data, 8, blk.ctypes.data, off.ctypes.data, 0, 1, byte.ctypes.data, st.ctypes.data) == 0
    assert st[0] == 6


def test_split_header_reads_the_files_of_bam_util(tmp_path):
    from strawberry_amd import bam
    rng = np.random.default_rng(22)
    for n in (0, 1, 40, 1500):
        path = str(tmp_path / ("t%d.bam" % n))
        B.write_bam(path, B.REFS, B.random_records(rng, n) + B.garbage_records(rng, n // 4))
        refs, rec = B.read_bam_records(path)
        got_refs, got = bam.split_header(open(path, "rb").read())
        assert got_refs == refs
        np.testing.assert_array_equal(got, rec)
    with pytest.raises(Exception):
        bam.split_header(B.bgzf_compress(b"BAM\1\x10\0\0\0"))
    x = bytearray(open(path, "rb").read())
    x[600] ^= 0x10
    with pytest.raises(Exception):
        bam.split_header(bytes(x))

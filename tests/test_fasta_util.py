"""The files tests/fasta_util.py generates for the device form's thresholds have the properties they are named for -- asserted on
the bytes and on the Python restatement alone, with the tile and the scan round taken from sbgpu_fasta_limits.  No GPU."""
import pytest

import fasta_util as FU


@pytest.fixture(scope="module")
def LIM():
    from strawberry_amd import fasta
    return fasta.limits()


def test_filler_and_wrapped_file_have_their_sizes(LIM):
    T = LIM["tile"]
    for n in list(range(2, 200)) + [T - 4, T - 3, T - 2, 2 * T - 4]:
        f = FU.filler(n)
        assert len(f) == n and f.endswith(b"\n") and b"\n\n" not in f and not f.startswith(b"\n")
    for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        for width in (60, 59):
            d = FU.wrapped_file(n, width)
            r = FU.restate(d)
            assert len(d) == n and len(r["names"]) == 1 and r["line_bases"] == [width] and r["flags"] == [0]


def test_headers_stand_where_the_names_say(LIM):
    T = LIM["tile"]
    for pos in (T - 1, T, T + 1, 2 * T - 1):
        d = FU.header_at(pos, b">edge of tile\n")
        assert d[pos:pos + 1] == b">" and d[pos - 1:pos] == b"\n" and FU.restate(d)["names"] == [b"a", b"edge"]
    assert (T - 1) % T == T - 1 and (2 * T - 1) % T == T - 1                      # '>' is a tile's last byte
    d = FU.header_at(T - 5, b">edge\n")
    assert d[T:T + 1] == b"\n" and d[T - 5:T] == b">edge"                         # the header's '\n' is a tile's first byte
    d = FU.header_at(T - 5, b">straddling_name x\n")
    assert d[T - 5:T + 11] == b">straddling_name" and FU.restate(d)["names"][1] == b"straddling_name"
    d = FU.header_at(T - 4, b">cr\r\n")
    assert d[T - 1:T + 1] == b"\r\n" and FU.restate(d)["offset"][1] == T + 1
    for ln in (T + 100, 2 * T + 100):
        d = FU.header_at(100, b">n " + b"d" * ln + b"\n")
        start, end, term = [x for x in FU.lines_of(d) if x[0] == 100][0]
        assert d[start:start + 1] == b">" and end - start == ln + 3 > ln and ln + 3 < LIM["max_header"]
    assert 2 * T + 100 > 2 * T and T + 100 > T


def test_crlf_pair_is_split_across_tiles(LIM):
    T = LIM["tile"]
    for pos in (T, 2 * T):
        d = FU.crlf_split_at(pos)
        assert d[pos - 1:pos + 1] == b"\r\n" and pos % T == 0
        r = FU.restate(d)
        assert r["flags"] == [0] and r["line_bases"] == [60] and r["line_width"] == [62]


def test_unwrapped_and_small_contigs(LIM):
    T = LIM["tile"]
    for nl in (True, False):
        d = FU.unwrapped(3 * T + 17, nl)
        r = FU.restate(d)
        assert len(r["seqs"][1]) == 3 * T + 17 >= 3 * T and r["flags"] == [0, 0] and d.endswith(b"\n") == nl and r["lines"] == 4
    S = LIM["scan_tile"]
    for n in (63, 64, 65, S - 1, S, S + 1):
        assert len(FU.restate(FU.small_contigs(n))["names"]) == n
    d = FU.many_contigs(5000, seed=11)
    r = FU.restate(d)
    heads = [o for o in r["offset"]]
    assert len(heads) == 5000 and all(1 <= len(s) <= 100 for s in r["seqs"])
    assert max(sum(1 for o in heads if t * T <= o < (t + 1) * T) for t in range(len(d) // T)) > 64     # a tile with more than 64 headers


def test_large_files_have_their_tile_counts(LIM):
    T, S, G = LIM["tile"], LIM["scan_tile"], LIM["grid_cap"]
    for delta in (-1, 0, 1):
        n = (S + delta) * T
        d = FU.blocks_file(n)[:n - 8] + b"\n>last\nA"
        assert len(d) == n and -(-len(d) // T) == S + delta and d.startswith(b">b00000\n")
    n = 2 * G * T + 5 * T + 11
    assert len(FU.blocks_file(n)) >= n and -(-n // T) > 2 * G
    block = FU.blocks_file(1)
    r = FU.restate(block)
    assert r["flags"] == [0] and len(r["seqs"][0]) == 100003 and r["line_bases"] == [60]


def test_refused_cases_are_refused_where_they_say():
    for name, (d, at) in FU.refused_cases().items():
        with pytest.raises(FU.LeadingText) as e:
            FU.restate(d)
        assert e.value.offset == at, name

"""The FASTA reader's host form (sbgpu_fasta_read_host) against the rule restated in Python (tests/fasta_util.py): every array,
flag and name, the packed bytes, the .fai text, the index arithmetic, fetch and find.  No GPU."""
import os

import numpy as np
import pytest

import fasta_util as FU

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = FU.cpu_cases()


def check_against_restatement(g, data):
    """a FastaGenome of `data` holds what the restatement says; -> the restatement"""
    r = FU.restate(data)
    assert g.names == r["names"]
    assert g.length.tolist() == [len(s) for s in r["seqs"]]
    assert g.offset.tolist() == r["offset"]
    assert g.line_bases.tolist() == r["line_bases"] and g.line_width.tolist() == r["line_width"]
    assert g.flags.tolist() == r["flags"]
    assert g.seq_off.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in r["seqs"]])]).tolist()
    for c, s in enumerate(r["seqs"]):
        assert g.sequence(c) == s, c
    info = g.info
    assert (info["bytes"], info["lines"], info["contigs"], info["bases"]) == (len(data), r["lines"], len(r["names"]), sum(len(s) for s in r["seqs"]))
    assert [info[k] for k in ("empty", "ragged", "duplicate", "noname")] == [sum(1 for f in r["flags"] if f & b) for b in (1, 2, 4, 8)]
    lens = [len(s) for s in r["seqs"]]
    assert (info["longest"], info["longest_contig"]) == ((max(lens), lens.index(max(lens))) if lens else (0, -1))
    return r


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_form_is_the_rule(name):
    from strawberry_amd.fasta import read_fasta
    data = CASES[name]
    g = read_fasta(data)
    r = check_against_restatement(g, data)
    assert not g.on_device and g.info["device"] == -1
    # the index arithmetic, for every base of every contig that is neither EMPTY nor RAGGED
    for c, seq in enumerate(r["seqs"]):
        if r["flags"][c] & (FU.EMPTY | FU.RAGGED):
            continue
        off, lb, lw = int(g.offset[c]), int(g.line_bases[c]), int(g.line_width[c])
        for p in range(1, len(seq) + 1):
            assert data[off + ((p - 1) // lb) * lw + (p - 1) % lb] == seq[p - 1], (c, p)


def test_the_cases_cover_every_flag():
    flags = {n: FU.restate(d)["flags"] for n, d in CASES.items()}
    assert all(any(f & FU.RAGGED for f in flags[n]) for n in CASES if n.startswith("ragged_"))
    assert not any(f & FU.RAGGED for n in CASES if not n.startswith("ragged_") and n != "many_small" for f in flags[n])
    assert all(any(f & FU.EMPTY for f in flags[n]) for n in CASES if n.startswith("empty_"))
    assert flags["noname"] == [FU.NONAME, FU.NONAME | FU.DUPLICATE, 0]
    assert flags["duplicate"] == [0, 0, FU.DUPLICATE] and flags["duplicate_by_case"] == [0, FU.DUPLICATE, FU.DUPLICATE]
    assert flags["last_full_line_other_terminator"] == [0] and flags["lone_cr_in_line"] == [0, 0]


@pytest.mark.parametrize("name", sorted(FU.refused_cases()))
def test_text_in_front_of_the_first_header_is_refused_with_its_offset(name):
    from strawberry_amd import _lib
    from strawberry_amd.fasta import read_fasta
    data, at = FU.refused_cases()[name]
    with pytest.raises(FU.LeadingText) as e:
        FU.restate(data)
    assert e.value.offset == at
    with pytest.raises(_lib.SbgpuError) as e:
        read_fasta(data)
    assert "(-1)" in str(e.value) and "offset %d" % at in str(e.value)


def test_fai_text():
    from strawberry_amd import _lib
    from strawberry_amd.fasta import read_fasta
    assert read_fasta(CASES["lf"]).fai_text() == "chr1\t150\t12\t60\t61\nchr2\t120\t171\t60\t61\n"
    assert read_fasta(CASES["crlf"]).fai_text() == "chr1\t150\t13\t60\t62\nchr2\t120\t176\t60\t62\n"
    assert read_fasta(CASES["no_final_newline"]).fai_text() == "a\t150\t3\t60\t61\n"
    assert read_fasta(b">a\nACGT").fai_text() == "a\t4\t3\t4\t4\n"                    # a first line without a terminator
    assert read_fasta(CASES["empty_header_header"]).fai_text() == "b\t70\t6\t60\t61\n"  # EMPTY contigs are left out
    assert read_fasta(CASES["zero_bytes"]).fai_text() == ""
    for name, d in CASES.items():
        r = FU.restate(d)
        if not any(f & (FU.RAGGED | FU.NONAME) and not f & FU.EMPTY for f in r["flags"]):
            assert read_fasta(d).fai_text() == FU.fai_of(r), name
    for name, word in (("ragged_long_last", "'a'"), ("noname", "no name")):
        with pytest.raises(_lib.SbgpuError) as e:
            read_fasta(CASES[name]).fai_text()
        assert "(-6)" in str(e.value) and word in str(e.value) and "contig 0" in str(e.value)


def test_fai_of_the_golden_genome():
    """tools/make_e2e_golden.py wrote this line for the reference to read"""
    from strawberry_amd.fasta import read_fasta
    path = os.path.join(HERE, "golden", "e2e_toy_bias", "genome.fa")
    g = read_fasta(path)
    assert g.fai_text() == "chr1\t%d\t6\t60\t61\n" % int(g.length[0])
    from strawberry_amd.binseq import read_fasta as old
    assert g.sequence("chr1") == old(path)["chr1"]


def test_fetch_windows():
    from strawberry_amd import _lib
    from strawberry_amd.fasta import read_fasta
    g = read_fasta(CASES["short_last_line"])
    r = FU.restate(CASES["short_last_line"])
    for c, s in enumerate(r["seqs"]):
        n = len(s)
        assert g.fetch(c, 1, 1) == s[:1] and g.fetch(c, n, 1) == s[-1:] and g.fetch(c, 1, n) == s and g.fetch(c, 7, n - 10) == s[6:n - 4]
        assert g.fetch(c, n + 1, 0) == b"" and g.fetch(c, 3, 0) == b""
        for start, ln in ((0, 1), (n + 1, 1), (n, 2), (1, n + 1), (-1, 1), (n + 2, 0)):
            with pytest.raises(_lib.SbgpuError):
                g.fetch(c, start, ln)
    with pytest.raises(_lib.SbgpuError):
        g.fetch(2, 1, 1)


def test_find():
    from strawberry_amd.fasta import read_fasta
    g = read_fasta(CASES["duplicate_by_case"])
    assert g.find("chr1") == 0 and g.find(b"CHR1") == 0 and g.find("cHr1") == 0 and g.find("chr2") == -1 and g.find("") == -1
    g = read_fasta(CASES["noname"])
    assert g.find("") == 0 and g.find("x") == 2 and g.find("X") == 2
    g = read_fasta(CASES["lf"])
    assert g.find("chr2") == 1 and g.find("chr1 first") == -1
    assert g.index[1] == (b"chr2", 120, 171, 60, 61)


def test_limits_and_bad_arguments():
    import ctypes as C
    from strawberry_amd import _lib, fasta
    lim = fasta.limits()
    assert lim["tile"] % 1024 == 0 and lim["scan_tile"] >= 64 and lim["grid_cap"] >= 1 and lim["max_header"] > 2 * lim["tile"] and lim["max_contigs"] > lim["scan_tile"]
    L = _lib.load()
    h = C.c_void_p()
    assert L.sbgpu_fasta_read_host(None, 4, C.byref(h)) == -1 and L.sbgpu_fasta_read_host(None, 0, None) == -1
    assert L.sbgpu_fasta_info(None, None) == -1 and L.sbgpu_fasta_fetch(None, 0, 1, 1, None) == -1
    L.sbgpu_fasta_destroy(None)

"""The GTF reader's host form (sbgpu_gtf_read_host through strawberry_amd.gtf) against the reference's own order on the goldens,
against what each rule of include/sbgpu.h says on one hand-written file per rule, and against the independent restatement of
tests/gtf_util.py on all of them and on seeded random files.  No GPU."""
import glob
import os

import numpy as np
import pytest

import e2e_util
import gtf_util as U
from strawberry_amd import _lib, gtf

GOLDENS = sorted(d for d in glob.glob(os.path.join(e2e_util.HERE, "golden", "e2e_toy*")) if d != e2e_util.E2E_ASSEMBLY)
HAND = U.hand_files()


def _read(name):
    data, refs = HAND[name]
    g = gtf.read_gtf(data, ref_names=refs)
    U.assert_matches(g, U.restate(data, refs))
    return g


def _tx(g):
    return [[t for t, _, _, _ in r["isoforms"]] for r in g.rows()]


def test_there_are_ten_goldens():
    assert len(GOLDENS) == 10 and all(os.path.exists(os.path.join(d, "toy.gtf")) for d in GOLDENS)


@pytest.mark.parametrize("directory", GOLDENS, ids=os.path.basename)
def test_goldens_in_the_reference_order(directory):
    data = open(os.path.join(directory, "toy.gtf"), "rb").read()
    g = gtf.read_gtf(data)
    U.assert_matches(g, U.restate(data))
    ordered = e2e_util.load(directory)[0]   # the reference's locus and isoform order (ctx.tsv)
    strands, chroms = e2e_util.gene_strands(directory), e2e_util.gene_chroms(directory)
    rows = g.rows()
    assert [r["gene_id"].decode() for r in rows] == list(ordered)
    for l, r in enumerate(rows):
        gene = r["gene_id"].decode()
        assert [(t.decode(), e) for t, _, _, e in r["isoforms"]] == [(t, list(e)) for t, e in ordered[gene]]
        assert r["strand"] == {"+": 1, "-": 2}.get(strands[gene], 0)
        assert g.chrom[r["chrom"]].decode() == chroms[gene]
        exons = sorted({e for _, ex in ordered[gene] for e in ex})
        s0, s1 = int(g.seg_off[l]), int(g.seg_off[l + 1])
        assert list(zip(g.seg_left[s0:s1].tolist(), g.seg_right[s0:s1].tolist())) == e2e_util.disjoint_segments(exons)
        assert [n for _, _, n, _ in r["isoforms"]] == [sum(b - a + 1 for a, b in e) for _, e in ordered[gene]]


def test_lines():
    g = _read("comment_short_tabs")
    assert g.line_status.tolist() == [U.SKIP, U.SKIP, U.SKIP, U.FIELDS, U.OK]
    assert g.info["lines"] == 5 and g.info["lines_skip"] == 3 and g.info["lines_fields"] == 1 and g.info["loci"] == 1
    for name in ("crlf", "no_final_newline"):
        g = _read(name)
        assert g.line_status.tolist() == [U.OK, U.OK] and g.rows()[0]["isoforms"] == [(b"t", 1, 202, [(100, 200), (300, 400)])]
    g = _read("empty")
    assert g.info["lines"] == 0 and g.n_loci == 0 and g.n_iso == 0 and g.iso_off.tolist() == [0] and g.chrom == []
    assert _read("only_comments").info["lines_skip"] == 2 and _read("only_comments").n_loci == 0
    assert _read("only_newlines").line_status.tolist() == [U.SKIP] * 3
    assert _read("hash_behind_tabs").line_status.tolist() == [U.SKIP, U.OK]


def test_feature_types():
    g = _read("types")
    assert g.line_status.tolist() == [U.OK, U.OK, U.OK, U.OTHER, U.OTHER, U.OTHER, U.OTHER, U.OK]
    assert _tx(g) == [[b"t0", b"t1", b"t2", b"t7"]]


def test_coordinates():
    g = _read("coords")
    #                                 0        ""       12x   x12      2^31-1 2^31     huge     " 7"     -7       end < start
    assert g.line_status.tolist() == [U.COORD, U.COORD, U.OK, U.COORD, U.OK, U.COORD, U.COORD, U.COORD, U.COORD, U.OK]
    assert g.rows()[0]["isoforms"][0][3] == [(5, 2 ** 31 - 1)]   # 12-20, 5-(2^31-1) and 800-900 overlap: one exon
    assert g.info["merged_exons"] == 2 and int(g.iso_len[0]) == 2 ** 31 - 5


def test_a_numeric_score_is_read():
    g = _read("score")
    assert g.line_status.tolist() == [U.OK] * 3 and g.info["exons"] == 3


def test_strand():
    g = _read("strand")
    assert sorted((t, s) for r in g.rows() for t, s, _, _ in r["isoforms"]) == [(b"a", 0), (b"b", 0), (b"c", 0), (b"d", 1), (b"e", 2)]


def test_attributes():
    g = _read("attributes")
    S = g.line_status.tolist()
    assert S == [0, 0, 0, 0, 0, 0, 0, 0, 0, U.NO_TRANSCRIPT, U.NO_TRANSCRIPT, U.NO_GENE, U.NO_GENE, U.NO_TRANSCRIPT, 0, 0, U.NO_TRANSCRIPT, 0]
    got = {r["isoforms"][0][0]: (r["gene_id"], r["gene_name"]) for r in g.rows()}
    assert got[b"bare"] == (b"quoted", b"n 1")               # quoted and bare values
    assert got[b"t2"] == (b"g2", b"")                        # a key inside a quoted value is not one
    assert got[b"t3"] == (b"right", b"")                     # ref_gene_id is not gene_id
    assert got[b"t4"] == (b"upper", b"N")                    # keys without case
    assert got[b"t5"] == (b"g5", b"") and got[b"t6"] == (b"g6", b"")   # no final ';'; transcript_id in front
    assert got[b"t7"] == (b"two blanks", b"bare name ")      # a bare value runs to the ';'
    assert got[b"t8"] == (b"g8", b"")                        # gene_idx is not gene_id
    assert got[b"unterminated"] == (b"g9", b"")
    assert got[b"t15"] == (b"g15", b"")                      # "hidden" stands inside quotes
    assert got[b"t16"] == (b'transcript_id "t16"', b"n16")   # every key is looked up in the original text
    assert (b"g\xc3\x83\xc2\xa9\x00z", b"") in got.values()  # bytes >= 0x80 and a NUL are bytes


def test_names_of_255_and_256_bytes():
    g = _read("name_255")
    assert g.gene_id == [b"g" * 255] and g.transcript_id == [b"t" * 255] and g.gene_name == [b"n" * 255] and g.chrom == [b"c" * 255]
    for which in range(4):
        n = [255] * 4
        n[which] = 256
        line = U._x(chrom="c" * n[0], attrs='gene_id "%s"; transcript_id "%s"; gene_name "%s";' % ("g" * n[1], "t" * n[2], "n" * n[3]))
        with pytest.raises(_lib.SbgpuError, match="255 bytes"):
            gtf.read_gtf(line + b"\n")
    assert gtf.read_gtf(U._x(kind="CDS", attrs='gene_id "%s"; transcript_id "t";' % ("g" * 300)) + b"\n").line_status.tolist() == [U.OTHER]


def test_transcripts():
    g = _read("scattered")
    assert [(r["gene_id"], r["isoforms"]) for r in g.rows()] == [(b"h", [(b"b", 1, 202, [(100, 200), (300, 400)])]),
                                                                  (b"g", [(b"a", 1, 253, [(100, 200), (500, 600), (900, 950)])])]
    g = _read("merges")
    assert g.rows()[0]["isoforms"] == [(b"t", 1, 400, [(100, 400), (402, 500)])] and g.info["merged_exons"] == 5
    g = _read("one_tx_two_strands_two_chroms")
    assert g.info["transcripts"] == 3 and g.chrom == [b"chr1", b"chr2"]
    assert [(r["chrom"], [(s, e) for _, s, _, e in r["isoforms"]]) for r in g.rows()] == [
        (0, [(1, [(100, 200), (700, 800)]), (2, [(300, 400)])]), (1, [(1, [(500, 600)])])]


def test_order():
    assert _tx(_read("identical_keep_file_order")) == [[b"t3", b"t1", b"t2"]]
    assert _tx(_read("prefix_first")) == [[b"first", b"short", b"long"]]
    g = _read("chroms_first_appearance")
    assert g.chrom == [b"chrB", b"chrA", b"chrZ"] and [r["gene_id"] for r in g.rows()] == [b"gb", b"ga", b"gz"]
    g = _read("chroms_table")
    assert g.chrom == [b"chrA", b"CHRB", b"chrC", b"chra"] and g.info["dropped_transcripts"] == 1 and g.info["chromosomes"] == 4
    assert [(r["chrom"], r["gene_id"]) for r in g.rows()] == [(0, b"ga"), (1, b"gb")]
    g = _read("interleaved_genes")
    assert [(r["gene_id"], r["left"], r["right"]) for r in g.rows()] == [(b"g1", 100, 300), (b"g2", 150, 310)]
    assert _tx(g) == [[b"a", b"c"], [b"b", b"d"]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_random_files(seed):
    data = U.random_gtf(seed)
    g = gtf.read_gtf(data)
    assert g.n_loci == 300 and g.info["merged_exons"] > 0
    U.assert_matches(g, U.restate(data))
    refs = ["chr2", "CHR1", "chrUn"]
    g = gtf.read_gtf(data, ref_names=refs)
    assert g.info["dropped_transcripts"] > 0
    U.assert_matches(g, U.restate(data, refs))


def test_clusters_ascend_and_arrays_are_the_annotation():
    g = gtf.read_gtf(U.random_gtf(4, n_genes=80))
    key = list(zip(g.cluster_ref.tolist(), g.cluster_left.tolist()))
    assert key == sorted(key)
    an, cl = g.annotation()
    assert an.n_loci == g.n_loci == cl.n_clusters
    assert np.all(g.exon_left <= g.exon_right)


def test_bad_arguments_are_refused_by_their_text():
    L = _lib.load()
    import ctypes as C
    h = C.c_void_p()
    assert L.sbgpu_gtf_read_host(None, 5, None, C.byref(h)) == _lib.SBGPU_EINVAL and b"sbgpu_gtf_read_host" in L.sbgpu_last_error()
    o = _lib.sbgpu_gtf_opts_t()
    o.n_ref, o.hash_bits = 2, 0
    assert L.sbgpu_gtf_read_host(None, 0, C.byref(o), C.byref(h)) == _lib.SBGPU_EINVAL and b"table" in L.sbgpu_last_error()
    assert L.sbgpu_gtf_info(None, None) == _lib.SBGPU_EINVAL
    lim = gtf.limits()
    assert lim["tile_lines"] == 64 and lim["max_name"] == 255 and lim["stage_limit"] < 64 * 1024 and lim["max_line"] >= lim["stage_limit"]

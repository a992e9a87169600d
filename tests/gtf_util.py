"""The GTF reader's rule (include/sbgpu.h, sbgpu_gtf_*) a second time, for the tests: plain Python over str.split, a regex,
dicts and sorted() -- nothing of the library's code --, seeded generators of annotation files, and the comparison of a
GtfAnnotation with the restatement's result."""
import re

import numpy as np

from e2e_util import disjoint_segments

OK, SKIP, FIELDS, OTHER, COORD, NO_TRANSCRIPT, NO_GENE = range(7)
SPACES = b" \t\n\v\f\r"


def _lower(b):
    return bytes(c + 32 if 65 <= c <= 90 else c for c in b)


def attribute(col, key):
    """GffLine::extractAttr on the column's original bytes -> the value (bytes), b"" when the key is missing."""
    in_str, n, k = False, len(col), len(key)
    for p in range(n):
        if col[p:p + 1] == b'"':
            in_str = not in_str
            continue
        if in_str or not (p == 0 or col[p - 1:p] in (b" ", b";")):
            continue
        if _lower(col[p:p + k]) != key or not (p + k == n or col[p + k:p + k + 1] == b" "):
            continue
        v = p + k
        while v < n and col[v:v + 1] == b" ":
            v += 1
        if v < n and col[v:v + 1] == b'"':
            m = re.match(rb'[^";]*', col[v + 1:])
        else:
            m = re.match(rb'[^;]*', col[v:])
        return m.group(0)
    return b""


def parse_line(line):
    """-> (status, fields) for one line without its newline; fields: (chrom, left, right, strand, gene_id, transcript_id, gene_name)."""
    if line.endswith(b"\r"):
        line = line[:-1]
    if len(line) < 10 or line.lstrip(SPACES)[:1] == b"#":
        return SKIP, None
    f = line.split(b"\t", 8)
    if len(f) < 9:
        return FIELDS, None
    kind = _lower(f[2])
    if b"utr" in kind or b"exon" not in kind:
        return OTHER, None
    coords = []
    for field in (f[3], f[4]):
        m = re.match(rb"[0-9]+", field)
        v = int(m.group(0)) if m else 0
        if not 1 <= v <= 2 ** 31 - 1:
            return COORD, None
        coords.append(v)
    strand = {b"+": 1, b"-": 2}.get(f[6][:1], 0)
    tx, gene, gname = attribute(f[8], b"transcript_id"), attribute(f[8], b"gene_id"), attribute(f[8], b"gene_name")
    if not tx:
        return NO_TRANSCRIPT, None
    if not gene:
        return NO_GENE, None
    if max(len(f[0]), len(tx), len(gene), len(gname)) > 255:
        raise ValueError("a name of more than 255 bytes")
    return OK, (f[0], min(coords), max(coords), strand, gene, tx, gname)


def split_lines(data):
    lines = bytes(data).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def restate(data, ref_names=None):
    """The whole rule -> dict with `status` (uint8 per line), `info`, `chrom` (names per id) and `loci`: per locus a dict chrom,
    left, right, strand, gene_id, gene_name, isoforms [(transcript_id, strand, length, [(l, r), ...])]."""
    status, txs = [], {}
    for k, line in enumerate(split_lines(data)):
        st, f = parse_line(line)
        status.append(st)
        if st != OK:
            continue
        chrom, left, right, strand, gene, tx, gname = f
        t = txs.setdefault((_lower(chrom), strand, tx), {"line": k, "chrom": chrom, "strand": strand, "gene": gene, "tx": tx, "gname": gname, "exons": []})
        t["exons"].append((left, right))
    merges = 0
    for t in txs.values():
        out = []
        for l, r in sorted(t["exons"]):
            if out and l <= out[-1][1] + 1:
                out[-1] = (out[-1][0], max(out[-1][1], r))
                merges += 1
            else:
                out.append((l, r))
        t["exons"] = out
    by_line = sorted(txs.values(), key=lambda t: t["line"])
    if ref_names is not None and len(ref_names):
        names = [n if isinstance(n, bytes) else n.encode() for n in ref_names]
        ids = {}
        for k, n in enumerate(names):
            ids.setdefault(_lower(n), k)
    else:
        names, ids = [], {}
        for t in by_line:
            if _lower(t["chrom"]) not in ids:
                ids[_lower(t["chrom"])] = len(names)
                names.append(t["chrom"])
    kept = [t for t in by_line if _lower(t["chrom"]) in ids]
    for t in kept:
        t["cid"] = ids[_lower(t["chrom"])]
    kept.sort(key=lambda t: (t["cid"], [c for e in t["exons"] for c in e], t["line"]))
    loci, where = [], {}
    for t in kept:
        key = (t["cid"], t["gene"])
        if key not in where:
            where[key] = len(loci)
            loci.append({"chrom": t["cid"], "strand": t["strand"], "gene_id": t["gene"], "gene_name": t["gname"], "isoforms": []})
        loci[where[key]]["isoforms"].append((t["tx"], t["strand"], sum(r - l + 1 for l, r in t["exons"]), t["exons"]))
    for locus in loci:
        locus["left"] = min(i[3][0][0] for i in locus["isoforms"])
        locus["right"] = max(i[3][-1][1] for i in locus["isoforms"])
        locus["segments"] = disjoint_segments(sorted({e for i in locus["isoforms"] for e in i[3]}))
    status = np.array(status, np.uint8)
    info = {"lines": int(status.size), "transcripts": len(kept), "loci": len(loci), "exons": sum(len(i[3]) for l in loci for i in l["isoforms"]),
            "segments": sum(len(l["segments"]) for l in loci), "chromosomes": len(names), "merged_exons": merges,
            "dropped_transcripts": len(by_line) - len(kept)}
    for k, name in enumerate(("ok", "skip", "fields", "other", "coord", "no_transcript", "no_gene")):
        info["lines_" + name] = int((status == k).sum())
    return {"status": status, "info": info, "chrom": names, "loci": loci}


def assert_matches(g, want):
    """A GtfAnnotation against restate()'s result: every array, name, status and info word."""
    np.testing.assert_array_equal(g.line_status, want["status"])
    assert g.info == want["info"], (g.info, want["info"])
    assert g.chrom == want["chrom"]
    rows = g.rows()
    assert len(rows) == len(want["loci"])
    for l, (got, exp) in enumerate(zip(rows, want["loci"])):
        for key in ("chrom", "left", "right", "strand", "gene_id", "gene_name"):
            assert got[key] == exp[key], (l, key, got[key], exp[key])
        assert got["isoforms"] == [(t, s, n, list(e)) for t, s, n, e in exp["isoforms"]], (l, got["isoforms"], exp["isoforms"])
        s0, s1 = int(g.seg_off[l]), int(g.seg_off[l + 1])
        assert list(zip(g.seg_left[s0:s1].tolist(), g.seg_right[s0:s1].tolist())) == exp["segments"], l


def assert_same(a, b):
    """Two GtfAnnotations (the device form against the host form): everything exact."""
    for name in ("iso_off", "exon_off", "exon_left", "exon_right", "seg_off", "seg_left", "seg_right", "cluster_ref", "cluster_left",
                 "cluster_right", "cluster_strand", "iso_len", "iso_strand", "line_status"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    for name in ("gene_id", "gene_name", "transcript_id", "chrom", "info", "n_loci", "n_iso"):
        assert getattr(a, name) == getattr(b, name), name


def exon_line(chrom, left, right, strand, gene, tx, gname=None, kind="exon", score=".", source="src", extra=""):
    attrs = 'gene_id "%s"; transcript_id "%s";' % (gene, tx)
    if gname is not None:
        attrs += ' gene_name "%s";' % gname
    return ("%s\t%s\t%s\t%d\t%d\t%s\t%s\t.\t%s%s" % (chrom, source, kind, left, right, score, strand, attrs, extra)).encode()


def random_gtf(seed, n_genes=300, n_chrom=3, shuffle=0.2, long_attrs=False):
    """A seeded annotation: genes of 1-6 transcripts over a shared pool of exons, on n_chrom chromosomes and both strands, with
    gene / transcript / CDS lines, comments, CRLF ends, scores, some exons given twice or touching, some genes overlapping, and
    a fraction `shuffle` of the exon lines moved to random places of the file."""
    rng = np.random.default_rng(seed)
    lines, movable = [b"# generated, seed %d" % seed, b"#!genome-build none"], []
    pos = {c: 1000 for c in range(n_chrom)}
    for g in range(n_genes):
        c = int(rng.integers(n_chrom))
        chrom = "chr%d" % (c + 1) if rng.random() < 0.9 else "CHR%d" % (c + 1)
        strand = "+-."[int(rng.choice(3, p=[0.48, 0.48, 0.04]))]
        start = pos[c] + int(rng.integers(-200, 2000))
        n_pool = int(rng.integers(1, 12))
        pool, at = [], max(start, 1)
        for _ in range(n_pool):
            length = int(rng.integers(20, 400))
            pool.append((at, at + length - 1))
            at += length + int(rng.choice([0, 1, 2, 50, 300, 3000]))
        pos[c] = at if rng.random() < 0.8 else start + 100
        gene, gname = "G%05d.%d" % (g, seed), "name%d" % g
        tail = ' gene_biotype "protein_coding"; level 2; tag "basic"; havana_gene "OTTHUMG%011d.1";' % g if long_attrs else ""
        lines.append(("%s\tsrc\tgene\t%d\t%d\t.\t%s\t.\tgene_id \"%s\"; gene_name \"%s\";%s" % (chrom, pool[0][0], pool[-1][1], strand, gene, gname, tail)).encode())
        for t in range(int(rng.integers(1, 7))):
            tx = "T%05d.%d" % (g, t)
            pick = sorted(set(rng.choice(n_pool, size=int(rng.integers(1, n_pool + 1)), replace=False).tolist()))
            lines.append(("%s\tsrc\ttranscript\t%d\t%d\t.\t%s\t.\tgene_id \"%s\"; transcript_id \"%s\";%s" %
                          (chrom, pool[pick[0]][0], pool[pick[-1]][1], strand, gene, tx, tail)).encode())
            for e in pick:
                l, r = pool[e]
                if rng.random() < 0.1:
                    l, r = r, l
                line = exon_line(chrom, l, r, strand, gene, tx, gname if rng.random() < 0.8 else None, kind="exon" if rng.random() < 0.9 else "coding_exon",
                                 score="." if rng.random() < 0.8 else "0.5", extra=" exon_number %d;%s" % (e + 1, tail))
                if rng.random() < 0.05:
                    line += b"\r"
                (movable if rng.random() < shuffle else lines).append(line)
                if rng.random() < 0.05:
                    lines.append(line)
                if rng.random() < 0.3:
                    lines.append(("%s\tsrc\tCDS\t%d\t%d\t.\t%s\t0\tgene_id \"%s\"; transcript_id \"%s\";" % (chrom, min(l, r), max(l, r), strand, gene, tx)).encode())
    for line in movable:
        lines.insert(int(rng.integers(2, len(lines) + 1)), line)
    return b"\n".join(lines) + b"\n"


def _x(chrom="chr1", left=100, right=200, strand="+", attrs='gene_id "g"; transcript_id "t";', kind="exon", score=".", c4=None, c5=None):
    """One line with every column free."""
    return ("%s\tsrc\t%s\t%s\t%s\t%s\t%s\t.\t%s" % (chrom, kind, left if c4 is None else c4, right if c5 is None else c5, score, strand, attrs)).encode()


def hand_files():
    """One small file per rule of include/sbgpu.h: name -> (bytes, ref_names or None)."""
    F = {}
    ok = _x()
    F["comment_short_tabs"] = (b"\n".join([b"# a comment", b"   \t# behind blanks", b"short", b"\t".join([b"chr1", b"src", b"exon", b"1", b"2", b".", b"+", b"no eighth tab"]), ok]) + b"\n", None)
    F["crlf"] = (ok + b"\r\n" + _x(left=300, right=400) + b"\r\n", None)
    F["no_final_newline"] = (ok + b"\n" + _x(left=300, right=400), None)
    F["empty"] = (b"", None)
    F["only_comments"] = (b"# one\n#two two two\n", None)
    F["only_newlines"] = (b"\n\n\n", None)
    F["hash_behind_tabs"] = (b"\t\t\t\t\t\t\t\t# a comment behind eight tabs\n" + ok + b"\n", None)
    F["types"] = (b"\n".join([_x(attrs='gene_id "g"; transcript_id "t%d";' % k, kind=kind) for k, kind in
                               enumerate(["exon", "EXON", "coding_exon", "five_prime_utr_exon", "CDS", "transcript", "UTR", "exonic_part"])]) + b"\n", None)
    F["coords"] = (b"\n".join([_x(c4="0"), _x(c4=""), _x(c4="12x", c5="20"), _x(c4="x12"), _x(c4="5", c5=str(2 ** 31 - 1)), _x(c4="5", c5=str(2 ** 31)),
                                _x(c4="5", c5="99999999999999999999999"), _x(c4=" 7"), _x(c4="-7"), _x(left=900, right=800)]) + b"\n", None)
    F["score"] = (b"\n".join([_x(score="0.5"), _x(left=300, right=400, score="1e3"), _x(left=500, right=600, score="abc")]) + b"\n", None)
    F["strand"] = (b"\n".join([_x(strand=".", attrs='gene_id "g"; transcript_id "a";'), _x(strand="?", attrs='gene_id "g"; transcript_id "b";'),
                                _x(strand="", attrs='gene_id "g"; transcript_id "c";'), _x(strand="+-", attrs='gene_id "g"; transcript_id "d";'),
                                _x(strand="-", attrs='gene_id "g"; transcript_id "e";')]) + b"\n", None)
    F["attributes"] = (b"\n".join([
        _x(attrs='gene_id "quoted"; transcript_id bare; gene_name "n 1";'),
        _x(attrs='note "has gene_id inside; transcript_id x"; gene_id "g2"; transcript_id "t2";'),
        _x(attrs='ref_gene_id "wrong"; gene_id "right"; transcript_id "t3";'),
        _x(attrs='GENE_ID "upper"; Transcript_Id "t4"; GENE_NAME "N";'),
        _x(attrs='gene_id "g5"; transcript_id "t5"'),
        _x(attrs='transcript_id "t6"; gene_id "g6";'),
        _x(attrs='gene_id  "two blanks";transcript_id "t7";gene_name bare name ;'),
        _x(attrs='gene_idx "no"; transcript_id "t8"; gene_id "g8";'),
        _x(attrs='gene_id "g9"; transcript_id "unterminated'),
        _x(attrs='gene_id "g10"; transcript_id'),
        _x(attrs='gene_id "g11"; transcript_id ;'),
        _x(attrs='transcript_id "t12"; gene_id "";'),
        _x(attrs='transcript_id "t13";'),
        _x(attrs='ID=exon1;Parent=tx1'),
        _x(attrs='gene_id "g15";x"y;transcript_id "hidden"; z" transcript_id "t15";'),
        _x(attrs='gene_id transcript_id "t16"; gene_name "n16";'),
        _x(attrs=''),
        _x(attrs='gene_id "g\xc3\xa9\x00z"; transcript_id "t\xff18";'.encode("latin-1").decode("latin-1")),
    ]) + b"\n", None)
    F["name_255"] = (_x(attrs='gene_id "%s"; transcript_id "%s"; gene_name "%s";' % ("g" * 255, "t" * 255, "n" * 255), chrom="c" * 255) + b"\n", None)
    F["scattered"] = (b"\n".join([_x(left=900, right=950, attrs='gene_id "g"; transcript_id "a";'), _x(left=100, right=200, attrs='gene_id "h"; transcript_id "b";'),
                                   _x(left=500, right=600, attrs='gene_id "g"; transcript_id "a";'), b"# between", _x(left=300, right=400, attrs='gene_id "h"; transcript_id "b";'),
                                   _x(left=100, right=200, attrs='gene_id "other"; transcript_id "a";')]) + b"\n", None)
    F["merges"] = (b"\n".join([_x(left=l, right=r) for l, r in [(100, 200), (100, 200), (150, 300), (301, 400), (402, 500), (450, 460), (100, 120)]]) + b"\n", None)
    F["one_tx_two_strands_two_chroms"] = (b"\n".join([_x(), _x(strand="-", left=300, right=400), _x(chrom="chr2", left=500, right=600), _x(chrom="CHR1", left=700, right=800)]) + b"\n", None)
    same = [_x(left=100, right=200, attrs='gene_id "g"; transcript_id "t%d";' % k) for k in (3, 1, 2)]
    F["identical_keep_file_order"] = (b"\n".join(same) + b"\n", None)
    F["prefix_first"] = (b"\n".join([_x(left=100, right=200, attrs='gene_id "g"; transcript_id "long";'), _x(left=300, right=400, attrs='gene_id "g"; transcript_id "long";'),
                                      _x(left=100, right=200, attrs='gene_id "g"; transcript_id "short";'), _x(left=100, right=150, attrs='gene_id "g"; transcript_id "first";')]) + b"\n", None)
    chroms = b"\n".join([_x(chrom="chrB", attrs='gene_id "gb"; transcript_id "tb";'), _x(chrom="chrA", attrs='gene_id "ga"; transcript_id "ta";'),
                         _x(chrom="CHRb", left=300, right=400, attrs='gene_id "gb"; transcript_id "tb";'), _x(chrom="chrZ", attrs='gene_id "gz"; transcript_id "tz";')]) + b"\n"
    F["chroms_first_appearance"] = (chroms, None)
    F["chroms_table"] = (chroms, ["chrA", "CHRB", "chrC", "chra"])
    F["interleaved_genes"] = (b"\n".join([_x(left=100, right=200, attrs='gene_id "g1"; transcript_id "a";'), _x(left=150, right=250, attrs='gene_id "g2"; transcript_id "b";'),
                                           _x(left=180, right=300, attrs='gene_id "g1"; transcript_id "c";'), _x(left=190, right=310, attrs='gene_id "g2"; transcript_id "d";')]) + b"\n", None)
    return F

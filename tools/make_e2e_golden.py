#!/usr/bin/env python3
"""End-to-end golden from the REFERENCE BINARY (config C1 plumbing, SURVEY 8(c) `e2e_toy`).

Runs only where /root/reference is mounted: builds oracle/_ref (the reference program
compiled from its own sources, plus our sam2bam), simulates paired-end reads over a small
synthetic annotation, runs

    strawberry_ref toy.bam -g toy.gtf -r -i 250/30 -o out.gtf -T log.txt -f ctx.tsv

and commits ONLY data: the annotation we wrote, and the reference's outputs (GTF attributes,
theta log lines, the -f context table).  The SAM/BAM are regenerable and not committed.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import build  # noqa: E402
from oracle.lib import REF_BIN, SAM2BAM  # noqa: E402

DUMP_BIN = os.path.join(ROOT, "oracle", "_ref", "strawberry_dump")   # the reference program with a tap on EmSolver (oracle/em_dump_shim.cpp)

RL = 75
MEAN, SD = 250.0, 30.0


def make_annotation(rng, n_genes, ex_lo=60, ex_hi=400):
    genes = []
    pos = 1000
    for g in range(n_genes):
        n_ex = int(rng.integers(4, 9))
        exons = []
        for _ in range(n_ex):
            ln = int(rng.integers(ex_lo, ex_hi))
            exons.append((pos, pos + ln - 1))
            pos += ln + int(rng.integers(80, 600))
        n_iso = int(rng.integers(2, 5))
        isos = [list(range(n_ex))]
        tries = 0
        while len(isos) < n_iso and tries < 50:
            tries += 1
            keep = [0] + [k for k in range(1, n_ex - 1) if rng.random() < 0.6] + [n_ex - 1]
            if keep not in isos and len(keep) >= 2:
                isos.append(keep)
        genes.append({"id": "G%d" % (g + 1), "exons": exons, "isos": isos, "strand": "+", "chrom": "chr1"})
        pos += 5000
    return genes, pos + 1000


def write_gtf(genes, path):
    with open(path, "w") as f:
        for g in genes:
            for t, iso in enumerate(g["isos"]):
                tid = "%s.%d" % (g["id"], t + 1)
                ex = [g["exons"][k] for k in iso]
                attr = 'gene_id "%s"; transcript_id "%s";' % (g["id"], tid)
                f.write("%s\tsynth\ttranscript\t%d\t%d\t.\t%s\t.\t%s\n" % (g["chrom"], ex[0][0], ex[-1][1], g["strand"], attr))
                for (a, b) in ex:
                    f.write("%s\tsynth\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (g["chrom"], a, b, g["strand"], attr))


def tx_to_genome(ex, t0, t1):
    """transcript interval [t0, t1) -> list of genomic blocks [(start, end)] (1-based closed)."""
    blocks = []
    off = 0
    for (a, b) in ex:
        ln = b - a + 1
        lo, hi = max(t0, off), min(t1, off + ln)
        if lo < hi:
            blocks.append((a + lo - off, a + hi - off - 1))
        off += ln
    return blocks


def cigar(blocks):
    s = ""
    for k, (a, b) in enumerate(blocks):
        if k:
            s += "%dN" % (a - blocks[k - 1][1] - 1)
        s += "%dM" % (b - a + 1)
    return s


def simulate(rng, genes, frags_per_gene, dup=0.0, multi=0.0, single=False, long_reads=False):
    """dup: chance that a fragment is sequenced again (1-3 PCR duplicates: same alignments, other read
    names); multi: chance that a pair is multi-mapped (NH 2 or 3 on both mates).  With either, two
    different fragments never share (left end, right end): the reference sorts hits by that pair only
    (src/read.cpp:917-923) before collapsing neighbours, and the order of ties is std::sort's business."""
    recs = []
    frags = []
    seen = set()
    spans = set()
    rid = 0
    for gi, g in enumerate(genes):
        w = rng.dirichlet(np.ones(len(g["isos"])) * 0.8)
        for _ in range(frags_per_gene):
            t = int(rng.choice(len(g["isos"]), p=w))
            ex = [g["exons"][k] for k in g["isos"][t]]
            L = sum(b - a + 1 for a, b in ex)
            fl = int(np.clip(np.rint(rng.normal(MEAN, SD)), 2 * RL + 1, L))
            if fl > L:
                continue
            st = int(rng.integers(0, L - fl + 1))
            left = tx_to_genome(ex, st, st + RL)
            right = tx_to_genome(ex, st + fl - RL, st + fl)
            sig = (tuple(left), tuple(right))
            if sig in seen:     # no duplicate fragments: bin counts then equal uniq-hit counts
                continue
            if long_reads:      # long-read library: one unpaired read of 1001..2600 bases of the transcript
                if L < 1100:
                    continue
                rlen = int(rng.integers(1001, min(L, 2600) + 1))
                st = int(rng.integers(0, L - rlen + 1))
                left = tx_to_genome(ex, st, st + rlen)
            if single or long_reads:  # single-end library: only the first mate is sequenced, unpaired (flag 0)
                rlen = sum(b - a + 1 for a, b in left)
                right = []
                sig = (tuple(left), ())
                if sig in seen or (left[0][0], left[-1][1]) in spans:
                    continue
                spans.add((left[0][0], left[-1][1]))
                seen.add(sig)
                rid += 1
                recs.append(((g["chrom"], left[0][0]), "r%06d\t0\t@CHROM@\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tNH:i:1\tXS:A:%s" % (
                    rid, left[0][0], cigar(left), "A" * rlen, "I" * rlen, g["strand"])))
                frags.append((gi, left, right, [1]))
                continue
            if dup or multi:
                if (left[0][0], right[-1][1]) in spans:
                    continue
                spans.add((left[0][0], right[-1][1]))
            seen.add(sig)
            copies = 1 + (int(rng.integers(1, 4)) if dup and rng.random() < dup else 0)
            nhs = []
            tlen = right[-1][1] - left[0][0] + 1
            for _ in range(copies):
                nh = int(rng.integers(2, 4)) if multi and rng.random() < multi else 1
                nhs.append(nh)
                rid += 1
                name = "r%06d" % rid
                recs.append(((g["chrom"], left[0][0]), "%s\t99\t@CHROM@\t%d\t255\t%s\t=\t%d\t%d\t%s\t%s\tNH:i:%d\tXS:A:%s" % (
                    name, left[0][0], cigar(left), right[0][0], tlen, "A" * RL, "I" * RL, nh, g["strand"])))
                recs.append(((g["chrom"], right[0][0]), "%s\t147\t@CHROM@\t%d\t255\t%s\t=\t%d\t%d\t%s\t%s\tNH:i:%d\tXS:A:%s" % (
                    name, right[0][0], cigar(right), left[0][0], -tlen, "A" * RL, "I" * RL, nh, g["strand"])))
            frags.append((gi, left, right, nhs))
    recs = [(k, line.replace("@CHROM@", k[0])) for k, line in recs]
    recs.sort(key=lambda r: r[0])
    return recs, frags


def save_frags(frags, path):
    """reads.npz: our simulated fragments (inputs of the golden run) as aligned blocks, 1-based closed."""
    def csr(which):
        off, bl, br = [0], [], []
        for f in frags:
            for (a, b) in f[which]:
                bl.append(a)
                br.append(b)
            off.append(len(bl))
        return np.asarray(off, np.int64), np.asarray(bl, np.uint32), np.asarray(br, np.uint32)
    lo, ll, lr = csr(1)
    ro, rl, rr = csr(2)
    # per fragment the NH tags of its copies (one copy with NH 1 in the plain toys)
    nh_off = np.concatenate([[0], np.cumsum([len(f[3]) for f in frags])]).astype(np.int64)
    np.savez_compressed(path, gene=np.asarray([f[0] for f in frags], np.int32), left_off=lo, left_l=ll, left_r=lr,
                        right_off=ro, right_l=rl, right_r=rr, nh_off=nh_off,
                        nh=np.asarray([n for f in frags for n in f[3]], np.int32))


def write_genome(rng, length, out_dir):
    """genome.fa (60 bases per line) + genome.fa.fai (the reference cannot build the index, fasta.cpp:89-91)."""
    seq = np.empty(length, np.uint8)
    at = 0
    while at < length:                       # stretches of 30-300 bases, each with its own GC content
        n = int(rng.integers(30, 300))
        gc = float(rng.choice([0.15, 0.35, 0.5, 0.65, 0.85, 0.95]))
        p = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
        seq[at:at + n] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n, p=p)[:length - at]
        at += n
    lower = rng.random(length) < 0.08
    seq[lower] |= 0x20
    seq[rng.random(length) < 0.01] = ord("N")
    text = seq.tobytes().decode()
    with open(os.path.join(out_dir, "genome.fa"), "w") as f:
        f.write(">chr1\n")
        for i in range(0, length, 60):
            f.write(text[i:i + 60] + "\n")
    with open(os.path.join(out_dir, "genome.fa.fai"), "w") as f:
        f.write("chr1\t%d\t6\t60\t61\n" % length)


def write_genome_chroms(rng, length, out_dir, chroms=(("chr1", 60), ("chr2", 50))):
    """genome.fa with one contig per chromosome, each wrapped at its own width, and the genome.fa.fai this library's reader
    writes for it (strawberry_amd.fasta, the host form): the reference then reads the sequence through an index built here."""
    from strawberry_amd.fasta import read_fasta
    alphabet = np.frombuffer(b"ACGT", np.uint8)
    path = os.path.join(out_dir, "genome.fa")
    with open(path, "w") as f:
        for name, width in chroms:
            seq = np.empty(length, np.uint8)
            at = 0
            while at < length:                   # stretches of 30-300 bases, each with its own GC content
                n = int(rng.integers(30, 300))
                gc = float(rng.choice([0.15, 0.35, 0.5, 0.65, 0.85, 0.95]))
                p = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
                seq[at:at + n] = rng.choice(alphabet, size=n, p=p)[:length - at]
                at += n
            seq[rng.random(length) < 0.08] |= 0x20
            seq[rng.random(length) < 0.01] = ord("N")
            text = seq.tobytes().decode()
            f.write(">%s\n" % name)
            for i in range(0, length, width):
                f.write(text[i:i + width] + "\n")
    with open(path + ".fai", "w") as f:
        f.write(read_fasta(path).fai_text())


def main():
    build(with_ref=True)
    only = sys.argv[1:]
    if only:                                  # regenerate the named runs only
        global make
        _make = make
        make = lambda name, *a, **k: _make(name, *a, **k) if name in only else None  # noqa: E731
    # e2e_toy: short exons -- bins spanning many segments, implicit (mate-gap) segments: pins the
    #          bin-weight model.  e2e_toy_long: every exon longer than any mate gap, so a bin's
    #          fragments all have the same isoform compatibility and the -f table shows the full
    #          EM input: pins EmSolver / FPKM / TPM end to end.
    make("e2e_toy", 4242, 60, 400)
    make("e2e_toy_long", 4343, 420, 900)
    # e2e_toy_mass: PCR duplicates and multi-mapped pairs (NH 2 / 3, --allow-multimapped-hits): hit masses
    #          are sums of 1, 1/2, 1/3 -- pins the collapse mass, the float accumulation of
    #          ExonBin::read_count with its int truncation, and the int-truncated mapped-read total.
    make("e2e_toy_mass", 4444, 200, 700, dup=0.3, multi=0.35, extra=["--allow-multimapped-hits"])
    # e2e_toy_filter: the reads of e2e_toy_long with `-e 0.05` after `-r` (kMinIsoformFrac = 0.05,
    #          Strawberry.cpp:158-177): isoforms below 5 % of their locus are erased after the EM
    #          (estimate.cpp:346-355), TPM is taken over the survivors, the -f table loses their columns.
    make("e2e_toy_filter", 4343, 420, 900, extra=["-e", "0.05"])
    # e2e_toy_emp: the reads of e2e_toy WITHOUT -i: the reference then builds the empirical insert-size
    #          distribution in its first pass (fragLenDist, alignments.cpp:1363-1407: the exonic span of every
    #          unique hit that fits exactly one transcript) and the bin weights use it (read.cpp:274-297).
    make("e2e_toy_emp", 4242, 60, 400, insert=False)
    # e2e_toy_single: a single-end library (unpaired reads).  The reference then forces the insert size to
    #          N(200, 80) whatever -i says (Strawberry.cpp:329-333) and every hit is a single read.
    make("e2e_toy_single", 4545, 60, 400, single=True)
    # e2e_toy_longread: unpaired reads of 1001-2600 bases.  More than ten read lengths above 1000 switch the
    #          reference to its long-read workflow (Strawberry.cpp:292-303): every bin weight is 1/L_j
    #          (set_bin_weight_without_frag_dist, estimate.cpp:236-247).
    make("e2e_toy_longread", 4646, 300, 700, long_reads=True, n_frags=400)
    # e2e_toy_bias: `-b genome.fa` -- the reference's bias option.  It changes no abundance (src/bias.cpp holds
    #          no code); it appends six columns to the -f table: GC ratio, hexamer entropy and four high-GC-stretch
    #          flags of every bin's sequence (alignments.cpp:1622-1636, kmer.h).  The genome is ours: random bases
    #          with GC-rich and GC-poor stretches, some lower case, some N.  Exons of 60+ bases: the reference
    #          aborts on a bin of 40 bases or fewer (kmer.h:82, asserts are live in its release build).
    make("e2e_toy_bias", 4747, 60, 400, genome=True)
    # e2e_toy_minus: every other gene on the minus strand (GTF strand column, XS:A:- on its reads): pins the
    #          strand handling of the output (Contig::print2gtf's strand column and exon numbering).
    make("e2e_toy_minus", 4848, 150, 500, minus=True)
    # e2e_toy_chroms: the genes alternate between two chromosomes: the mapped-read total runs over both
    #          (alignments.cpp:1372) and the output is written chromosome by chromosome.
    make("e2e_toy_chroms", 4949, 150, 500, chroms=2)
    # e2e_bias_chroms: `-b genome.fa` over two chromosomes.  The genome's two contigs are wrapped at 60 and at 50 bases, and
    #          its .fai is the one strawberry_amd.fasta writes: the reference reads every bin's sequence through an index this
    #          library built, and the library's reader reproduces the reference's six columns.
    make("e2e_bias_chroms", 5050, 60, 400, chroms=2, genome="chroms", plain_header=True)
    # e2e_toy_assembly (BASELINE config 4 / C1 plumbing): the reference in its DEFAULT mode -- no -g, no -r: the first pass
    #          assembles transcripts from the reads (assembleSample, alignments.cpp:1658), the second quantifies the
    #          ASSEMBLED contigs (reset_refmRNAs, alignments.cpp:1091-1101) with kMinIsoformFrac = 0.01, so the post-EM
    #          filter fires (estimate.cpp:346-355: this seed loses one of 18 isoforms).  toy.gtf is only the
    #          simulation's source here; the program never sees it.
    make("e2e_toy_assembly", 5165, 150, 500, n_frags=2500, assembly=True)
    if not only or "em_c4_assembled" in only:
        make_c4_em_golden()


def write_sam(recs, genes, chrom_len, path):
    with open(path, "w") as f:
        f.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (c, chrom_len) for c in sorted(set(g["chrom"] for g in genes))))
        for _, line in recs:
            f.write(line + "\n")


def read_em_dump(path):
    """oracle/em_dump_shim.cpp's records -> [(n[nrow] int32, alpha[nrow, niso] f64, init, run, theta[niso])]."""
    import struct
    d = open(path, "rb").read()
    loci, p = [], 0
    while p < len(d):
        tag = d[p:p + 1]
        p += 1
        if tag == b"I":
            niso, nrow = struct.unpack_from("ii", d, p)
            p += 8
            n = np.frombuffer(d, np.int32, nrow, p).copy()
            p += 4 * nrow
            alpha = np.frombuffer(d, np.float64, nrow * niso, p).reshape(nrow, niso).copy()
            p += 8 * nrow * niso
            ok, = struct.unpack_from("i", d, p)
            p += 4
            loci.append([n, alpha, ok, 0, None])
        else:
            assert tag == b"R", tag
            ok, k = struct.unpack_from("ii", d, p)
            p += 8
            loci[-1][3] = ok
            loci[-1][4] = np.frombuffer(d, np.float64, k, p).copy()
            p += 8 * k
    return loci


def make_c4_em_golden():
    """tests/golden/em_c4_assembled.npz: the EXACT (n, alpha) that loci of ASSEMBLED isoforms hand to EmSolver::init in
    the reference's default mode, with the reference's own theta / flags -- captured by oracle/_ref/strawberry_dump
    (the reference program; em_dump_shim.cpp taps the seam and forwards to the reference's bodies).  Four runs of 40
    genes each over different exon-size ranges; loci the assembler leaves with one isoform are kept (1-column EM)."""
    from strawberry_amd import synth
    loci, thetas, flags = [], [], []
    for seed, ex_lo, ex_hi, n_frags in ((6101, 150, 500, 1500), (6102, 60, 400, 2500), (6103, 300, 800, 800), (6104, 100, 300, 4000)):
        rng = np.random.Generator(np.random.PCG64(seed))
        genes, chrom_len = make_annotation(rng, 40, ex_lo, ex_hi)
        with tempfile.TemporaryDirectory() as tmp:
            recs, _ = simulate(rng, genes, n_frags)
            write_sam(recs, genes, chrom_len, os.path.join(tmp, "toy.sam"))
            subprocess.check_call([SAM2BAM, os.path.join(tmp, "toy.sam"), os.path.join(tmp, "toy.bam")], stderr=subprocess.DEVNULL)
            outs = {}
            for prog in (REF_BIN, DUMP_BIN):     # the tap must not change the program's outputs
                for n in ("out.gtf", "ctx.tsv", "log.txt"):
                    if os.path.exists(os.path.join(tmp, n)):
                        os.remove(os.path.join(tmp, n))
                r = subprocess.run([prog, "toy.bam", "-i", "%d/%d" % (MEAN, SD), "-o", "out.gtf", "-T", "log.txt", "-f", "ctx.tsv"], cwd=tmp,
                                   capture_output=True, text=True, env=dict(os.environ, SB_EM_DUMP=os.path.join(tmp, "em.bin")))
                r.check_returncode()
                outs[prog] = [open(os.path.join(tmp, "out.gtf")).read().split("\n", 1)[1], open(os.path.join(tmp, "ctx.tsv")).read()]
            assert outs[REF_BIN] == outs[DUMP_BIN], "strawberry_dump's outputs differ from strawberry_ref's"
            got = read_em_dump(os.path.join(tmp, "em.bin"))
            n_log = sum("raw read count" in l for l in open(os.path.join(tmp, "log.txt")))
            n_out = sum("\ttranscript\t" in l for l in open(os.path.join(tmp, "out.gtf")))
            print("seed %d: %d records, %d loci reached the EM, %d isoforms solved, %d survive the 0.01 filter" % (
                seed, len(recs), len(got), n_log, n_out))
        for n, alpha, ok, ran, theta in got:
            loci.append((n, alpha))
            if theta is None:           # init() false: run() never called; theta_0 is not observable -- the flags say so
                theta = np.full(alpha.shape[1], float(n.sum()) / alpha.shape[1])
            thetas.append(theta)
            flags.append((1 if ok else 0) | (2 if ran else 0))
    b = synth.from_loci(loci, name="c4_assembled")
    path = os.path.join(ROOT, "tests", "golden", "em_c4_assembled.npz")
    np.savez_compressed(path, row_off=b.row_off, iso_off=b.iso_off, f_off=b.f_off, count=b.count, F=b.F, length=b.length,
                        ref_theta=np.concatenate(thetas), ref_flags=np.asarray(flags, np.int32))
    print("em_c4_assembled: %d loci, %d isoforms, %d bins -> %s (%d KB)" % (
        b.n_loci, int(b.iso_off[-1]), int(b.row_off[-1]), os.path.relpath(path, ROOT), os.path.getsize(path) // 1024))


def make(name, seed, ex_lo, ex_hi, dup=0.0, multi=0.0, extra=(), insert=True, single=False, long_reads=False, n_frags=900,
         genome=False, minus=False, chroms=1, assembly=False, plain_header=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    genes, chrom_len = make_annotation(rng, 6, ex_lo, ex_hi)
    if minus:
        for g in genes[1::2]:
            g["strand"] = "-"
    if chroms == 2:
        for g in genes[1::2]:
            g["chrom"] = "chr2"
    out_dir = os.path.join(ROOT, "tests", "golden", name)
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        gtf = os.path.join(tmp, "toy.gtf")
        write_gtf(genes, gtf)
        recs, frags = simulate(rng, genes, n_frags, dup, multi, single, long_reads)
        save_frags(frags, os.path.join(out_dir, "reads.npz"))
        sam = os.path.join(tmp, "toy.sam")
        with open(sam, "w") as f:
            f.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (c, chrom_len) for c in sorted(set(g["chrom"] for g in genes))))
            for _, line in recs:
                f.write(line + "\n")
        bam = os.path.join(tmp, "toy.bam")
        subprocess.check_call([SAM2BAM, sam, bam])
        extra = list(extra)
        if genome == "chroms":
            write_genome_chroms(rng, chrom_len + 500, tmp)
            extra += ["-b", "genome.fa"]
        elif genome:
            write_genome(rng, chrom_len + 500, tmp)
            extra += ["-b", "genome.fa"]
        cmd = [REF_BIN, bam] + ([] if assembly else ["-g", gtf, "-r"]) + (["-i", "%d/%d" % (MEAN, SD)] if insert else []) + ["-o", os.path.join(tmp, "out.gtf"),
               "-T", os.path.join(tmp, "log.txt"), "-f", os.path.join(tmp, "ctx.tsv")] + list(extra)
        r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
        print(r.stdout[-2000:])
        print(r.stderr[-3000:])
        r.check_returncode()
        for name in ("toy.gtf", "out.gtf", "ctx.tsv") + (("genome.fa",) if genome else ()):
            data = open(os.path.join(tmp, name)).read()
            if plain_header and name == "out.gtf" and data.startswith("#"):
                # the program writes its command line into the first line: keep the words, not where the files lay
                first, rest = data.split("\n", 1)
                data = "#" + " ".join(os.path.basename(w) if w.startswith("/") else w for w in first[1:].split(" ")) + "\n" + rest
            open(os.path.join(out_dir, name), "w").write(data)
        with open(os.path.join(out_dir, "theta_log.txt"), "w") as f:
            for line in open(os.path.join(tmp, "log.txt")):
                if "raw read count" in line or "not compatible" in line:
                    f.write(line)
        with open(os.path.join(out_dir, "README.txt"), "w") as f:
            f.write("Generated by tools/make_e2e_golden.py from the reference binary (oracle/_ref/strawberry_ref):\n"
                    "  %s\n"
                    "toy.gtf is our synthetic annotation%s; out.gtf, ctx.tsv and theta_log.txt are the reference's outputs.\n"
                    "%d read records, read length %d, %s, %d genes.\n" % (
                        " ".join(os.path.basename(c) if c.startswith("/") else c for c in cmd),
                        " (the simulation's source only: the run is in assembly mode and never reads it)" if assembly else "", len(recs), RL,
                        ("insert size -i %d/%d (Gaussian)" % (MEAN, SD)) if insert else
                        "no -i: empirical insert-size distribution (fragments simulated from N(%d, %d))" % (MEAN, SD),
                        len(genes)))
    for name in sorted(os.listdir(out_dir)):
        print(name, os.path.getsize(os.path.join(out_dir, name)))


if __name__ == "__main__":
    main()

"""`-b genome.fa` over chromosomes (sbgpu_binseq_fasta_device / _host) with the genome read by the library's FASTA reader on the
device: the reference binary's -f table of tests/golden/e2e_toy_bias byte for byte, and that of e2e_bias_chroms -- two
chromosomes whose contigs are wrapped at 60 and at 50 bases, which the reference read through the .fai this library wrote.  Then
the runs themselves: any contig order, an EMPTY contig, a handle on the host, zero runs, the host form."""
import os

import numpy as np
import pytest

import e2e_util as U
import exonbin_util as XU
import fasta_util as FU

pytestmark = pytest.mark.gpu

E2E_BIAS_CHROMS = os.path.join(U.HERE, "golden", "e2e_bias_chroms")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.mark.parametrize("which", ["e2e_toy_bias", "e2e_bias_chroms"])
def test_context_table_with_the_library_reading_the_genome(ctx, which, tmp_path):
    from strawberry_amd import fasta
    from strawberry_amd.output import context_table
    from strawberry_amd.quantify import InsertSize, LocusQuantifier
    d = os.path.join(U.HERE, "golden", which)
    ordered, rows, gtf, theta_log = U.load(d)
    genome = fasta.read_fasta(os.path.join(d, "genome.fa"), ctx=ctx)
    assert genome.on_device and genome.n_contigs == (2 if which.endswith("chroms") else 1) and not genome.flags.any()
    if which.endswith("chroms"):
        assert genome.line_bases.tolist() == [60, 50] and genome.line_width.tolist() == [61, 51] and genome.names == [b"chr1", b"chr2"]
    annot, hits, names, _ = XU.e2e_inputs(d, ordered)
    chrom_of = U.gene_chroms(d)
    locus_chrom = [chrom_of[g] for g in names]
    q = LocusQuantifier(annot, hits, InsertSize(250.0, 30.0), 75, ctx=ctx)
    bins = q.assign_bins()
    F = q.bin_weights().cpu().numpy()
    res = q.solve(hits.total_mapped, min_isoform_frac=0.0)
    run_off, run_contig = genome.runs(bins, locus_chrom)
    assert len(set(run_contig.tolist())) == genome.n_contigs and run_off[-1] == bins.n_bins
    stats = genome.bin_sequence_stats(bins, locus_chrom)
    compat = q.d_compat.cpu().numpy().view(np.uint32)[:hits.n_hits]
    table = context_table("toy", hits.total_mapped, names, [[t for t, _ in ordered[g]] for g in names], bins, compat, F,
                          res["fpkm"], res["frac"], keep=res["keep"], seq_stats=stats)
    mine = tmp_path / "ctx.tsv"
    mine.write_text(table)
    got = U.parse_ctx(str(mine))
    assert len(got) == len(rows) > 50 and [r["seq"] for r in got] == [r["seq"] for r in rows] and all(len(r["seq"]) == 6 for r in rows)
    assert table == open(os.path.join(d, "ctx.tsv")).read()
    # the host form, from the device handle and from a host handle, gives the same numbers
    from strawberry_amd.binseq import bin_segments
    seg = bin_segments(bins)
    for g in (genome, fasta.read_fasta(os.path.join(d, "genome.fa"))):
        again = g.run_stats(run_off, run_contig, *seg, ctx=ctx, host_form=True)
        assert all((a == b).all() for a, b in zip(stats, again))


def two_contig_bins(seed=7):
    """A genome of three contigs (the middle one EMPTY) and bins on the first and the last, by run"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s1, s2 = FU.bases(5000, 21), FU.bases(3000, 22)
    data = b">one\n" + FU.wrap(s1, 60) + b">hollow\n>two\n" + FU.wrap(s2, 50)

    def bins_on(n, length):
        out = []
        for _ in range(n):
            k = int(rng.integers(1, 4))
            cuts = np.sort(rng.choice(np.arange(1, length), size=2 * k, replace=False))
            out.append([(int(cuts[2 * j]), int(cuts[2 * j + 1])) for j in range(k)])
        return out
    return data, {0: s1, 2: s2}, bins_on


def flat(bins):
    off = np.cumsum([0] + [len(b) for b in bins]).astype(np.int64)
    return off, np.asarray([a for b in bins for a, _ in b], np.uint32), np.asarray([c for b in bins for _, c in b], np.uint32)


def test_runs_in_any_contig_order_against_the_oracle(ctx, oracle):
    from strawberry_amd import fasta
    data, seqs, bins_on = two_contig_bins()
    g = fasta.read_fasta(data, ctx=ctx)
    assert g.flags.tolist() == [0, FU.EMPTY, 0]
    parts = [(2, bins_on(40, 3000)), (0, bins_on(50, 5000)), (2, bins_on(1, 3000)), (0, []), (0, bins_on(9, 5000))]    # not ascending; an empty run
    allbins = [b for _, bs in parts for b in bs]
    run_off = np.cumsum([0] + [len(bs) for _, bs in parts])
    run_contig = [c for c, _ in parts]
    gc, ent, fl = g.run_stats(run_off, run_contig, *flat(allbins))
    at = 0
    for c, bs in parts:
        if not bs:
            continue
        o, l, r = flat(bs)
        ogc, oent, ofl = oracle.binseq_batch(seqs[c], 1, o, l.tolist(), r.tolist())
        n = len(bs)
        np.testing.assert_array_equal(gc[at:at + n], ogc)
        np.testing.assert_array_equal(fl[at:at + n], ofl)
        assert np.all(np.abs(ent[at:at + n] - oent) <= 1e-12 * np.maximum(1.0, np.abs(oent)))
        at += n
    host = g.run_stats(run_off, run_contig, *flat(allbins), host_form=True)
    assert all((a == b).all() for a, b in zip((gc, ent, fl), host))


def test_refusals_and_zero_runs(ctx):
    from strawberry_amd import _lib, fasta
    data, seqs, bins_on = two_contig_bins()
    g = fasta.read_fasta(data, ctx=ctx)
    bs = bins_on(5, 3000)
    none = g.run_stats([0], [], [0], [], [])
    assert all(len(x) == 0 for x in none)
    for host_form in (False, True):
        with pytest.raises(_lib.SbgpuError) as e:                 # a run on an EMPTY contig
            g.run_stats([0, 5], [1], *flat(bs), host_form=host_form)
        assert "(-1)" in str(e.value) and "empty contig" in str(e.value)
        with pytest.raises(_lib.SbgpuError):                      # a contig the genome does not have
            g.run_stats([0, 5], [3], *flat(bs), host_form=host_form)
        with pytest.raises(_lib.SbgpuError):                      # runs that do not cover the bins
            g.run_stats([0, 4], [2], *flat(bs), host_form=host_form)
    with pytest.raises(_lib.SbgpuError) as e:                     # a segment beyond the contig's end, host form: refused by validation
        g.run_stats([0, 1], [2], [0, 1], [2990], [3001], host_form=True)
    assert "outside" in str(e.value)
    with pytest.raises(_lib.SbgpuError):                          # device form: the kernel's error word
        g.run_stats([0, 1], [2], [0, 1], [2990], [3001])
    # a handle whose sequence is on the host, given to the device entry
    import ctypes as C
    h = fasta.read_fasta(data)
    L = _lib.load()
    run_off, run_contig = np.array([0, 5], np.int64), np.array([2], np.int32)
    rc = L.sbgpu_binseq_fasta_device(ctx.h, h._h, 1, run_off.ctypes.data, run_contig.ctypes.data, 5, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"not on the context's device" in L.sbgpu_last_error()
    assert C.c_void_p(h.sequence_pointer()[0]).value and not h.sequence_pointer()[1]

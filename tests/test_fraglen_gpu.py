"""Pass 1 on the device (fraglen_hist_kernel, strawberry_amd/csrc/fraglen_device.h) against a plain numpy restatement of
Sample::fragLenDist (/root/reference/src/alignments.cpp:1363-1410; tests/fraglen_util.py), on hand-built loci that reach
every route of the kernel:

  * a uniform wave with its locus' table in registers (<= 63 isoforms, <= 64 exon entries), up to the last lane of the
    table (an isoform at index 62, readlane(t_eoff, 63));
  * a uniform wave that walks a bigger locus through scalar loads (64 or 65 exon entries, 64 .. 512 isoforms);
  * several compat words (the unique isoform at 31, 32, 62, 63, 64, the last of 512);
  * waves that straddle a small and a big locus, with loci of 63 .. 65 and 1023 .. 1025 hits and loci of none;
  * lengths of 8191, 8192, 8193 and tens of kilobases (the global atomics), mixed with ordinary ones in one wave;
  * a locus of 1.2e6 hits and batches of more than 2 x CU x 1024 hits (several tiles per workgroup, a locus split
    across workgroups).

The law sbgpu_quantify_resident / sbgpu_quantify_host build from it (insert = NULL) must carry the reference histogram
exactly, and its mean, sd and extremes must be the reference's own InsertSize(frag_lens) (oracle/ref_shim.cpp) bit for
bit.  Every case asserts that it reached its route.  Then: degenerate laws against the reference's emp_dist_pdf and bin
weights, the overflow refusal, and long reads without a law.
"""
import numpy as np
import pytest

import e2e_util as U
import exonbin_util as XU
import fraglen_util as FU

pytestmark = pytest.mark.gpu
RL = 75


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_law(got, hist):
    """the law a quantify call returns == the reference histogram, exactly"""
    lo, h = FU.law_of(hist)
    assert got["use_emp"]
    assert got["start_offset"] == lo and got["end_offset"] == lo + len(h) - 1
    assert got["total_reads"] == int(h.sum())
    np.testing.assert_array_equal(got["emp_hist"], h.astype(np.float64))


def run_pass1(ctx, annot, hits, both=True):
    """the compat words, the reference, and the law of both entries without a law == the reference's histogram"""
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import quantify_host, quantify_resident
    compat, _ = eb.compat_and_keys(annot, hits, ctx)
    # (the kernel masks each locus' last word; the exon-bin kernel never sets a bit past a locus' isoforms either)
    niso = np.diff(annot.iso_off)[hits.hit_locus.astype(np.int64)]
    for w in range(compat.shape[1]):
        beyond = niso <= 32 * w + np.arange(32)[:, None]          # [bit, hit]
        assert not ((compat[:, w][None, :] >> np.arange(32, dtype=np.uint32)[:, None]) & 1)[beyond].any()
    ref = FU.reference(annot, hits, compat)
    np.testing.assert_array_equal(np.bincount(eb.frag_lens(annot, hits, compat)), ref["hist"])
    r = quantify_resident(annot, hits, None, RL, max(hits.n_hits, 1), ctx=ctx)
    assert_law(r["insert"], ref["hist"])
    assert r["n_frag_lens"] == len(ref["lens"])
    if both:
        h = quantify_host(annot, hits, None, RL, ctx=ctx)
        assert_law(h["insert"], ref["hist"])
        np.testing.assert_array_equal(h["compat"], compat)
    return ref, r


def wide_locus_case(niso_shapes, marks, seed, n_big=3000):
    """Loci: a small one of 65 hits (its second wave straddles into the next), the big one, a small one of no hits, a
    small one of 63.  The big locus' hits: `marks` (its unique isoforms that must be reached) 40 times each, the rest over
    all its isoforms with exons, hits in its introns, hits without features."""
    from strawberry_amd import exonbin as eb
    rng = np.random.Generator(np.random.PCG64(seed))
    small_a, pos = FU.make_locus(1000, [(2, 150, 200)] * 3)
    big, pos = FU.make_locus(pos + 5000, niso_shapes)
    small_b, pos = FU.make_locus(pos + 5000, [(3, 120, 90)] * 2)
    small_c, pos = FU.make_locus(pos + 5000, [(2, 200, 150), (1, 300, 0), "dup", (4, 100, 100)])
    annot = eb.Annotation([small_a, big, small_b, small_c])
    hs = FU.HitSet()
    hs.add_pairs(rng, annot, 0, [0, 1, 2], 65)
    with_exons = [j for j, x in enumerate(big) if x]
    for m in marks:
        hs.add_pairs(rng, annot, 1, [m], 40)
    hs.add_pairs(rng, annot, 1, with_exons, n_big)
    if any(len(x) > 1 for x in big):
        hs.add_intronic(rng, annot, 1, 20)
    hs.add_featureless(1, 7)
    hs.add_pairs(rng, annot, 3, [0, 1, 2, 3], 63)
    return annot, hs.hits()


def shapes(n, exons=1, wide_last=0, empty=(), dup=()):
    """n isoforms of `exons` exons, the last `wide_last` of them with one exon more; `empty` without exons; `dup` copies"""
    out = []
    for j in range(n):
        if j in empty:
            out.append(None)
        elif j in dup:
            out.append("dup")
        else:
            out.append((exons + (1 if j >= n - wide_last else 0), 120 + 7 * (j % 5), 80 + 3 * (j % 7)))
    return out


# (isoform shapes of the big locus, unique isoforms to reach, route checks) -- counts from fraglen_util.routes
WIDE = {
    "iso32_words1": (shapes(32, exons=2), [0, 31], dict(words=1, table=True)),
    "iso33_words2": (shapes(33), [31, 32], dict(words=2, table=True)),
    "iso63_entries64": (shapes(63, wide_last=1), [61, 62], dict(words=2, table=True, last_lane=True)),
    "iso63_entries65": (shapes(63, wide_last=2), [62], dict(words=2, table=False)),
    "iso64_entries64": (shapes(64), [62, 63], dict(words=2, table=False)),
    "iso65": (shapes(65), [63, 64], dict(words=3, table=False)),
    "iso200": (shapes(200, exons=3, empty=(5, 77, 150), dup=(9, 10, 120)), [0, 31, 32, 63, 64, 199], dict(words=7, table=False)),
    "iso512": (shapes(512, exons=2, empty=(1, 300, 510), dup=(40, 41, 400)), [0, 31, 32, 62, 63, 64, 511], dict(words=16, table=False)),
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_locus_routes(ctx, name):
    iso_shapes, marks, want = WIDE[name]
    annot, hits = wide_locus_case(iso_shapes, marks, seed=len(iso_shapes) * 7 + len(marks))
    niso = np.diff(annot.iso_off)
    nex = annot.exon_off[annot.iso_off[1:]] - annot.exon_off[annot.iso_off[:-1]]
    assert annot.compat_words == want["words"]
    big = len(iso_shapes)
    assert niso[1] == big
    if name.startswith("iso63") or name.startswith("iso64"):
        assert nex[1] == {"iso63_entries64": 64, "iso63_entries65": 65, "iso64_entries64": 64}[name]
    ref, _ = run_pass1(ctx, annot, hits)
    rt = FU.routes(annot, hits, ref)
    for m in marks:
        assert (big, m) in rt["marks"], (name, m)
    assert rt["table"] > 0 and rt["straddle"] > 0
    if want["table"]:
        assert rt["table"] > 1000 and rt["scalar"] == 0
    else:
        assert rt["scalar"] > 1000 and rt["straddle_big"] > 0
    if want.get("last_lane"):
        assert rt["table_last_lane"] > 0
    if want["words"] > 1:
        assert rt["word_1_plus"] > 0
    intronic = any(len(x) > 1 for x in FU.make_locus(0, iso_shapes)[0])
    assert rt["no_features"] == 7 and rt["zero_compat"] >= 7 + (20 if intronic else 0)
    if "dup" in iso_shapes:
        assert rt["multi_compat"] > 0


def long_case(seed=5):
    """Isoforms with long exons and many exons: single blocks of exactly 8191 / 8192 / 8193 bases, pairs over tens of
    kilobases, and ordinary fragments between them in the same waves."""
    from strawberry_amd import exonbin as eb
    rng = np.random.Generator(np.random.PCG64(seed))
    small, pos = FU.make_locus(1000, [(2, 150, 200)] * 2)
    iso_shapes = [(1, 10000, 0), (30, 500, 300), (3, 12000, 2000), (2, 300, 400), (5, 3000, 5000)]   # (a bin spans <= 32 segments)
    big, pos = FU.make_locus(pos + 3000, iso_shapes)
    annot = eb.Annotation([small, big])
    hs = FU.HitSet()
    hs.add_pairs(rng, annot, 0, [0, 1], 40)
    x0 = big[0][0][0]
    blocks = [[(x0 + d, x0 + d + L - 1)] for L in (8191, 8192, 8193) for d in (0, 1, 1000, 10000 - L)]
    blocks += [[(x0 + d, x0 + d + 250)] for d in range(0, 9700, 150)]     # ordinary lengths among them
    hs.add_blocks(1, blocks)
    hs.add_pairs(rng, annot, 1, [0, 1, 2, 3, 4], 4000, edge=0.3)
    return annot, hs.hits()


@pytest.mark.timeout(300)
def test_long_fragments_take_the_global_histogram(ctx):
    annot, hits = long_case()
    ref, r = run_pass1(ctx, annot, hits)
    rt = FU.routes(annot, hits, ref)
    lens = ref["lens"]
    for L in (8191, 8192, 8193):
        assert (lens == L).sum() >= 4, L
    assert lens.max() > 30000 and rt["global"] > 500 and rt["lds"] > 500
    # a wave with kept lengths on both sides of 8192
    keep = ref["keep"]
    wave = np.flatnonzero(keep) // FU.WAVE
    hi = np.zeros(hits.n_hits // FU.WAVE + 1, bool)
    lo = hi.copy()
    hi[wave[lens >= FU.LDS_BINS]] = True
    lo[wave[lens < FU.LDS_BINS]] = True
    assert (hi & lo).any()
    assert r["insert"]["end_offset"] == lens.max() >= 30000


def many_loci_case(n_target, seed, huge=0):
    """Loci of 1-7 isoforms with hit counts spread around 0, 63-65, 1023-1025 and random ones, until `n_target` hits; with
    `huge` > 0 one locus of that many hits in the middle."""
    from strawberry_amd import exonbin as eb
    rng = np.random.Generator(np.random.PCG64(seed))
    special = [0, 63, 64, 65, 1023, 1024, 1025, 1, 0]
    loci, counts, pos, total = [], [], 1000, 0
    while total < n_target:
        k = len(loci)
        c = special[(k // 3) % len(special)] if k % 3 == 0 else int(rng.integers(1, 2000))
        if huge and k == 40:
            c = huge
        nis = int(rng.integers(1, 8))
        isos, pos = FU.make_locus(pos, [(int(rng.integers(1, 6)), int(rng.integers(100, 400)), int(rng.integers(60, 500))) for _ in range(nis)])
        loci.append(isos)
        counts.append(c)
        total += c
        pos += 2000
    annot = eb.Annotation(loci)
    hs = FU.HitSet()
    for l, c in enumerate(counts):
        hs.add_pairs(rng, annot, l, list(range(len(loci[l]))), c)
    return annot, hs.hits(), counts


@pytest.mark.timeout(600)
def test_huge_locus_split_across_workgroups(ctx):
    annot, hits, counts = many_loci_case(1_500_000, seed=21, huge=1_200_000)
    assert max(counts) == 1_200_000 and hits.n_hits > 2 * n_cu() * 1024
    ref, _ = run_pass1(ctx, annot, hits)
    rt = FU.routes(annot, hits, ref)
    assert rt["table"] > 1_000_000 and rt["straddle"] > 0
    # the kernel's split: whole tiles of 1024 per workgroup, at most 2 x CU workgroups -- the huge locus spans several
    tiles = -(-hits.n_hits // 1024)
    wg = min(tiles, 2 * n_cu())
    per = -(-tiles // wg)
    assert per >= 2
    first = int(np.searchsorted(hits.hit_locus, 40))
    assert (first + 1_200_000) // (per * 1024) - first // (per * 1024) >= 2


@pytest.mark.timeout(600)
def test_many_loci_over_several_tiles_per_workgroup(ctx):
    annot, hits, counts = many_loci_case(2 * n_cu() * 1024 + 5000, seed=22)
    assert hits.n_hits > 2 * n_cu() * 1024
    assert {0, 63, 64, 65, 1023, 1024, 1025} <= set(counts)
    ref, _ = run_pass1(ctx, annot, hits)
    rt = FU.routes(annot, hits, ref)
    assert rt["table"] > 100_000 and rt["straddle"] > 10_000


# ---- the law against the reference's InsertSize ----------------------------------------------------------------------------

@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", ["long", "iso65"])
def test_law_is_the_references_insert_size(ctx, reflib, case):
    """mean, sd and extremes of the law == the reference's InsertSize(frag_lens) of the reference histogram, bitwise; theta,
    status and iterations without a law == those given InsertSize.from_hist of that histogram, bitwise."""
    from strawberry_amd.quantify import InsertSize, quantify_host
    if case == "long":
        annot, hits = long_case(seed=6)
    else:
        iso_shapes, marks, _ = WIDE["iso65"]
        annot, hits = wide_locus_case(iso_shapes, marks, seed=9)
    ref, r = run_pass1(ctx, annot, hits, both=False)
    lo, h = FU.law_of(ref["hist"])
    frag_lens = np.repeat(np.arange(lo, lo + len(h)), h).astype(np.int32)
    pdf, info = reflib.insert_pdf(0.0, 0.0, frag_lens, lo, lo + len(h) - 1)
    law = r["insert"]
    assert law["mean"] == info[0] and law["sd"] == info[1]
    assert law["start_offset"] == info[2] and law["end_offset"] == info[3]
    np.testing.assert_allclose(InsertSize.from_hist(lo, h).pdf_table(lo + len(h), RL)[lo:], pdf, rtol=1e-14, atol=0)
    a = quantify_host(annot, hits, None, RL, ctx=ctx)
    b = quantify_host(annot, hits, InsertSize.from_hist(lo, h), RL, ctx=ctx)
    np.testing.assert_array_equal(a["theta"], b["theta"])
    np.testing.assert_array_equal(a["status"], b["status"])
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["F"], b["F"])


def check(w, ref, rtol):
    """the bin-weight tests' bar: exact zeros where the reference's are, `rtol` elsewhere"""
    nz = ref != 0
    assert ((w != 0) == nz).all()
    err = np.abs(w[nz] - ref[nz]) / np.abs(ref[nz])
    assert err.max() < rtol, err.max()


def random_pairs(rng, n, seg_hi):
    from strawberry_amd.binweight import pack_pairs
    segs, imps, lens = [], [], []
    for _ in range(n):
        nseg = int(rng.integers(1, 6))
        s = rng.integers(20, seg_hi, nseg)
        imp = list(range(1, nseg - 1)) if nseg > 2 and rng.random() < 0.7 else []
        segs.append(s)
        imps.append(imp)
        lens.append(int(s.sum() + rng.integers(0, 3 * seg_hi)))
    return segs, imps, lens, pack_pairs(segs, imps)


# (name, fragment lengths, read length, longest segment)
LAWS = [
    ("two_far_apart", [180] * 5 + [900] * 3, 75, 600),
    ("start_below_read_len", list(range(40, 60)) * 3 + [200, 260], 75, 400),
    ("start_above_read_len", list(range(300, 340)) + [360, 500], 75, 500),
    ("beyond_8192", list(range(8100, 8300, 7)) + [9000, 12000], 75, 5000),
]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,fl,rl,seg_hi", LAWS, ids=[x[0] for x in LAWS])
def test_degenerate_laws_against_reference(ctx, reflib, name, fl, rl, seg_hi):
    """Empirical laws with holes (the Normal fills them), a start offset below and above the read length (lmin), lengths
    past 8192: the host pdf table == the reference's emp_dist_pdf (1e-14), the device weights == its bin weights (1e-12)."""
    from strawberry_amd.binweight import InsertSize, bin_weights
    fl = np.asarray(fl, np.int32)
    ins = InsertSize.from_frag_lens(fl)
    assert (ins.start_offset < rl) == (name == "start_below_read_len")
    hi = int(fl.max()) + 400
    pdf, info = reflib.insert_pdf(0.0, 0.0, fl, 0, hi)
    assert ins.mean == info[0] and ins.sd == info[1] and ins.start_offset == info[2] and ins.end_offset == info[3]
    np.testing.assert_allclose(ins.pdf_table(hi + 1, rl), pdf, rtol=1e-14, atol=0)
    rng = np.random.Generator(np.random.PCG64(len(fl)))
    segs, imps, lens, (seg_off, seg_lens, mask) = random_pairs(rng, 400, seg_hi)
    w = bin_weights(seg_off, seg_lens, mask, lens, ins, rl, ctx=ctx)
    want = np.array([reflib.bin_weight(s, i, L, rl, 0.0, 0.0, fl) for s, i, L in zip(segs, imps, lens)])
    assert (want > 0).sum() > 50
    check(w, want, 1e-12)


@pytest.mark.timeout(300)
def test_one_distinct_length(ctx, reflib):
    """sd = 0: the reference (-Ofast) leaves the Normal's 0/0 undefined; the library's documented value is a density of 1
    at the one length and 0 everywhere else (sbgpu_insert_pdf_table: a NaN density is not >= the smallest normal), so
    every weight is effective_len(l0) / (L - l0 + 1) where l0 lies in the bin's range, else 0."""
    from strawberry_amd.binweight import InsertSize, bin_weights
    l0, rl = 250, 75
    ins = InsertSize.from_frag_lens([l0] * 17)
    assert ins.sd == 0.0 and ins.mean == l0
    tab = ins.pdf_table(2000, rl)
    want = np.zeros(2000)
    want[l0] = 1.0
    np.testing.assert_array_equal(tab, want)
    rng = np.random.Generator(np.random.PCG64(3))
    segs, imps, lens, (seg_off, seg_lens, mask) = random_pairs(rng, 400, 300)
    w = bin_weights(seg_off, seg_lens, mask, lens, ins, rl, ctx=ctx)
    exp = []
    for s, i, L in zip(segs, imps, lens):
        lmin = max(l0, int(np.sum(s[1:-1]))) if len(s) > 2 else l0
        ok = lmin <= l0 <= int(np.sum(s))
        exp.append(reflib.effective_len(s, i, l0, rl) / (L - l0 + 1) if ok else 0.0)
    exp = np.array(exp)
    assert (exp > 0).sum() > 20
    nz = exp != 0
    assert ((w != 0) == nz).all()
    np.testing.assert_allclose(w[nz], exp[nz], rtol=1e-14, atol=0)


# ---- the overflow slot and long reads ----------------------------------------------------------------------------------------

# (overlapping exons of one isoform, the pair's two mates, its length, the longest locus' segments together)
OVERFLOW = {
    "lds": ([(100, 200), (150, 250)], [(100, 140), (210, 250)], 202, 151),
    "global": ([(1, 6000), (1000, 7000)], [(1, 100), (6901, 7000)], 12001, 7000),
}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("route", list(OVERFLOW))
def test_length_beyond_the_longest_locus_is_refused(ctx, route):
    """Overlapping exons of one isoform count twice in exonic_overlaps_len, more than the locus' segments hold: the
    length lands in the overflow slot -- from the workgroup's LDS counters or from the global atomics -- and the call
    is refused; the length is counted nowhere in a law."""
    from strawberry_amd import _lib
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import quantify_host, quantify_resident
    exons, mates, length, seg_total = OVERFLOW[route]
    annot = eb.Annotation([[exons], [[(20000, 20100)]]])
    hs = FU.HitSet()
    (l1, r1), (l2, r2) = mates
    hs.add(0, [3], [FU.MATCH, FU.GAP, FU.MATCH], [l1, r1 + 1, l2], [r1, l2 - 1, r2])
    hs.add(1, [1], [FU.MATCH], [20000], [20099])
    hits = hs.hits()
    compat, _ = eb.compat_and_keys(annot, hits, ctx)
    ref = FU.reference(annot, hits, compat)
    seg = annot.seg_right.astype(np.int64) - annot.seg_left + 1
    assert ref["keep"].all() and ref["lens"][0] == length and seg[annot.seg_off[0]:annot.seg_off[1]].sum() == seg_total
    assert (length >= FU.LDS_BINS) == (route == "global") and length > seg_total
    with pytest.raises(_lib.SbgpuError, match="beyond the longest locus"):
        quantify_resident(annot, hits, None, RL, 2, ctx=ctx)
    with pytest.raises(_lib.SbgpuError, match="beyond the longest locus"):
        quantify_host(annot, hits, None, RL, ctx=ctx)


@pytest.mark.timeout(300)
def test_long_reads_without_a_law(ctx):
    """long_read = 1 with no law: the long-read workflow builds none (Strawberry.cpp:335-337) -- the weights are 1/L as with
    a given law, so theta and TPM equal those of the call given N(200, 80); the law in use is all zeros."""
    from strawberry_amd import _lib
    from strawberry_amd.quantify import InsertSize, quantify_host, quantify_resident
    d = U.E2E_LONGREAD
    ordered, rows, gtf, theta_log = U.load(d)
    annot, hits, names, _ = XU.e2e_inputs(d, ordered)
    given = quantify_resident(annot, hits, InsertSize(200.0, 80.0), RL, hits.total_mapped, long_read=True, ctx=ctx)
    none = quantify_resident(annot, hits, None, RL, hits.total_mapped, long_read=True, ctx=ctx)
    for k in ("theta", "status", "iters", "fpkm", "frac", "tpm", "keep"):
        np.testing.assert_array_equal(none[k], given[k], err_msg=k)
    assert none["total_mapped_reads"] == given["total_mapped_reads"] == hits.total_mapped
    law = none["insert"]
    assert not law["use_emp"] and law["mean"] == 0.0 and law["sd"] == 0.0 and law["emp_hist"] is None
    assert none["n_frag_lens"] == 0
    for l, ref_theta in enumerate(theta_log):
        th = none["theta"][annot.iso_off[l]:annot.iso_off[l + 1]]
        assert np.abs(th - np.array(ref_theta)).max() < 1e-6, names[l]
    hg = quantify_host(annot, hits, InsertSize(200.0, 80.0), RL, long_read=True, ctx=ctx)
    hn = quantify_host(annot, hits, None, RL, long_read=True, ctx=ctx)
    np.testing.assert_array_equal(hn["theta"], hg["theta"])
    np.testing.assert_array_equal(hn["F"], hg["F"])
    assert not hn["insert"]["use_emp"]
    with pytest.raises(_lib.SbgpuError, match="effective_len_norm"):
        quantify_resident(annot, hits, None, RL, hits.total_mapped, long_read=True, ctx=ctx, effective_len_norm=True)

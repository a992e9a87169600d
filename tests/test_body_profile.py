"""Transcript-body coverage profile on the host: sbgpu_body_profile_host (csrc/body_host.cpp), the CPU statement of what the device
form computes, against tests/body_util.py::by_hand -- the rule of include/sbgpu.h restated with Python floats and ints -- under the
bounds of that file's head, zeros and -1.0 exactly; the all-integer case against an int64 count; the conservation against the
isoform-resolved coverage; hand-made loci with closed forms; the refusals.

No GPU here: the hits' compat / key words and the bin weights come from the oracle's restatement, as in
tests/test_isoform_coverage.py, whose toy inputs and hand-made loci are reused."""
import ctypes as C

import numpy as np
import pytest

import body_util as BU
import retained_util as R
from strawberry_amd import _lib, body, coverage
from strawberry_amd import exonbin as eb
from test_context_table import NINE, Handle, oracle_weights, toy_inputs
from test_fragment_assign import three_loci

N_SMALL = 200
EPS = BU.EPS


def host(H, annot, hits, compat, theta, **kw):
    return body.body_profile_host(H.h, annot, hits, compat, theta, **kw)


def one_hot(annot):
    theta = np.zeros(int(annot.iso_off[-1]))
    theta[np.asarray(annot.iso_off[:-1], np.int64)] = 1.0
    return theta


def integer_count(annot, hits, assigned, strand, P):
    """The all-integer case (unit masses, one-hot theta) counted in int64 with numpy: every assigned hit adds each of its matched
    bases inside its locus' isoform 0 to the bin t * P // L of that base."""
    n_iso = int(annot.iso_off[-1])
    out = np.zeros((n_iso, P), np.int64)
    for h in np.nonzero(np.asarray(assigned, bool))[0]:
        i = int(annot.iso_off[hits.hit_locus[h]])
        e0, e1 = int(annot.exon_off[i]), int(annot.exon_off[i + 1])
        xl, xr = annot.exon_left[e0:e1].astype(np.int64), annot.exon_right[e0:e1].astype(np.int64)
        pre = np.concatenate([[0], np.cumsum(xr - xl + 1)])
        q = slice(int(hits.feat_off[h]), int(hits.feat_off[h + 1]))
        for a, b, c in zip(hits.feat_left[q].astype(np.int64), hits.feat_right[q].astype(np.int64), hits.feat_code[q]):
            if c != 0:
                continue
            for e in np.nonzero((xl <= b) & (xr >= a))[0]:
                t = pre[e] + np.arange(max(a, xl[e]), min(b, xr[e]) + 1) - xl[e]
                np.add.at(out[i], t * P // pre[-1], 1)
    if strand is not None:
        flip = np.asarray(strand) == 2
        out[flip] = out[flip, ::-1]
    return out


def conservation(t, cov, annot, hit_locus, P, exact=False):
    """sum_p body_bases[j, p] against the coverage's iso_bases[j]: every isoform of every locus"""
    hits_of, niso, iso_locus = BU.shape(annot, hit_locus)
    sums = t.body_bases.sum(axis=1)
    if exact:
        np.testing.assert_array_equal(sums, cov.iso_bases)
        return
    bound = (2.0 * hits_of[iso_locus] + np.diff(annot.exon_off) + P + 16.0) * EPS
    assert (np.abs(sums - cov.iso_bases) <= bound * cov.iso_bases).all()
    np.testing.assert_array_equal(sums[cov.iso_bases == 0.0], 0.0)


def exact_case(H, annot, hits, bins, compat, F, keep, status, strand, P):
    theta = one_hot(annot)
    t = host(H, annot, hits, compat, theta, F=F, keep=keep, status=status, iso_strand=strand, n_pos=P)
    want = BU.by_hand(bins, annot, hits, compat, F, theta, keep, status, None, strand, P)
    count = integer_count(annot, hits, want["assigned"], strand, P)
    np.testing.assert_array_equal(t.body_bases, count.astype(np.float64))
    np.testing.assert_array_equal(t.body_total, count.sum(axis=1).astype(np.float64))
    assert count.sum() > 0
    cov = coverage.isoform_coverage_host(H.h, annot, hits, compat, theta, F=F, keep=keep, status=status)
    conservation(t, cov, annot, hits.hit_locus, P, exact=True)
    BU.stats_of_own_bins(t, annot, strand, "one-hot theta, unit masses")
    return t


@pytest.mark.parametrize("which", NINE)
def test_host_form_on_the_toy_directories(oracle, which):
    d, ordered, rows, annot, hits, names, compat, key, bins, F, status, ab = toy_inputs(oracle, which)
    theta, _, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    strand = BU.strands_of(annot)
    P = 20
    with Handle(annot, hits, compat, key) as H:
        kw = dict(F=F, keep=ab["keep"], status=status)
        t = host(H, annot, hits, compat, theta, hit_mass=hits.mass, iso_strand=strand, **kw)
        t7 = host(H, annot, hits, compat, theta, iso_strand=strand, n_pos=7, **kw)
        few = host(H, annot, hits, compat, theta, hit_mass=hits.mass, iso_strand=strand, want=("body_cv", "class_n"), **kw)
        exact_case(H, annot, hits, bins, compat, F, ab["keep"], status, strand, P)
        cov = coverage.isoform_coverage_host(H.h, annot, hits, compat, theta, hit_mass=hits.mass, **kw)
    assert t.n_pos == body.N_POS == P and t.body_bases.shape == (int(annot.iso_off[-1]), P)
    want = BU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status, hits.mass, strand, P, per_base=True)
    closed = BU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status, hits.mass, strand, P)
    assert closed["body_bases"] == want["body_bases"]          # the restatement's two ways to a bin agree
    BU.compare(t, want, annot, hits.hit_locus, True, which, P, strand)
    BU.compare(t7, BU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status, None, strand, 7, per_base=True), annot, hits.hit_locus, True,
               which + ", unit masses, P = 7", 7, strand)
    conservation(t, cov, annot, hits.hit_locus, P)
    BU.stats_of_own_bins(t, annot, strand, which)
    assert few.body_bases is None and few.body_total is None and few.class_profile is None
    np.testing.assert_array_equal(few.body_cv, t.body_cv)
    np.testing.assert_array_equal(few.class_n, t.class_n)
    erased = np.asarray(ab["keep"]) == 0
    assert (t.body_total[erased] == 0.0).all() and (t.body_center[erased] == -1.0).all() and (t.body_cv[erased] == -1.0).all() and (t.body_total > 0.0).any()
    assert int(t.class_n.sum()) == int((t.body_total > 0.0).sum())
    # what the Python object adds: depth, an isoform's profile, a class' curve, the 3' bias, the rows of a TSV
    i = int(np.argmax(t.body_total))
    wd = body.bin_widths(body.iso_lengths(annot), P, strand)
    assert (wd.sum(axis=1) == body.iso_lengths(annot)).all()
    np.testing.assert_array_equal(t.depth(annot)[i], t.body_bases[i] / wd[i])
    np.testing.assert_array_equal(t.profile(i), t.body_bases[i] / t.body_total[i])
    c = int(np.argmax(t.class_n))
    np.testing.assert_array_equal(t.class_curve(c), t.class_profile[c] / float(t.class_n[c]))
    assert abs(t.class_curve(c).sum() - 1.0) <= (P + 8 + t.class_n[c]) * EPS * 4
    k = P // 5
    total = t.class_profile.sum(axis=0)
    assert t.bias_3p() == total[-k:].sum() / total[:k].sum() and t.bias_3p(c) == t.class_profile[c][-k:].sum() / t.class_profile[c][:k].sum()
    rows_ = list(t.rows(annot))
    assert len(rows_) == int(annot.iso_off[-1]) and len(rows_[i]) == 7 + P
    assert rows_[i][2] == int(body.iso_lengths(annot)[i]) and rows_[i][4:7] == (t.body_total[i], t.body_center[i], t.body_cv[i]) and rows_[i][7:] == tuple(t.body_bases[i])


@pytest.fixture(scope="module")
def S(oracle):
    annot, hits = BU.body_sample(N_SMALL, oracle=oracle)
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    F = oracle_weights(oracle, bins, oracle.make_insert(*R.LAW), False)
    theta, status, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    ab = oracle.abundance(bins.iso_off, theta, status, bins.iso_len, hits.n_hits, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    strand = BU.strands_of(annot)
    want = BU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status, hits.mass, strand, 20)
    return dict(annot=annot, hits=hits, compat=compat, key=key, bins=bins, F=F, theta=theta, status=status, keep=ab["keep"], strand=strand, want=want)


def test_host_form_on_the_edge_sample(S):
    annot, hits, strand = S["annot"], S["hits"], S["strand"]
    at = R.edge_layout(N_SMALL)
    print(BU.sample_conditions(annot, S["want"], strand, 20))
    kw = dict(F=S["F"], keep=S["keep"], status=S["status"])
    with Handle(annot, hits, S["compat"], S["key"]) as H:
        t = host(H, annot, hits, S["compat"], S["theta"], hit_mass=hits.mass, iso_strand=strand, **kw)
        t100 = host(H, annot, hits, S["compat"], S["theta"], hit_mass=hits.mass, iso_strand=strand, n_pos=100, **kw)
        t1 = host(H, annot, hits, S["compat"], S["theta"], hit_mass=hits.mass, iso_strand=strand, n_pos=1, **kw)
        cov = coverage.isoform_coverage_host(H.h, annot, hits, S["compat"], S["theta"], hit_mass=hits.mass, **kw)
        exact_case(H, annot, hits, S["bins"], S["compat"], S["F"], S["keep"], S["status"], strand, 20)
    BU.compare(t, S["want"], annot, hits.hit_locus, True, "edge sample", 20, strand)
    BU.compare(t100, BU.by_hand(S["bins"], annot, hits, S["compat"], S["F"], S["theta"], S["keep"], S["status"], hits.mass, strand, 100), annot,
               hits.hit_locus, True, "edge sample, P = 100", 100, strand)
    for x, P in ((t, 20), (t100, 100), (t1, 1)):
        conservation(x, cov, annot, hits.hit_locus, P)
        BU.stats_of_own_bins(x, annot, strand, "edge sample, P = %d" % P)
    # P = 1: one bin per isoform, the coverage's iso_bases from the same terms; centre 0.5 and cv 0.0 wherever anything lies
    some = t1.body_total > 0.0
    assert (t1.body_center[some] == 0.5).all() and (t1.body_cv[some] == 0.0).all() and (t1.body_total == t1.body_bases[:, 0]).all()
    # the loci the device form treats differently exist in this sample: either side of every threshold, by the library's constants
    lim = body.limits()
    niso, nex = np.diff(annot.iso_off), np.diff(np.asarray(annot.exon_off)[np.asarray(annot.iso_off)])
    assert set(lim) == set(body.LIMIT_NAMES) and lim["max_iso"] == 4096 and lim["max_bins"] == 5632 and lim["item_hits"] == R.ITEM_HITS
    in_lds = lambda l, P: niso[l] <= lim["lds_iso"] and nex[l] <= lim["lds_exons"] and niso[l] * P <= lim["lds_sums"]  # noqa: E731
    copies = lambda l, P: in_lds(l, P) and niso[l] <= lim["narrow_iso"] and niso[l] * P * lim["copies"] <= lim["lds_sums"]  # noqa: E731
    assert niso[at["C"]] == 300 > lim["lds_iso"] and not in_lds(at["C"], 1)
    assert in_lds(at["B"], 20) and not in_lds(at["B"], 100) and in_lds(at["T32"], 96) and not in_lds(at["T33"], 96)
    assert copies(at["T8"], 20) and not copies(at["T9"], 20) and in_lds(at["T9"], 20) and copies(at["A"], 20) and not copies(at["A"], 100)
    assert copies(at["T8"], 24) and not copies(at["T8"], 25)
    for l in (at["EMPTY"], at["NOBIN"]):
        i0, i1 = int(annot.iso_off[l]), int(annot.iso_off[l + 1])
        assert (t.body_bases[i0:i1] == 0.0).all() and (t.body_center[i0:i1] == -1.0).all() and (t.body_cv[i0:i1] == -1.0).all()


def locus(oracle, isoforms, feats):
    annot = eb.Annotation([isoforms])
    hits = eb.Hits([0] * len(feats), feats)
    compat, key = oracle.exonbin_batch(annot, hits)
    return annot, hits, compat, key, eb.LocusBins(annot, hits, compat, key)


def single(oracle, exons, reads, P, strand=0, per_base=True):
    """one isoform, single-block reads, theta = 1: every posterior is exactly 1.0, every term an integer"""
    annot, hits, compat, key, bins = locus(oracle, [exons], [eb.hit_features([r], []) for r in reads])
    assert compat[:, 0].tolist() == [1] * len(reads)
    F = np.full(bins.n_elem, 0.5)
    s = np.array([strand], np.uint8)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, np.array([1.0]), F=F, iso_strand=s, n_pos=P)
    want = BU.by_hand(bins, annot, hits, compat, F, np.array([1.0]), strand=s, n_pos=P, per_base=per_base)
    BU.bitwise(t, want, "a single isoform", P)
    return t, annot


def test_an_isoform_shorter_than_its_bins(oracle):
    """L = 7, P = 20: q(t) = 20 t // 7 = 0, 2, 5, 8, 11, 14, 17 -- thirteen bins of width 0, which depth() and body_cv pass by"""
    t, annot = single(oracle, [(101, 107)], [(101, 107), (103, 105)], 20)
    want = np.zeros(20)
    want[[0, 2, 5, 8, 11, 14, 17]] = [1, 1, 2, 2, 2, 1, 1]
    assert t.body_bases[0].tolist() == want.tolist() and t.body_total[0] == 10.0
    wd = body.bin_widths([7], 20)[0]
    assert wd.tolist() == [1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    assert t.depth(annot)[0].tolist() == want.tolist()
    d = np.array([1, 1, 2, 2, 2, 1, 1], float)
    m = d.sum() / 7.0
    assert t.body_cv[0] == np.sqrt(((d - m) ** 2).sum() / 7.0) / m      # over the seven bins that exist, not over twenty
    # mirrored: the same numbers at P - 1 - q
    r, _ = single(oracle, [(101, 107)], [(101, 107), (103, 105)], 20, strand=2)
    assert r.body_bases[0].tolist() == want[::-1].tolist() and r.body_cv[0] == t.body_cv[0]


@pytest.mark.parametrize("L", [20, 21])
def test_an_isoform_as_long_as_its_bins_and_one_base_longer(oracle, L):
    t, _ = single(oracle, [(1001, 1000 + L)], [(1001, 1000 + L)], 20)
    if L == 20:
        assert t.body_bases[0].tolist() == [1.0] * 20 and t.body_center[0] == 0.5 and t.body_cv[0] == 0.0
    else:               # ceil(21 q / 20) = q + (q > 0): bin 0 holds t = 0 and 1
        assert t.body_bases[0].tolist() == [2.0] + [1.0] * 19 and body.bin_widths([21], 20)[0].tolist() == [2] + [1] * 19 and t.body_cv[0] == 0.0


def test_bin_edges_exon_edges_and_a_hit_over_every_bin(oracle):
    """Two exons of 100 and 300 bases, P = 20: bins of 20 bases, and the exon boundary (t = 100) is the boundary of bins 4 | 5.
    X ends on the last base of bin 1 (t = 39), Y starts on the first of bin 2 (t = 40); Z crosses the exon boundary spliced;
    W covers the whole isoform."""
    ex = [(1, 100), (1001, 1300)]
    annot, hits, compat, key, bins = locus(oracle, [ex], [eb.hit_features([(21, 40)], []), eb.hit_features([(41, 65)], []),
                                                           eb.hit_features([(91, 100), (1001, 1015)], []), eb.hit_features([(1, 100), (1001, 1300)], [])])
    assert compat[:, 0].tolist() == [1, 1, 1, 1]
    F = np.full(bins.n_elem, 0.5)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, np.array([1.0]), F=F)
        plus = host(H, annot, hits, compat, np.array([1.0]), F=F, iso_strand=np.array([1], np.uint8))
        minus = host(H, annot, hits, compat, np.array([1.0]), F=F, iso_strand=np.array([2], np.uint8))
    want = np.full(20, 20.0)            # W
    want[1] += 20                       # X: t = 20 .. 39
    want[2] += 20                       # Y: t = 40 .. 64
    want[3] += 5
    want[4] += 10                       # Z: t = 90 .. 99 | 100 .. 114
    want[5] += 15
    assert t.body_bases[0].tolist() == want.tolist() and t.body_total[0] == 400.0 + 20 + 25 + 25
    BU.bitwise(t, BU.by_hand(bins, annot, hits, compat, F, np.array([1.0]), per_base=True), "edges", 20)
    BU.bitwise(plus, t, "strand 1 is strand 0", 20)
    s2 = np.array([2], np.uint8)
    BU.bitwise(minus, BU.by_hand(bins, annot, hits, compat, F, np.array([1.0]), strand=s2, per_base=True), "strand 2", 20)
    np.testing.assert_array_equal(minus.body_bases[0].view(np.uint64), t.body_bases[0, ::-1].view(np.uint64))
    assert minus.body_total[0] == t.body_total[0] and minus.body_center[0] != t.body_center[0]


def test_strand_2_is_the_mirror_image_bit_for_bit(oracle):
    """two isoforms that share their hits, fractional masses and posteriors: the bins of strand 2 are those of strand 1 at P - 1 - p"""
    annot, hits, compat, key, bins = three_loci(oracle)
    F = np.array([0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 3)
    theta = np.array([6.0, 1.0, 3.0, 2.0, 1.0, 7.0])
    mass = np.linspace(0.3, 1.7, hits.n_hits).astype(np.float32)
    n_iso = int(annot.iso_off[-1])
    with Handle(annot, hits, compat, key) as H:
        got = [host(H, annot, hits, compat, theta, F=F, hit_mass=mass, iso_strand=np.full(n_iso, s, np.uint8), n_pos=13) for s in (0, 1, 2)]
    BU.bitwise(got[0], got[1], "strand 0 and strand 1", 13)
    np.testing.assert_array_equal(got[2].body_bases.view(np.uint64), got[1].body_bases[:, ::-1].view(np.uint64))
    assert (got[1].body_bases > 0.0).sum() > 6 and (got[1].body_bases != np.round(got[1].body_bases)).any()
    BU.compare(got[2], BU.by_hand(bins, annot, hits, compat, F, theta, mass=mass, strand=np.full(n_iso, 2), n_pos=13, per_base=True), annot, hits.hit_locus,
               True, "three loci, strand 2", 13, np.full(n_iso, 2))


def test_one_bin_and_a_hundred(oracle):
    ex, reads = [(1, 150), (301, 450)], [(11, 60), (100, 140), (320, 449)]
    one, _ = single(oracle, ex, reads, 1)
    assert one.body_bases[0].tolist() == [50.0 + 41.0 + 130.0] and one.body_center[0] == 0.5 and one.body_cv[0] == 0.0
    many, _ = single(oracle, ex, reads, 100)
    assert many.body_bases.shape == (1, 100) and many.body_total[0] == 221.0 and many.body_bases[0].max() == 3.0
    for bad in (0, 101, -1):
        with pytest.raises(_lib.SbgpuError, match="n_pos must be 1 .. 100"):
            single(oracle, ex, reads, bad)


def test_a_single_exon_of_2_to_the_26_bases(oracle):
    """L * P = 100 * 2^26 > 2^32: the 64-bit division.  ceil(50 L / 100) = 2^25: a read over t = 2^25 - 33 .. 2^25 + 67"""
    L = 1 << 26
    half = 1 << 25
    t, _ = single(oracle, [(1, L)], [(1, 100), (half - 32, half + 68), (L - 99, L)], 100, per_base=False)
    first = -(-L // 100)
    assert t.body_bases[0][0] == 100.0 and t.body_bases[0][99] == 100.0 and first > 100
    assert t.body_bases[0][49] == 33.0 and t.body_bases[0][50] == 68.0 and t.body_total[0] == 301.0
    m, _ = single(oracle, [(1, L)], [(1, 100), (half - 32, half + 68), (L - 99, L)], 100, strand=2, per_base=False)
    assert m.body_bases[0].tolist() == t.body_bases[0][::-1].tolist()


def test_a_uniform_tiling_has_centre_one_half_and_no_variation(oracle):
    ex = [(1, 300), (1001, 1500)]             # 800 bases, P = 20: bins of 40
    reads = [(1 + 40 * k, 40 * k + 40) for k in range(7)] + [(281, 300)] + [(1001, 1020)] + [(1021 + 40 * k, 1060 + 40 * k) for k in range(12)]
    annot, hits, compat, key, bins = locus(oracle, [ex], [eb.hit_features([r], []) for r in reads[:7] + reads[9:]] + [eb.hit_features([(281, 300), (1001, 1020)], [])])
    F = np.full(bins.n_elem, 0.5)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, np.array([1.0]), F=F, hit_mass=np.full(hits.n_hits, 3.0, np.float32))
    assert t.body_bases[0].tolist() == [120.0] * 20 and t.body_center[0] == 0.5 and t.body_cv[0] == 0.0 and t.class_n.tolist() == [1, 0, 0, 0]
    assert t.class_profile[0].tolist() == [0.05] * 20 and t.bias_3p() == 1.0


def test_the_class_edges(oracle):
    lengths = [999, 1000, 1999, 2000, 3999, 4000]
    loci = [[[(10000 * k + 1, 10000 * k + L)]] for k, L in enumerate(lengths)]
    annot = eb.Annotation(loci)
    hits = eb.Hits(list(range(6)), [eb.hit_features([(10000 * k + 11, 10000 * k + 60)], []) for k in range(6)])
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    F = np.full(bins.n_elem, 0.5)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, np.ones(6), F=F)
        st = host(H, annot, hits, compat, np.ones(6), F=F, status=np.array([0, 1, 0, 0, 0, 0], np.int32), keep=np.array([1, 1, 1, 0, 1, 1], np.int32))
    assert t.class_n.tolist() == [1, 2, 2, 1] and [r[3] for r in t.rows(annot)] == [0, 1, 1, 2, 2, 3]
    BU.compare(t, BU.by_hand(bins, annot, hits, compat, F, np.ones(6), per_base=True), annot, hits.hit_locus, True, "class edges", 20)
    # an INIT_EMPTY locus and an erased isoform: zeros, -1.0, and in no class
    assert st.class_n.tolist() == [1, 1, 1, 1] and st.body_total.tolist()[1] == 0.0 == st.body_total.tolist()[3]
    assert st.body_center[[1, 3]].tolist() == [-1.0, -1.0] and st.body_cv[[1, 3]].tolist() == [-1.0, -1.0] and (st.body_bases[[1, 3]] == 0.0).all()
    BU.compare(st, BU.by_hand(bins, annot, hits, compat, F, np.ones(6), keep=[1, 1, 1, 0, 1, 1], status=[0, 1, 0, 0, 0, 0], per_base=True), annot, hits.hit_locus,
               True, "class edges, erased", 20)


def test_host_form_reports_what_is_missing(oracle):
    annot, hits, compat, key, bins = three_loci(oracle, with_a_hit_in_no_bin=False)
    L = _lib.load()
    F, theta = np.array([0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 3), np.array([6.0, 1.0] * 3)
    s = _lib.sbgpu_body_profile_t()
    a, h = annot._struct(), hits._struct()

    def call(handle, a_=a, h_=h, theta_=theta, strand=None, P=20, cw=1, F_=F):
        rc = L.sbgpu_body_profile_host(handle, C.byref(a_), C.byref(h_), compat.ctypes.data, cw, None if F_ is None else F_.ctypes.data,
                                       None if theta_ is None else theta_.ctypes.data, None, None, None,
                                       None if strand is None else strand.ctypes.data, P, C.byref(s))
        return rc, L.sbgpu_last_error().decode()
    with Handle(annot, hits, compat, key) as H:
        rc, why = call(H.h, theta_=None)
        assert rc == _lib.SBGPU_EINVAL and "theta is needed" in why, why
        rc, why = call(None)
        assert rc == _lib.SBGPU_EINVAL and "null argument" in why, why
        for P in (0, 101):
            rc, why = call(H.h, P=P)
            assert rc == _lib.SBGPU_EINVAL and "n_pos must be 1 .. 100" in why, why
        rc, why = call(H.h, strand=np.array([0, 1, 2, 3, 0, 0], np.uint8))
        assert rc == _lib.SBGPU_EINVAL and "iso_strand holds a value above 2" in why, why
        rc, why = call(H.h, F_=None)
        assert rc == _lib.SBGPU_EINVAL and "holds no weights" in why, why
        rc, why = call(H.h, cw=0)
        assert rc == _lib.SBGPU_EINVAL and "compat words are needed" in why, why
        fewer = R.select_hits(hits, np.arange(hits.n_hits - 1))
        rc, why = call(H.h, h_=fewer._struct())
        assert rc == _lib.SBGPU_EINVAL and "hits->n_hits is not the handle's" in why, why
        nofeat = hits._struct()
        nofeat.feat_off = None
        rc, why = call(H.h, h_=nofeat)
        assert rc == _lib.SBGPU_EINVAL and "the hits' features are needed" in why, why
        other = eb.Annotation([[[(1, 100), (201, 300)], [(1, 100), (401, 500)]]] * 2)
        rc, why = call(H.h, a_=other._struct())
        assert rc == _lib.SBGPU_EINVAL and "the annotation's loci or isoforms are not the handle's" in why, why
        ok = host(H, annot, hits, compat, theta, F=F)
        assert abs(ok.body_total.sum() - 12 * 41.0) <= 64 * EPS * 12 * 41.0
    # hits that did not come grouped by locus, one of them in no bin
    annot, hits, compat, key, bins = three_loci(oracle)
    order = np.array([4, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12])
    with Handle(annot, R.select_hits(hits, order), compat[order], key[order]) as H:
        with pytest.raises(_lib.SbgpuError, match="did not come grouped by locus"):
            host(H, annot, R.select_hits(hits, order), compat[order], np.array([6.0, 1.0] * 3), F=F)
    # a handle that holds no hit -> bin
    none, hh = _lib.sbgpu_hits_t(), C.c_void_p()
    _lib.check(L.sbgpu_bins_create(C.byref(a), C.byref(none), None, 1, 1, None, None, C.byref(hh)), "sbgpu_bins_create")
    try:
        rc, why = call(hh)
        assert rc == _lib.SBGPU_EINVAL and "holds no hit -> bin" in why, why
    finally:
        L.sbgpu_bins_destroy(hh)
    assert L.sbgpu_body_profile_limits(None) == _lib.SBGPU_EINVAL

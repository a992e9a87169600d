"""Isoform-resolved coverage on the host: sbgpu_isoform_coverage_host (csrc/coverage_host.cpp), the CPU statement of what the
device form computes, against tests/coverage_util.py::by_hand -- the rule of include/sbgpu.h restated with Python floats and
loops over every (feature, exon) pair -- under (2 hits + niso + 16) * 2^-52 relative, zeros exactly; hand-made loci with closed
forms; the conservation of the matched bases; the all-integer case exactly; the refusals.

No GPU here: the hits' compat / key words and the bin weights come from the oracle's restatement, as in
tests/test_fragment_assign.py, whose toy inputs and hand-made loci are reused."""
import ctypes as C

import numpy as np
import pytest

import coverage_util as CU
import retained_util as R
from strawberry_amd import _lib, coverage
from strawberry_amd import exonbin as eb
from test_context_table import NINE, Handle, oracle_weights, toy_inputs
from test_fragment_assign import three_loci

N_SMALL = 200


def host(H, annot, hits, compat, theta, **kw):
    return coverage.isoform_coverage_host(H.h, annot, hits, compat, theta, **kw)


def one_hot(annot):
    """theta = 1 on every locus' isoform 0, 0 elsewhere"""
    theta = np.zeros(int(annot.iso_off[-1]))
    theta[np.asarray(annot.iso_off[:-1], np.int64)] = 1.0
    return theta


def integer_count(annot, hits, want):
    """The all-integer case (unit masses, one-hot theta) counted in int64 with numpy: every assigned hit adds its overlaps to the
    exons of its locus' isoform 0, every unassigned hit its matched bases to its locus."""
    n_exon = int(annot.exon_off[-1])
    bases, junc, unexpl = np.zeros(n_exon, np.int64), np.zeros(n_exon, np.int64), np.zeros(annot.n_loci, np.int64)
    is_match = hits.feat_code == 0
    flen = np.where(is_match, hits.feat_right.astype(np.int64) - hits.feat_left.astype(np.int64) + 1, 0)
    matchlen = np.add.reduceat(np.concatenate([flen, [0]]), hits.feat_off[:-1]) * (np.diff(hits.feat_off) > 0)
    assigned = np.asarray(want["assigned"], bool)
    np.add.at(unexpl, hits.hit_locus[~assigned], matchlen[~assigned])
    for h in np.nonzero(assigned)[0]:
        i = int(annot.iso_off[hits.hit_locus[h]])
        e0, e1 = int(annot.exon_off[i]), int(annot.exon_off[i + 1])
        L, Rr = annot.exon_left[e0:e1].astype(np.int64), annot.exon_right[e0:e1].astype(np.int64)
        q = slice(int(hits.feat_off[h]), int(hits.feat_off[h + 1]))
        fl, fr, fc = hits.feat_left[q].astype(np.int64), hits.feat_right[q].astype(np.int64), hits.feat_code[q]
        ov = np.maximum(0, np.minimum(Rr[:, None], fr[None, :]) - np.maximum(L[:, None], fl[None, :]) + 1) * (fc == 0)[None, :]
        bases[e0:e1] += ov.sum(axis=1)
        if e1 - e0 > 1:
            spans = (fc == 1)[None, :] & (fl[None, :] == Rr[:-1, None] + 1) & (fr[None, :] == L[1:, None] - 1)
            junc[e0:e1 - 1] += spans.sum(axis=1)
    return bases, junc, unexpl


def exact_case(H, annot, hits, bins, compat, F, keep, status):
    """unit masses and a one-hot theta: every term is an integer, so the sums are exact in any order"""
    theta = one_hot(annot)
    t = host(H, annot, hits, compat, theta, F=F, keep=keep, status=status)
    want = CU.by_hand(bins, annot, hits, compat, F, theta, keep, status)
    bases, junc, unexpl = integer_count(annot, hits, want)
    np.testing.assert_array_equal(t.exon_bases, bases.astype(np.float64))
    np.testing.assert_array_equal(t.junction_mass, junc.astype(np.float64))
    np.testing.assert_array_equal(t.unexplained_bases, unexpl.astype(np.float64))
    np.testing.assert_array_equal(t.iso_bases, np.add.reduceat(np.concatenate([bases, [0]]), annot.exon_off[:-1]) * (np.diff(annot.exon_off) > 0))
    assert bases.sum() > 0 and junc.sum() > 0
    return t, want


@pytest.mark.parametrize("which", NINE)
def test_host_form_on_the_toy_directories(oracle, which):
    d, ordered, rows, annot, hits, names, compat, key, bins, F, status, ab = toy_inputs(oracle, which)
    theta, _, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, theta, F=F, keep=ab["keep"], status=status, hit_mass=hits.mass)
        t_unit = host(H, annot, hits, compat, theta, F=F, keep=ab["keep"], status=status)
        few = host(H, annot, hits, compat, theta, F=F, keep=ab["keep"], status=status, hit_mass=hits.mass, want=("iso_bases",))
        exact_case(H, annot, hits, bins, compat, F, ab["keep"], status)
    want = CU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status, hits.mass)
    CU.compare(t, want, annot, hits.hit_locus, True, which)
    CU.compare(t_unit, CU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status), annot, hits.hit_locus, True, which + ", unit masses")
    CU.conservation(t, want, annot, hits.hit_locus, which)
    # iso_bases is a function of exon_bases' bits, asked for alone or not; an erased isoform holds nothing
    np.testing.assert_array_equal(t.iso_bases, CU.iso_bases_of(t.exon_bases, annot))
    assert few.exon_bases is None and few.unexplained_bases is None
    np.testing.assert_array_equal(few.iso_bases, t.iso_bases)
    erased = np.asarray(ab["keep"]) == 0
    assert (t.iso_bases[erased] == 0.0).all() and (t.iso_bases > 0.0).any() and (t.junction_mass > 0.0).any()
    # depth, and the rows of a TSV
    depth = t.exon_depth(annot)
    rows_ = list(t.rows(annot))
    assert len(rows_) == int(annot.exon_off[-1]) and rows_[0][:3] == (0, 0, 0)
    e = int(np.argmax(t.exon_bases))
    assert rows_[e][5] == t.exon_bases[e] and rows_[e][6] == depth[e] == t.exon_bases[e] / (int(annot.exon_right[e]) - int(annot.exon_left[e]) + 1)
    i = int(np.argmax(t.iso_bases))
    length = sum(int(annot.exon_right[x]) - int(annot.exon_left[x]) + 1 for x in range(int(annot.exon_off[i]), int(annot.exon_off[i + 1])))
    assert t.iso_depth(annot)[i] == t.iso_bases[i] / length


@pytest.fixture(scope="module")
def S(oracle):
    annot, hits = R.edge_sample(N_SMALL, oracle=oracle)
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    F = oracle_weights(oracle, bins, oracle.make_insert(*R.LAW), False)
    theta, status, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    ab = oracle.abundance(bins.iso_off, theta, status, bins.iso_len, hits.n_hits, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    want = CU.by_hand(bins, annot, hits, compat, F, theta, ab["keep"], status, hits.mass)
    return dict(annot=annot, hits=hits, compat=compat, key=key, bins=bins, F=F, theta=theta, status=status, keep=ab["keep"], want=want)


def test_host_form_on_the_edge_sample(S):
    annot, hits = S["annot"], S["hits"]
    at = R.edge_layout(N_SMALL)
    fig = CU.sample_conditions(annot, hits, S["want"], nobin_locus=at["NOBIN"])
    print(fig)
    with Handle(annot, hits, S["compat"], S["key"]) as H:
        t = host(H, annot, hits, S["compat"], S["theta"], F=S["F"], keep=S["keep"], status=S["status"], hit_mass=hits.mass)
        exact_case(H, annot, hits, S["bins"], S["compat"], S["F"], S["keep"], S["status"])
    CU.compare(t, S["want"], annot, hits.hit_locus, True, "edge sample")
    CU.conservation(t, S["want"], annot, hits.hit_locus, "edge sample")
    np.testing.assert_array_equal(t.iso_bases, CU.iso_bases_of(t.exon_bases, annot))
    # the loci the device form treats differently exist in this sample too: either side of every threshold
    lim = coverage.limits()
    niso, nex = np.diff(annot.iso_off), np.diff(np.asarray(annot.exon_off)[np.asarray(annot.iso_off)])
    assert nex[at["C"]] > lim["lds_exons"] and lim["lds_iso"] == lim["lds_exons"]
    assert all(nex[at[k]] <= lim["lds_exons"] for k in R.SPECIAL if k != "C")
    assert niso[at["T8"]] == lim["narrow_iso"] and nex[at["T8"]] <= lim["copy_exons"] and niso[at["T9"]] == lim["narrow_iso"] + 1
    assert niso[at["A"]] <= lim["narrow_iso"] and nex[at["A"]] <= lim["copy_exons"]
    assert niso[at["T1024"]] <= lim["narrow_iso"] and nex[at["T1024"]] > lim["copy_exons"]
    assert lim["copy_exons"] * lim["copies"] <= lim["lds_exons"] and lim["item_hits"] == R.ITEM_HITS
    e, n = at["EMPTY"], at["NOBIN"]
    assert t.unexplained_bases[e] == 0.0 and t.unexplained_bases[n] > 0.0
    for l in (e, n):
        assert (t.iso_bases[annot.iso_off[l]:annot.iso_off[l + 1]] == 0.0).all()


def locus(oracle, isoforms, feats):
    annot = eb.Annotation([isoforms])
    hits = eb.Hits([0] * len(feats), feats)
    compat, key = oracle.exonbin_batch(annot, hits)
    return annot, hits, compat, key, eb.LocusBins(annot, hits, compat, key)


def test_a_hit_split_over_two_isoforms_that_share_an_exon(oracle):
    """A = [1-100],[201-300]; B = [1-100],[401-500].  X lies in the shared exon (40 bases): one bin of its own, so c_j = F_j,
    W = 1 and its posterior is theta's own split 0.25 : 0.75.  Y (30 bases of A's second exon) and Z (20 of B's) are theirs alone."""
    annot, hits, compat, key, bins = locus(oracle, [[(1, 100), (201, 300)], [(1, 100), (401, 500)]],
                                           [eb.hit_features([(11, 50)], []), eb.hit_features([(211, 240)], []), eb.hit_features([(411, 430)], [])])
    assert compat[:, 0].tolist() == [3, 1, 2] and bins.hit_bin.tolist() == [0, 1, 2]
    F = np.array([0.5, 0.25, 0.5, 0.0, 0.0, 0.25])
    theta = np.array([1.0, 3.0])
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, theta, F=F)
        m = host(H, annot, hits, compat, theta, F=F, hit_mass=np.array([2.0, 0.5, 1.0], np.float32))
    # X: num_A = 1 * (0.5 / 1.0) = 0.5, num_B = 3 * (0.25 / 0.5) = 1.5: 0.25 : 0.75
    assert t.exon_bases.tolist() == [0.25 * 40, 30.0, 0.75 * 40, 20.0] and t.junction_mass.tolist() == [0.0] * 4
    assert t.iso_bases.tolist() == [40.0, 50.0] and t.unexplained_bases.tolist() == [0.0]
    assert m.exon_bases.tolist() == [2.0 * 0.25 * 40, 0.5 * 30, 2.0 * 0.75 * 40, 20.0] and m.iso_bases.tolist() == [35.0, 80.0]
    assert t.exon_depth(annot).tolist() == [0.1, 0.3, 0.3, 0.2] and t.iso_depth(annot).tolist() == [0.2, 0.25]
    CU.compare(t, CU.by_hand(bins, annot, hits, compat, F, theta), annot, hits.hit_locus, True, "split")


def test_a_spliced_read_supports_the_junction_a_pair_across_it_does_not(oracle):
    """One isoform [1-100],[201-300].  S: a read of 81-100 + 201-220 (S_INTRON 101-200).  P: mates 61-90 and 211-250, whose
    unsequenced gap 91-210 spans the intron (S_GAP): it supports no junction, and the gap's bases are not counted."""
    S_ = eb.hit_features([(81, 100), (201, 220)], [])
    P = eb.hit_features([(61, 90)], [(211, 250)])
    assert [int(c) for c in S_[0]] == [0, 1, 0] and 2 in [int(c) for c in P[0]] and 1 not in [int(c) for c in P[0]]
    annot, hits, compat, key, bins = locus(oracle, [[(1, 100), (201, 300)]], [S_, P])
    assert compat[:, 0].tolist() == [1, 1]
    F = np.full(bins.n_elem, 0.5)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, np.array([1.0]), F=F, hit_mass=np.array([0.5, 1.0], np.float32))
    assert t.junction_mass.tolist() == [0.5, 0.0]                       # the spliced read alone
    assert t.exon_bases.tolist() == [0.5 * 20 + 30.0, 0.5 * 20 + 40.0]    # the gap's bases are not sequenced: they add nothing
    assert t.iso_bases.tolist() == [90.0] and t.unexplained_bases.tolist() == [0.0]


def test_a_read_overhanging_an_exon_end_and_hits_nobody_explains(oracle):
    """three_loci(): isoforms A = [1-100],[201-300], C = [1-100],[401-500] per locus.  Locus 0's C-only bin is dead, locus 1 holds a
    hit in no bin, locus 2 never started (INIT_EMPTY): all of those hits are unexplained, with their matched bases."""
    annot, hits, compat, key, bins = three_loci(oracle)
    F = np.array([0.5, 0.0, 0.0, 1e-5, 0.25, 0.25] + [0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 2)
    theta = np.array([6.0, 1.0, 6.0, 0.0, 6.0, 1.0])
    status = np.array([0, 0, _lib.EM_INIT_EMPTY], np.int32)
    keep = np.array([1, 1, 1, 1, 1, 1], np.int32)
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, theta, F=F, status=status, keep=keep)
        erased = host(H, annot, hits, compat, theta, F=F, status=status, keep=np.array([0, 1, 1, 1, 1, 1], np.int32))
    want = CU.by_hand(bins, annot, hits, compat, F, theta, keep, status)
    CU.compare(t, want, annot, hits.hit_locus, True, "three loci")
    assert CU.conservation(t, want, annot, hits.hit_locus, "three loci") == 0.0
    # every hit is one block of 41 bases; locus 0: the hit of the dead bin; locus 1: the hit in no bin, and the C-only hit whose
    # only candidate has theta = 0 (a zero denominator); locus 2: all four
    assert t.unexplained_bases.tolist() == [41.0, 82.0, 164.0]
    assert (t.exon_bases[8:] == 0.0).all() and (t.iso_bases[4:] == 0.0).all()
    # locus 1, theta_C = 0: the hit of both goes to A entirely; C holds nothing
    assert t.iso_bases[2:4].tolist() == [123.0, 0.0]
    # A erased in locus 0: its two hits have no candidate (unexplained), the hit of both is C's alone -- but C's column is the
    # dead bin's and the shared one's: c_C = 0.25, fine -- so C gets its 41 bases
    assert erased.iso_bases[:2].tolist() == [0.0, 41.0] and erased.unexplained_bases[0] == 3 * 41.0
    # a read over the end of an exon by 3 bases: 98-100 inside, 101-103 outside -> the locus is left out of the conservation
    a2, h2, c2, k2, b2 = locus(oracle, [[(1, 100), (201, 300)], [(1, 300)]], [eb.hit_features([(81, 103)], [])])
    assert c2[:, 0].tolist() == [2]
    F2 = np.full(b2.n_elem, 0.5)
    with Handle(a2, h2, c2, k2) as H:
        t2 = host(H, a2, h2, c2, np.array([1.0, 1.0]), F=F2)
        keep_a = np.array([1, 0], np.int32)
        t3 = host(H, a2, h2, c2, np.array([1.0, 1.0]), F=F2, keep=keep_a)
    assert t2.exon_bases.tolist() == [0.0, 0.0, 23.0] and t3.unexplained_bases.tolist() == [23.0] and (t3.exon_bases == 0.0).all()


def test_an_overhang_is_counted_inside_the_exon_only(oracle):
    """The walk itself (no compat test in between): a hit compatible by construction with an isoform whose exon ends 3 bases before
    the read does.  Isoform [1-100],[201-300]; the read 81-100 + 201-220 is spliced as the isoform; the same words are given to a
    hit 78-103 ... which the exon-bin kernel would refuse -- so the words are written by hand."""
    annot = eb.Annotation([[[(1, 100), (201, 300)]]])
    hits = eb.Hits([0, 0], [eb.hit_features([(81, 100), (201, 220)], []), eb.hit_features([(78, 103)], [])])
    compat, key = np.array([[1], [1]], np.uint32), np.array([[1], [1]], np.uint32)
    bins = eb.LocusBins(annot, hits, compat, key)
    assert bins.n_bins == 1
    with Handle(annot, hits, compat, key) as H:
        t = host(H, annot, hits, compat, np.array([1.0]), F=np.array([0.5]))
    want = CU.by_hand(bins, annot, hits, compat, np.array([0.5]), np.array([1.0]))
    assert t.exon_bases.tolist() == [20.0 + 23.0, 20.0] and t.junction_mass.tolist() == [1.0, 0.0]
    assert want["outside"] == [True] and want["matched"] == [66.0] and t.iso_bases.tolist() == [63.0]
    with pytest.raises(AssertionError):         # three bases are nobody's: the locus may be left out, and only such loci
        CU.conservation(t, want, annot, hits.hit_locus, "overhang", most_left_out=0.0)
    CU.compare(t, want, annot, hits.hit_locus, True, "overhang")


def test_ungrouped_hits_that_all_have_bins(oracle):
    annot, hits, compat, key, bins = three_loci(oracle)
    order = np.array([4, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12])      # locus 1's first hit in front of locus 0's
    F = np.array([0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 3)
    theta = np.array([6.0, 1.0] * 3)
    with Handle(annot, R.select_hits(hits, order), compat[order], key[order]) as H:
        with pytest.raises(_lib.SbgpuError, match="did not come grouped by locus"):
            host(H, annot, R.select_hits(hits, order), compat[order], theta, F=F)
    binned = order[order != 7]
    sh = R.select_hits(hits, binned)
    with Handle(annot, sh, compat[binned], key[binned]) as H:
        t = host(H, annot, sh, compat[binned], theta, F=F)
    sb = eb.LocusBins(annot, sh, compat[binned], key[binned])
    want = CU.by_hand(sb, annot, sh, compat[binned], F, theta)
    CU.compare(t, want, annot, sh.hit_locus, True, "ungrouped")
    assert t.unexplained_bases.tolist() == [0.0, 0.0, 0.0] and abs(t.iso_bases.sum() - 12 * 41.0) <= 64 * CU.EPS * 12 * 41.0


def test_host_form_reports_what_is_missing(oracle):
    annot, hits, compat, key, bins = three_loci(oracle, with_a_hit_in_no_bin=False)
    L = _lib.load()
    F, theta = np.array([0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 3), np.array([6.0, 1.0] * 3)
    s = _lib.sbgpu_isoform_coverage_t()
    a, h = annot._struct(), hits._struct()

    def call(handle, a_=a, h_=h, theta_=theta):
        rc = L.sbgpu_isoform_coverage_host(handle, C.byref(a_), C.byref(h_), compat.ctypes.data, 1, F.ctypes.data,
                                           None if theta_ is None else theta_.ctypes.data, None, None, None, C.byref(s))
        return rc, L.sbgpu_last_error().decode()
    with Handle(annot, hits, compat, key) as H:
        rc, why = call(H.h, theta_=None)
        assert rc == _lib.SBGPU_EINVAL and "theta is needed" in why, why
        assert call(None)[0] == _lib.SBGPU_EINVAL
        with pytest.raises(_lib.SbgpuError, match="holds no weights"):
            host(H, annot, hits, compat, theta)
        # the hits or the annotation of another call
        fewer = R.select_hits(hits, np.arange(hits.n_hits - 1))
        rc, why = call(H.h, h_=fewer._struct())
        assert rc == _lib.SBGPU_EINVAL and "hits->n_hits is not the handle's" in why, why
        other = eb.Annotation([[[(1, 100), (201, 300)], [(1, 100), (401, 500)]]] * 2)
        rc, why = call(H.h, a_=other._struct())
        assert rc == _lib.SBGPU_EINVAL and "the annotation's loci or isoforms are not the handle's" in why, why
        wider = eb.Annotation([[[(1, 100), (201, 300)], [(1, 100), (401, 500)], [(1, 500)]]] + [[[(1, 100), (201, 300)]]] * 2)
        rc, why = call(H.h, a_=wider._struct())
        assert rc == _lib.SBGPU_EINVAL and "the annotation's loci or isoforms are not the handle's" in why, why
        ok = host(H, annot, hits, compat, theta, F=F)
        assert abs(ok.iso_bases.sum() - 12 * 41.0) <= 64 * CU.EPS * 12 * 41.0
    # a handle that holds no hit -> bin
    none, hh = _lib.sbgpu_hits_t(), C.c_void_p()
    _lib.check(L.sbgpu_bins_create(C.byref(a), C.byref(none), None, 1, 1, None, None, C.byref(hh)), "sbgpu_bins_create")
    try:
        rc, why = call(hh)
        assert rc == _lib.SBGPU_EINVAL and "holds no hit -> bin" in why, why
    finally:
        L.sbgpu_bins_destroy(hh)
    lim = coverage.limits()
    assert set(lim) == set(coverage.LIMIT_NAMES) and lim["max_iso"] == 4096 and lim["max_bins"] == 5632

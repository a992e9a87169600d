"""Splicing events on the CPU (sbgpu_splice_events_shapes_host / _build_host, sbgpu_splice_psi_host, sbgpu_splice_support_host;
DESIGN 3.27): the table against tests/splice_util.py::by_hand on the sample and on every hand-made locus alone, the expected events
of the hand-made loci, PSI and defined_count against psi_by_hand bit for bit (no tolerance: IEEE addition and division in the
rule's order), 0 <= psi <= 1, the closed forms, the support against a Python loop, the result holder, and every refusal with its text."""
import ctypes as C

import numpy as np
import pytest

import splice_util as SU
from strawberry_amd import _lib, splice
from strawberry_amd import exonbin as eb

N_SMALL = 150
ROWS = (1, 2, 65)


@pytest.fixture(scope="module")
def sample():
    annot, loci, at = SU.splice_annotation(N_SMALL)
    events = splice.SpliceEvents.build(annot)
    want = SU.by_hand(loci)
    return dict(annot=annot, loci=loci, at=at, events=events, want=want)


def event_of(want, l, kind, left, right):
    u = [u for u in range(want["event_kind"].size) if (want["event_locus"][u], want["event_kind"][u], want["event_left"][u], want["event_right"][u]) ==
         (l, kind, left, right)]
    assert len(u) == 1, (l, kind, left, right)
    return u[0]


def test_the_table_equals_the_restatement_on_the_sample(sample):
    SU.assert_same_table(sample["events"], sample["want"], "the sample")
    ev = sample["events"]
    assert ev.n_loci == sample["annot"].n_loci and ev.n_iso == int(sample["annot"].iso_off[-1]) and ev.n_exons == sample["annot"].exon_left.size
    # ordered by (left, right, kind) inside every locus
    for l in range(ev.n_loci):
        s = slice(int(ev.event_off[l]), int(ev.event_off[l + 1]))
        keys = list(zip(ev.event_left[s].tolist(), ev.event_right[s].tolist(), ev.event_kind[s].tolist()))
        assert keys == sorted(set(keys))
        assert (ev.event_locus[s] == l).all()


@pytest.mark.parametrize("name", list(SU.HAND))
def test_every_hand_made_locus_alone(name):
    loci = [SU.shifted(SU.HAND[name], 5000)]
    want = SU.by_hand(loci)
    ev = splice.SpliceEvents.build(eb.Annotation(loci))
    SU.assert_same_table(ev, want, name)
    B = 5000
    n = ev.n_events
    flag = lambda kind, a, b: int(ev.event_flags[event_of(want, 0, kind, a + B, b + B)])  # noqa: E731
    if name == "cassette":
        assert n == 6 and flag(0, 200, 299) == SU.INTERNAL | SU.SKIPPED
    elif name == "retained":
        assert flag(1, 100, 199) == SU.RETAINED
    elif name == "altss":
        assert n == 7
    elif name == "alttss":
        u = event_of(want, 0, 0, B, B + 99)
        assert want["span"][u] == [0] and ev.n_span[u] == 1 and flag(0, 200, 299) == SU.FIRST | SU.SKIPPED
    elif name == "exon_is_intron":
        u, w = event_of(want, 0, 0, B + 100, B + 199), event_of(want, 0, 1, B + 100, B + 199)
        assert w == u + 1
    elif name == "abut":
        introns = ev.event_kind == 1
        assert n == 5 and list(zip(ev.event_left[introns] - B, ev.event_right[introns] - B)) == [(100, 399), (200, 399)]
    elif name == "dup":
        assert n == 3 and np.diff(ev.incl_off).tolist() == [2, 2, 2]
    elif name == "single":
        assert n == 1 and int(ev.event_flags[0]) == SU.FIRST | SU.LAST
    else:
        assert n == 0 and ev.n_incl == 0 and ev.event_off.tolist() == [0, 0]


def erase_locus(keep, annot, l):
    keep = keep.copy()
    keep[:, int(annot.iso_off[l]):int(annot.iso_off[l + 1])] = 0
    return keep


@pytest.mark.parametrize("n_rows", ROWS)
def test_psi_equals_the_restatement_bit_for_bit(sample, n_rows):
    ev, want, annot, at = sample["events"], sample["want"], sample["annot"], sample["at"]
    x, keep = SU.random_rows(n_rows, ev.n_iso, 100 + n_rows)
    keep = erase_locus(keep, annot, at["cassette"])            # an all-erased locus: NaN in every row
    for k, what in ((keep, "keep of 0 / 1 / 2"), (None, "a NULL keep")):
        psi, defined = splice.splice_psi_host(ev, x, k)
        wpsi, wdefined = SU.psi_by_hand(want, x, k)
        SU.same_bits(psi, wpsi, what)
        np.testing.assert_array_equal(defined, wdefined, err_msg=what)
        ok = ~np.isnan(psi)
        assert ((psi[ok] >= 0.0) & (psi[ok] <= 1.0)).all() and (ok.sum(axis=0) == defined).all()
        if k is not None:
            s = slice(int(ev.event_off[at["cassette"]]), int(ev.event_off[at["cassette"] + 1]))
            assert np.isnan(psi[:, s]).all() and (defined[s] == 0).all()
            print(SU.sample_conditions(want, k, wdefined, n_rows))
    # a NaN in x: NaN wherever that isoform is added, nothing else changes
    j = int(annot.iso_off[at["W40"]]) + 3
    xn = x.copy()
    xn[0, j] = np.nan
    keep[0, j] = 1
    psi_n, def_n = splice.splice_psi_host(ev, xn, keep)
    wpsi_n, wdef_n = SU.psi_by_hand(want, xn, keep)
    SU.same_bits(psi_n, wpsi_n, "a NaN in x")
    np.testing.assert_array_equal(def_n, wdef_n)
    s = slice(int(ev.event_off[at["W40"]]), int(ev.event_off[at["W40"] + 1]))
    spans = np.array([3 in want["span"][u] for u in range(s.start, s.stop)])
    assert spans.any() and np.isnan(psi_n[0, s][spans]).all()


def test_closed_forms():
    loci = [SU.shifted(SU.HAND["cassette"], 1000), SU.shifted(SU.HAND["dup"], 40000)]
    want = SU.by_hand(loci)
    ev = splice.SpliceEvents.build(eb.Annotation(loci))
    psi, defined = splice.splice_psi_host(ev, np.array([3.0, 1.0, 0.25, 7.0]))
    assert psi[0, event_of(want, 0, 0, 1200, 1299)] == 0.75 and psi[0, event_of(want, 0, 1, 1100, 1399)] == 0.25
    assert (psi[0, int(ev.event_off[1]):] == 1.0).all() and (defined == 1).all()
    assert ev.alternative().tolist() == [False, True, True, True, True, False, False, False, False]
    # a one-dimensional x is one row; keep of the same shape
    psi1, _ = splice.splice_psi_host(ev, np.array([3.0, 1.0, 0.25, 7.0]), np.array([1, 0, 1, 1]))
    assert psi1[0, event_of(want, 0, 0, 1200, 1299)] == 1.0 and psi1[0, event_of(want, 0, 1, 1100, 1399)] == 0.0


def test_support_equals_a_python_loop(sample):
    ev, want = sample["events"], sample["want"]
    rng = np.random.default_rng(5)
    xb, jm = rng.gamma(2.0, 50.0, ev.n_exons), rng.gamma(1.0, 3.0, ev.n_exons)
    for a, b in ((xb, jm), (xb, None), (None, jm), (None, None)):
        got = splice.splice_support_host(ev, a, b)
        assert got.tobytes() == SU.support_by_hand(want, a, b).tobytes()
    only = splice.splice_support_host(ev, xb, None)
    assert (only[ev.event_kind == 1] == 0.0).all() and (only[ev.event_kind == 0] > 0.0).all()


def test_the_result_holder(sample):
    ev = sample["events"]
    x, keep = SU.random_rows(3, ev.n_iso, 9)
    psi, defined = splice.splice_psi_host(ev, x, keep)
    r = splice.SplicePsi(ev, psi[0], lo=psi.min(axis=0), hi=psi.max(axis=0), defined_count=defined, support=np.ones(ev.n_events))
    rows = list(r.rows())
    assert len(rows) == ev.n_events and r.header() == ("locus", "kind", "left", "right", "flags", "n_incl", "n_span", "psi", "lo", "hi", "defined_count", "support")
    assert all(len(row) == len(r.header()) for row in rows)
    u = int(np.nonzero(ev.event_flags == (SU.INTERNAL | SU.SKIPPED))[0][0])
    assert rows[u][1] == "exon" and rows[u][4] == "INTERNAL|SKIPPED" and rows[u][5] == int(np.diff(ev.incl_off)[u])
    np.testing.assert_array_equal(r.alternative(), np.diff(ev.incl_off) != ev.n_span)
    assert r.mean is None and r.rep is None and splice.flag_words(0) == "-"
    c = ev.census()
    assert c["events"] == ev.n_events and c["exon_events"] + c["intron_events"] == ev.n_events and c["skipped"] > 0 and c["retained"] > 0
    with pytest.raises(ValueError, match="unknown arrays"):
        splice.SplicePsi(ev, psi[0], median=psi[0])
    lim = splice.limits()
    assert lim == {"mask_iso": 64, "threads": 256}


def refuse(rc, text):
    assert rc == _lib.SBGPU_EINVAL, rc
    why = _lib.load().sbgpu_last_error().decode()
    assert text in why, why


def test_refusals_of_the_build():
    L = _lib.load()
    shape = (C.c_int64 * 2)()

    def shapes(loci=None, iso_off=None, exon_off=None, left=None, right=None, null=()):
        a = eb.Annotation(loci or [SU.HAND["cassette"]])
        for k, v in (("iso_off", iso_off), ("exon_off", exon_off), ("exon_left", left), ("exon_right", right)):
            if v is not None:
                setattr(a, k, np.asarray(v, getattr(a, k).dtype))
        s = a._struct()
        for k in null:
            setattr(s, k, None)
        return L.sbgpu_splice_events_shapes_host(C.byref(s), shape), a
    refuse(L.sbgpu_splice_events_shapes_host(None, shape), "null argument")
    refuse(shapes(null=("iso_off",))[0], "null offsets")
    refuse(shapes(null=("exon_off",))[0], "null offsets")
    refuse(shapes(null=("exon_left",))[0], "exons are needed")
    two = [SU.HAND["cassette"], SU.shifted(SU.HAND["dup"], 9000)]
    refuse(shapes(two, iso_off=[0, 4, 2])[0], "isoform offsets descend")
    refuse(shapes(exon_off=[0, 5, 3])[0], "exon offsets descend")
    refuse(shapes(left=[0, 200, 400, 0, 90])[0], "not ascending and disjoint")         # overlaps the exon before it
    refuse(shapes(left=[0, 200, 400, 0, 400], right=[99, 299, 499, 99, 399])[0], "not ascending and disjoint")   # ends before it begins
    refuse(shapes(left=[200, 0, 400, 0, 400], right=[299, 99, 499, 99, 499])[0], "not ascending and disjoint")   # descending
    rc, a = shapes()
    assert rc == _lib.SBGPU_OK and list(shape) == [6, 8]
    ev = splice.SpliceEvents.build(a)
    s, st = ev._struct(), a._struct()
    s.n_events = 5
    refuse(L.sbgpu_splice_events_build_host(C.byref(st), C.byref(s)), "not this annotation's")
    s = ev._struct()
    s.n_span = None
    refuse(L.sbgpu_splice_events_build_host(C.byref(st), C.byref(s)), "null array")
    refuse(L.sbgpu_splice_events_build_host(C.byref(st), None), "null argument")


def test_refusals_of_the_host_forms(sample):
    L = _lib.load()
    loci = [SU.HAND["cassette"], SU.shifted(SU.HAND["altss"], 9000)]
    ev = splice.SpliceEvents.build(eb.Annotation(loci))
    x = np.ones(ev.n_iso)
    psi, sup = np.zeros(ev.n_events), np.zeros(ev.n_events)

    def both(text, **changed):
        t = splice.SpliceEvents()
        t.__dict__.update(ev.__dict__)
        for k, (at, v) in changed.items():
            a = getattr(ev, k).copy()
            a[at] = v
            setattr(t, k, a)
        s = t._struct()
        refuse(L.sbgpu_splice_psi_host(C.byref(s), 1, x.ctypes.data, None, psi.ctypes.data, None), text)
        refuse(L.sbgpu_splice_support_host(C.byref(s), None, None, sup.ctypes.data), text)
    both("event offsets descend", event_off=(1, ev.n_events + 1))
    both("isoform offsets descend", iso_off=(1, ev.n_iso + 1))
    both("inclusion offsets descend", incl_off=(3, 0))
    both("incl_off does not run", incl_off=(ev.n_events, ev.n_incl + 1))
    both("an incl_iso outside its locus", incl_iso=(0, 2))         # the cassette has isoforms 0 and 1
    both("an incl_iso outside its locus", incl_iso=(0, -1))
    both("an incl_exon outside the exons", incl_exon=(ev.n_incl - 1, ev.n_exons))
    both("an incl_exon outside the exons", incl_exon=(0, -1))
    both("an event_locus outside the loci", event_locus=(0, 2))
    s = ev._struct()
    refuse(L.sbgpu_splice_psi_host(None, 1, x.ctypes.data, None, psi.ctypes.data, None), "null argument")
    refuse(L.sbgpu_splice_psi_host(C.byref(s), 1, None, None, psi.ctypes.data, None), "x is needed")
    refuse(L.sbgpu_splice_psi_host(C.byref(s), 1, x.ctypes.data, None, None, None), "psi is needed")
    refuse(L.sbgpu_splice_psi_host(C.byref(s), -1, x.ctypes.data, None, psi.ctypes.data, None), "negative row count")
    refuse(L.sbgpu_splice_support_host(C.byref(s), None, None, None), "support is needed")
    s.incl_iso = None
    refuse(L.sbgpu_splice_support_host(C.byref(s), None, None, sup.ctypes.data), "inclusion lists are needed")
    with pytest.raises(ValueError, match="n_rows, n_iso"):
        splice.splice_psi_host(ev, np.ones(ev.n_iso + 1))
    with pytest.raises(ValueError, match="are needed"):
        splice.splice_support_host(ev, np.ones(ev.n_exons - 1))
    # no rows: nothing to write, every count 0
    _, defined = splice.splice_psi_host(ev, np.zeros((0, ev.n_iso)))
    assert (defined == 0).all()

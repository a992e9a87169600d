"""What the tests of the splicing events share (tests/test_splice_events.py, test_splice_events_cpp.py, test_splice_events_gpu.py):
by_hand(), the event table restated over Python sets and dicts (no code shared with the library); psi_by_hand(), Python floats
added in the rule's order -- IEEE addition and division are correctly rounded in Python, in g++ without contraction and on gfx950,
so every comparison with it is exact and no tolerance is chosen anywhere; splice_annotation(), the sample; sample_conditions(), what
the sample must hold for the tests on it to mean something."""
import functools
import math

import numpy as np

import retained_util as R
from strawberry_amd import exonbin as eb

FIRST, LAST, INTERNAL, SKIPPED, RETAINED = 1, 2, 4, 8, 16
STRIDE = 20000
# the hand-made loci, coordinates relative to the locus' base
HAND = {
    "cassette": [[(0, 99), (200, 299), (400, 499)], [(0, 99), (400, 499)]],
    "retained": [[(0, 99), (200, 299)], [(0, 299)]],
    "altss": [[(0, 99), (200, 299)], [(0, 119), (200, 299)], [(0, 99), (180, 299)]],
    "alttss": [[(0, 99), (400, 499)], [(200, 299), (400, 499)]],
    "exon_is_intron": [[(0, 99), (200, 299), (400, 499)], [(100, 199), (400, 499)]],
    "abut": [[(0, 99), (100, 199), (400, 499)], [(0, 99), (400, 499)]],
    "dup": [[(0, 99), (200, 299)], [(0, 99), (200, 299)]],
    "single": [[(0, 99)]],
    "none": [],
}
WIDE = (8, 9, 32, 33, 40, 63, 64, 65, 300)          # isoforms, from retained_util.exon_subsets over 12 exons
SPECIAL = tuple(HAND) + tuple("W%d" % n for n in WIDE)
SEED = 27


def shifted(isos, base):
    return [[(a + base, b + base) for a, b in ex] for ex in isos]


def layout(n_small):
    """name -> locus index of the loci that are not small, spread evenly through the n_small + len(SPECIAL) loci"""
    n = n_small + len(SPECIAL)
    return {name: (k + 1) * n // (len(SPECIAL) + 1) for k, name in enumerate(SPECIAL)}


@functools.lru_cache(maxsize=4)
def splice_loci(n_small):
    """-> (loci as lists of isoforms' exon lists, name -> locus index)"""
    rng = np.random.default_rng(SEED)
    at = layout(n_small)
    where = {l: name for name, l in at.items()}
    loci = []
    for l in range(n_small + len(SPECIAL)):
        base = 10000 + STRIDE * l
        name = where.get(l)
        if name in HAND:
            loci.append(shifted(HAND[name], base))
        elif name is not None:
            ex = [(base + 400 * k, base + 400 * k + 119) for k in range(12)]
            loci.append(R.exon_subsets(rng, ex, int(name[1:]), p=0.5))
        else:
            e0, e1, e2 = (base, base + 199), (base + 500, base + 659), (base + 1000, base + 1239)
            loci.append([[e0, e1, e2], [e0, e2], [e0, e1]][:R.small_width(l, 64)])
    return loci, at


def splice_annotation(n_small):
    """-> (eb.Annotation, loci, name -> locus index): the hand-made loci by name, loci of 8 .. 300 isoforms ("W8" .. "W300") and
    n_small loci of 2 and 3 isoforms, spread between them"""
    loci, at = splice_loci(n_small)
    return eb.Annotation(loci), loci, at


def by_hand(loci):
    """-> dict of the table's arrays (as the library types them), and "span": per event the list of spanning isoforms (inside the
    locus) that psi_by_hand adds over"""
    out = {k: [] for k in ("event_locus", "event_kind", "event_left", "event_right", "event_flags", "n_span", "incl_iso", "incl_exon", "span")}
    event_off, incl_off, iso_off, iso_left, iso_right = [0], [0], [0], [], []
    g = 0
    for l, isos in enumerate(loci):
        owners, where = {}, {}
        for j, ex in enumerate(isos):
            iso_left.append(ex[0][0] if ex else 0xFFFFFFFF)
            iso_right.append(ex[-1][1] if ex else 0)
            for k, (a, b) in enumerate(ex):
                owners.setdefault((a, b, 0), []).append((j, g + k))
                pos = (FIRST if k == 0 else 0) | (LAST if k == len(ex) - 1 else 0)
                where.setdefault((a, b, 0), set()).add(pos or INTERNAL)
                if k + 1 < len(ex) and b + 1 <= ex[k + 1][0] - 1:
                    owners.setdefault((b + 1, ex[k + 1][0] - 1, 1), []).append((j, g + k))
            g += len(ex)
        exons = {(a, b) for (a, b, kind) in owners if kind == 0}
        introns = {(a, b) for (a, b, kind) in owners if kind == 1}
        for (a, b, kind) in sorted(owners):
            flags = 0
            if kind == 0:
                for bit in where[(a, b, 0)]:
                    flags |= bit
                if any(a2 <= a and b <= b2 for a2, b2 in introns):
                    flags |= SKIPPED
            elif any(a2 <= a and b <= b2 for a2, b2 in exons):
                flags |= RETAINED
            span = [j for j, ex in enumerate(isos) if ex and ex[0][0] <= a and b <= ex[-1][1]]
            own = sorted(owners[(a, b, kind)])
            assert set(j for j, _ in own) <= set(span) and len(set(j for j, _ in own)) == len(own)
            out["event_locus"].append(l), out["event_kind"].append(kind), out["event_left"].append(a), out["event_right"].append(b)
            out["event_flags"].append(flags), out["n_span"].append(len(span)), out["span"].append(span)
            out["incl_iso"] += [j for j, _ in own]
            out["incl_exon"] += [e for _, e in own]
            incl_off.append(len(out["incl_iso"]))
        event_off.append(len(out["event_kind"]))
        iso_off.append(iso_off[-1] + len(isos))
    dt = dict(event_locus=np.int32, event_kind=np.uint8, event_left=np.uint32, event_right=np.uint32, event_flags=np.uint8, n_span=np.int32,
              incl_iso=np.int32, incl_exon=np.int64)
    t = {k: np.asarray(out[k], dt[k]) for k in dt}
    t.update(event_off=np.asarray(event_off, np.int64), incl_off=np.asarray(incl_off, np.int64), iso_off=np.asarray(iso_off, np.int64),
             iso_left=np.asarray(iso_left, np.uint32), iso_right=np.asarray(iso_right, np.uint32), span=out["span"], n_exons=g)
    return t


TABLE_ARRAYS = ("event_off", "event_locus", "event_kind", "event_left", "event_right", "event_flags", "n_span", "incl_off", "incl_iso", "incl_exon",
                "iso_off", "iso_left", "iso_right")


def assert_same_table(events, want, what=""):
    """a splice.SpliceEvents against by_hand()'s dict: every array exact, dtype included"""
    assert events.n_events == want["event_kind"].size and events.n_incl == want["incl_iso"].size and events.n_exons == want["n_exons"], what
    for k in TABLE_ARRAYS:
        got = getattr(events, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.dtype, got.shape, want[k].shape)
        np.testing.assert_array_equal(got, want[k], err_msg="%s %s" % (what, k))


def psi_by_hand(want, x, keep=None):
    """want: by_hand()'s dict; x [n_rows, n_iso]; keep the same shape or None -> (psi [n_rows, n_events], defined_count [n_events])"""
    x = np.asarray(x, np.float64)
    n_rows, nu = x.shape[0], want["event_kind"].size
    psi = np.zeros((n_rows, nu))
    defined = np.zeros(nu, np.int32)
    rows = [[float(v) for v in x[k]] for k in range(n_rows)]
    kept = None if keep is None else [[int(v) != 0 for v in np.asarray(keep)[k]] for k in range(n_rows)]
    iso_off, incl_off, incl_iso, event_locus = want["iso_off"].tolist(), want["incl_off"].tolist(), want["incl_iso"].tolist(), want["event_locus"].tolist()
    for u in range(nu):
        j0 = iso_off[event_locus[u]]
        own = [j0 + j for j in incl_iso[incl_off[u]:incl_off[u + 1]]]
        span = [j0 + j for j in want["span"][u]]
        for k in range(n_rows):
            row, kp = rows[k], None if kept is None else kept[k]
            inc = 0.0
            for j in own:
                if kp is None or kp[j]:
                    inc += row[j]
            tot = 0.0
            for j in span:
                if kp is None or kp[j]:
                    tot += row[j]
            if tot > 0.0:
                psi[k, u] = inc / tot
                defined[u] += 1
            else:
                psi[k, u] = math.nan
    return psi, defined


def support_by_hand(want, exon_bases, junction_mass):
    out = np.zeros(want["event_kind"].size)
    for u in range(out.size):
        v = exon_bases if want["event_kind"][u] == 0 else junction_mass
        s = 0.0
        if v is not None:
            for e in want["incl_exon"][want["incl_off"][u]:want["incl_off"][u + 1]]:
                s += float(v[e])
        out[u] = s
    return out


def same_bits(a, b, what=""):
    """float64 arrays equal bit for bit, except that any NaN equals any NaN (psi: NaN for NaN)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb, err_msg=what + ": NaN for NaN")
    np.testing.assert_array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64), err_msg=what)


def random_rows(n_rows, n_iso, seed, keep=True):
    """non-negative x [n_rows, n_iso] with exact zeros among them, and keep of 0 / 1 / 2 (or None)"""
    rng = np.random.default_rng(seed)
    x = rng.gamma(0.7, 40.0, size=(n_rows, n_iso)) * (rng.random((n_rows, n_iso)) > 0.15)
    k = rng.choice(np.array([0, 1, 2], np.int32), size=(n_rows, n_iso), p=[0.3, 0.5, 0.2]) if keep else None
    return np.ascontiguousarray(x), k


def sample_conditions(want, keep, defined, n_rows):
    """want: by_hand() of the sample; keep: the test's keep; defined: psi_by_hand's defined_count under it -> the figures"""
    n_incl = np.diff(want["incl_off"])
    alt = n_incl != want["n_span"]
    assert alt.mean() >= 0.5, alt.mean()
    flags = want["event_flags"]
    for bit in (FIRST, LAST, INTERNAL, SKIPPED, RETAINED):
        assert (flags & bit).any(), bit
    keys = set(zip(want["event_locus"].tolist(), want["event_left"].tolist(), want["event_right"].tolist()))
    ties = want["event_kind"].size - len(keys)
    assert ties >= 1
    niso = np.diff(want["iso_off"])[want["event_locus"]]
    assert (want["n_span"] < niso).any() and (n_incl <= want["n_span"]).all()
    assert (defined < n_rows).any() and (defined > 0).any()
    return dict(events=int(alt.size), alternative=float(alt.mean()), ties=int(ties), undefined=int((defined < n_rows).sum()))

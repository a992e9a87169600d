"""Fragment assignment on the host: sbgpu_fragment_assign_host (csrc/assign_host.cpp), the CPU statement of what the device
form computes, against a per-hit restatement written out here -- Python floats, every sum in ascending order, no numpy
reductions -- that follows include/sbgpu.h's definitions (theta_j * (F / c_j)), not the library's order of the
multiplications.

No GPU here: the hits' compat / key words and the bin weights come from the oracle's restatement, as in
tests/test_context_table.py, whose toy inputs and hand-made loci are reused."""
import ctypes as C

import numpy as np
import pytest

from strawberry_amd import _lib, assign
from strawberry_amd import exonbin as eb
from test_context_table import NINE, Handle, toy_inputs

EPS = 2.0 ** -52
ROW_EPS = 1e-5
# the toy directories as the issue's restatement found them on the CPU
MOST_CANDIDATES = 4
UNIQUE_HITS = (736, 2224)
HITS = (2399, 5395)


def by_hand(bins, hit_locus, compat, F, theta, keep=None, status=None, mass=None):
    """The rule of include/sbgpu.h, hit by hit.  -> dict of lists, and per hit the posterior of every candidate."""
    nl, n_iso, nh = bins.n_loci, int(bins.iso_off[-1]), len(hit_locus)
    kept, live, scale = [False] * n_iso, [False] * bins.n_bins, [0.0] * n_iso
    for l in range(nl):
        i0, i1, b0, b1, f0 = int(bins.iso_off[l]), int(bins.iso_off[l + 1]), int(bins.row_off[l]), int(bins.row_off[l + 1]), int(bins.f_off[l])
        niso = i1 - i0
        started = status is None or int(status[l]) != _lib.EM_INIT_EMPTY
        for j in range(niso):
            kept[i0 + j] = started and (keep is None or int(keep[i0 + j]) != 0)
        for b in range(b1 - b0):
            live[b0 + b] = any(float(F[f0 + b * niso + j]) > ROW_EPS for j in range(niso))
        for j in range(niso):
            c = 0.0
            for b in range(b1 - b0):
                if live[b0 + b]:
                    c += float(F[f0 + b * niso + j])
            scale[i0 + j] = c
    out = {"map_iso": [-1] * nh, "map_prob": [0.0] * nh, "n_cand": [0] * nh, "unique_mass": [0.0] * n_iso, "map_mass": [0.0] * n_iso,
           "post_mass": [0.0] * n_iso, "unassigned": [0] * nl}
    posterior = [None] * nh
    for h in range(nh):
        l = int(hit_locus[h])
        i0, niso, f0 = int(bins.iso_off[l]), int(bins.iso_off[l + 1] - bins.iso_off[l]), int(bins.f_off[l])
        cand = [j for j in range(niso) if (int(compat[h][j >> 5]) >> (j & 31)) & 1 and kept[i0 + j]]
        out["n_cand"][h] = len(cand)
        b = int(bins.hit_bin[h])
        num, den = {}, 0.0
        if b >= 0 and live[b]:
            for j in cand:
                c = scale[i0 + j]
                w = float(F[f0 + (b - int(bins.row_off[l])) * niso + j]) / c if c != 0.0 else 0.0
                num[j] = float(theta[i0 + j]) * w
                den += num[j]
        if not (b >= 0 and live[b] and cand and den > 0.0):
            out["unassigned"][l] += 1
            continue
        best = cand[0]
        for j in cand[1:]:
            if num[j] > num[best]:
                best = j
        m = 1.0 if mass is None else float(mass[h])
        out["map_iso"][h], out["map_prob"][h] = best, num[best] / den
        out["map_mass"][i0 + best] += m
        if len(cand) == 1:
            out["unique_mass"][i0 + best] += m
        posterior[h] = {j: num[j] / den for j in cand}
        for j in cand:
            out["post_mass"][i0 + j] += m * posterior[h][j]
    return out, posterior


def check(t, want, bins, hit_locus, unit_masses, keep=None, mass=None):
    """The library's arrays against the restatement's, under the issue's bounds; then the invariants."""
    nl = bins.n_loci
    hits_of = np.bincount(np.asarray(hit_locus, np.int64), minlength=nl) if len(hit_locus) else np.zeros(nl, np.int64)
    assert t.map_iso.tolist() == want["map_iso"] and t.n_cand.tolist() == want["n_cand"] and t.unassigned.tolist() == want["unassigned"]
    for l in range(nl):
        i0, i1 = int(bins.iso_off[l]), int(bins.iso_off[l + 1])
        bound = (i1 - i0 + int(hits_of[l]) + 8) * EPS
        for h in np.nonzero(np.asarray(hit_locus) == l)[0]:
            assert abs(t.map_prob[h] - want["map_prob"][h]) <= bound * want["map_prob"][h], (l, h, t.map_prob[h], want["map_prob"][h])
        for i in range(i0, i1):
            assert abs(t.post_mass[i] - want["post_mass"][i]) <= bound * want["post_mass"][i], (l, i, t.post_mass[i], want["post_mass"][i])
            for k in ("unique_mass", "map_mass"):
                got, w = float(getattr(t, k)[i]), want[k][i]
                assert got == w if unit_masses else abs(got - w) <= bound * w, (k, l, i, got, w)
        # invariants: the posterior mass is the assigned hits' mass; the unique hits are among the MAP hits; an erased isoform holds nothing
        assigned = 0.0
        for h in np.nonzero(np.asarray(hit_locus) == l)[0]:
            if t.map_iso[h] >= 0:
                assigned += 1.0 if mass is None else float(mass[h])
                assert keep is None or keep[i0 + t.map_iso[h]] != 0
                assert 0.0 < t.map_prob[h] <= 1.0 + bound
            else:
                assert t.map_prob[h] == 0.0
        total = 0.0
        for i in range(i0, i1):
            total += float(t.post_mass[i])
            assert t.unique_mass[i] <= t.map_mass[i]
            if keep is not None and keep[i] == 0:
                assert t.unique_mass[i] == t.map_mass[i] == t.post_mass[i] == 0.0
        assert abs(total - assigned) <= bound * assigned, (l, total, assigned)
        assert int(t.unassigned[l]) == int(hits_of[l]) - sum(1 for h in np.nonzero(np.asarray(hit_locus) == l)[0] if t.map_iso[h] >= 0)


@pytest.mark.parametrize("which", NINE)
def test_host_form_on_the_toy_directories(oracle, which):
    d, ordered, rows, annot, hits, names, compat, key, bins, F, status, ab = toy_inputs(oracle, which)
    theta, _, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    unit = which != "E2E_MASS"
    assert unit == bool((hits.mass == 1.0).all())
    with Handle(annot, hits, compat, key) as H:
        t = assign.fragment_assign_host(H.h, compat, theta, F=F, keep=ab["keep"], status=status, hit_mass=hits.mass)
        t_unit = assign.fragment_assign_host(H.h, compat, theta, F=F, keep=ab["keep"], status=status)
    want, posterior = by_hand(bins, hits.hit_locus, compat, F, theta, ab["keep"], status, hits.mass)
    check(t, want, bins, hits.hit_locus, unit, keep=ab["keep"], mass=hits.mass)
    check(t_unit, by_hand(bins, hits.hit_locus, compat, F, theta, ab["keep"], status)[0], bins, hits.hit_locus, True, keep=ab["keep"])
    # what the directories hold, so that the cases above mean something
    assert HITS[0] <= hits.n_hits <= HITS[1]
    assert UNIQUE_HITS[0] <= sum(1 for h in range(hits.n_hits) if want["n_cand"][h] == 1) <= UNIQUE_HITS[1]
    assert max(want["n_cand"]) <= MOST_CANDIDATES
    assert (bins.hit_bin >= 0).all()                                       # no hit without a bin ...
    assert all(any(float(x) > ROW_EPS for x in F[bins.f_off[l] + b * n:bins.f_off[l] + (b + 1) * n])     # ... and no dead bin:
               for l in range(bins.n_loci) for n in [int(bins.iso_off[l + 1] - bins.iso_off[l])]
               for b in range(int(bins.row_off[l + 1] - bins.row_off[l])))                                # the hand-made loci below
    for h in range(hits.n_hits):                                           # no MAP decision rests on a rounding
        if posterior[h] is not None and len(posterior[h]) > 1:
            top = sorted(posterior[h].values())[-2:]
            assert top[1] - top[0] >= 0.03, (h, top)
    without_candidate = sum(1 for h in range(hits.n_hits) if want["n_cand"][h] == 0)
    assert without_candidate == (13 if which == "E2E_FILTER" else 0)
    if which == "E2E_FILTER":
        assert (np.asarray(ab["keep"]) == 0).sum() == 5 and sum(want["unassigned"]) == 13


def two_isoform_locus(oracle, order):
    """test_context_table.py::test_the_last_hit_of_a_bin_decides_its_columns' locus: isoform A = [1-100],[201-300], B = [1-300];
    X fits both, Y (spliced) fits A only; both overlap the same segments: ONE bin."""
    annot = eb.Annotation([[[(1, 100), (201, 300)], [(1, 300)]]])
    X = eb.hit_features([(50, 90)], [(210, 250)])
    Y = eb.hit_features([(80, 100), (201, 220)], [])
    hits = eb.Hits([0] * len(order), [{"X": X, "Y": Y}[k] for k in order])
    compat, key = oracle.exonbin_batch(annot, hits)
    assert [int(c) for c in compat[:, 0]] == [{"X": 0b11, "Y": 0b01}[k] for k in order]
    bins = eb.LocusBins(annot, hits, compat, key)
    assert bins.n_bins == 1 and bins.hit_bin.tolist() == [0] * len(order)
    return annot, hits, compat, key, bins


def test_two_hits_of_one_bin_with_different_words(oracle):
    """One live bin: c_j = F_j, W = 1, so X's posterior is theta's own split 3 : 1 and Y's is all A's -- exactly."""
    annot, hits, compat, key, bins = two_isoform_locus(oracle, "XYX")
    F, theta = np.array([0.25, 0.125]), np.array([3.0, 1.0])
    with Handle(annot, hits, compat, key) as H:
        t = assign.fragment_assign_host(H.h, compat, theta, F=F)
        t_mass = assign.fragment_assign_host(H.h, compat, theta, F=F, hit_mass=np.array([2.0, 0.5, 1.0], np.float32))
    assert t.n_cand.tolist() == [2, 1, 2] and t.map_iso.tolist() == [0, 0, 0] and t.map_prob.tolist() == [0.75, 1.0, 0.75]
    assert t.unique_mass.tolist() == [1.0, 0.0] and t.map_mass.tolist() == [3.0, 0.0] and t.post_mass.tolist() == [2.5, 0.5]
    assert t.unassigned.tolist() == [0] and t.n_hits == 3
    assert t_mass.unique_mass.tolist() == [0.5, 0.0] and t_mass.map_mass.tolist() == [3.5, 0.0] and t_mass.post_mass.tolist() == [2.75, 0.75]
    check(t, by_hand(bins, hits.hit_locus, compat, F, theta)[0], bins, hits.hit_locus, True)


def test_zero_theta_and_the_exact_tie(oracle):
    annot, hits, compat, key, bins = two_isoform_locus(oracle, "XY")
    with Handle(annot, hits, compat, key) as H:
        # theta_A = 0: never the MAP; Y, whose only candidate it is, has a zero denominator
        t = assign.fragment_assign_host(H.h, compat, np.array([0.0, 5.0]), F=np.array([0.25, 0.125]))
        assert t.map_iso.tolist() == [1, -1] and t.map_prob.tolist() == [1.0, 0.0] and t.n_cand.tolist() == [2, 1]
        assert t.unassigned.tolist() == [1] and t.post_mass.tolist() == [0.0, 1.0] and t.unique_mass.tolist() == [0.0, 0.0]
        # two identical columns under equal theta: the lower index
        tie = assign.fragment_assign_host(H.h, compat, np.array([2.0, 2.0]), F=np.array([0.25, 0.25]))
        assert tie.map_iso.tolist() == [0, 0] and tie.map_prob.tolist() == [0.5, 1.0] and tie.post_mass.tolist() == [1.5, 0.5]
        # ... and the higher index when it is strictly ahead
        ahead = assign.fragment_assign_host(H.h, compat, np.array([2.0, 2.5]), F=np.array([0.25, 0.25]))
        assert ahead.map_iso.tolist() == [1, 0]
        # the same with A erased by the caller's filter: X is B's alone, Y has no candidate
        erased = assign.fragment_assign_host(H.h, compat, np.array([3.0, 1.0]), F=np.array([0.25, 0.125]), keep=np.array([0, 1], np.int32))
        assert erased.n_cand.tolist() == [1, 0] and erased.map_iso.tolist() == [1, -1] and erased.unique_mass.tolist() == [0.0, 1.0]
        only = assign.fragment_assign_host(H.h, compat, np.array([3.0, 1.0]), F=np.array([0.25, 0.125]), want=("map_iso", "unassigned"))
        assert only.map_prob is None and only.post_mass is None and only.map_iso.tolist() == [0, 0] and only.unassigned.tolist() == [0]


def three_loci(oracle, with_a_hit_in_no_bin=True):
    """test_context_table.py::test_the_expression_filter_drops_bins_and_loci's loci: isoforms A = [1-100],[201-300] and
    C = [1-100],[401-500], three times.  Per locus: two hits of A only (bin 0), one of C only (bin 1), one of both (bin 2);
    locus 1 also holds a hit inside both isoforms' intron: compatible with neither, so in no bin."""
    iso = [[(1, 100), (201, 300)], [(1, 100), (401, 500)]]
    shift = lambda ex, d: [(a + d, b + d) for a, b in ex]  # noqa: E731
    annot = eb.Annotation([[shift(e, 10000 * l) for e in iso] for l in range(3)])
    feats, loc = [], []
    for l in range(3):
        d = 10000 * l
        feats += [eb.hit_features([(d + 220, d + 260)], []), eb.hit_features([(d + 230, d + 270)], []), eb.hit_features([(d + 420, d + 460)], [])]
        if l == 1 and with_a_hit_in_no_bin:
            feats.append(eb.hit_features([(d + 120, d + 160)], []))
        feats.append(eb.hit_features([(d + 10, d + 50)], []))
        loc += [l] * (len(feats) - len(loc))
    hits = eb.Hits(loc, feats)
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    assert np.diff(bins.row_off).tolist() == [3, 3, 3]
    return annot, hits, compat, key, bins


def test_dead_bins_hits_without_a_bin_and_loci_that_never_started(oracle):
    annot, hits, compat, key, bins = three_loci(oracle)
    assert compat[:, 0].tolist() == [1, 1, 2, 3, 1, 1, 2, 0, 3, 1, 1, 2, 3] and bins.hit_bin.tolist() == [0, 0, 1, 2, 3, 3, 4, -1, 5, 6, 6, 7, 8]
    # locus 0: bin 1 (the C-only hit's) is dead -- both weights <= 1e-5 -- and does not enter C's column sum either
    # locus 1: all alive; locus 2: alive, but its EM never started
    F = np.array([0.5, 0.0, 0.0, 1e-5, 0.25, 0.25] + [0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 2)
    theta = np.array([6.0, 1.0, 6.0, 1.0, 6.0, 1.0])
    status = np.array([0, 0, _lib.EM_INIT_EMPTY], np.int32)
    with Handle(annot, hits, compat, key) as H:
        t = assign.fragment_assign_host(H.h, compat, theta, F=F, status=status)
    assert t.n_cand.tolist() == [1, 1, 1, 2, 1, 1, 1, 0, 2, 0, 0, 0, 0]
    assert t.map_iso.tolist() == [0, 0, -1, 0, 0, 0, 1, -1, 0, -1, -1, -1, -1]
    assert t.unassigned.tolist() == [1, 1, 4]
    # locus 0: c_A = 0.75, c_C = 0.25 (without the dead bin's 1e-5): the hit of both has 6 (1/3) : 1 (1) = 2 : 1
    assert abs(t.map_prob[3] - 2.0 / 3.0) <= 4 * EPS and t.map_prob[:3].tolist() == [1.0, 1.0, 0.0]
    # locus 1: c_A = c_C = 0.75: 6 (1/3) : 1 (1/3) = 6 : 1
    assert abs(t.map_prob[8] - 6.0 / 7.0) <= 4 * EPS and t.map_prob[7] == 0.0
    assert t.unique_mass.tolist() == [2.0, 0.0, 2.0, 1.0, 0.0, 0.0] and t.map_mass.tolist() == [3.0, 0.0, 3.0, 1.0, 0.0, 0.0]
    check(t, by_hand(bins, hits.hit_locus, compat, F, theta, None, status)[0], bins, hits.hit_locus, True)


def test_a_hit_without_a_bin_needs_the_hits_grouped_by_locus(oracle):
    """The handle knows a binless hit's locus from the hits' grouping alone: hits that come in another order are served as long
    as every one of them has a bin, and refused with the reason otherwise."""
    annot, hits, compat, key, bins = three_loci(oracle)
    order = np.array([4, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12])      # locus 1's first hit in front of locus 0's
    F = np.array([0.5, 0.0, 0.0, 0.5, 0.25, 0.25] * 3)
    theta = np.array([6.0, 1.0] * 3)

    def shuffled(sel):
        feats = [([int(c) for c in hits.feat_code[hits.feat_off[h]:hits.feat_off[h + 1]]], [int(x) for x in hits.feat_left[hits.feat_off[h]:hits.feat_off[h + 1]]],
                  [int(x) for x in hits.feat_right[hits.feat_off[h]:hits.feat_off[h + 1]]]) for h in sel]
        return eb.Hits([int(hits.hit_locus[h]) for h in sel], feats)
    with Handle(annot, shuffled(order), compat[order], key[order]) as H:
        with pytest.raises(_lib.SbgpuError, match="did not come grouped by locus"):
            assign.fragment_assign_host(H.h, compat[order], theta, F=F)
    binned = order[order != 7]
    sh = shuffled(binned)
    with Handle(annot, sh, compat[binned], key[binned]) as H:
        t = assign.fragment_assign_host(H.h, compat[binned], theta, F=F)
    sb = eb.LocusBins(annot, sh, compat[binned], key[binned])
    check(t, by_hand(sb, sh.hit_locus, compat[binned], F, theta)[0], sb, sh.hit_locus, True)
    assert t.unassigned.tolist() == [0, 0, 0] and (t.map_iso >= 0).all()


def test_host_form_reports_what_is_missing(oracle):
    annot, hits, compat, key, bins = two_isoform_locus(oracle, "XY")
    L = _lib.load()
    F, theta = np.array([0.25, 0.125]), np.array([3.0, 1.0])
    s = _lib.sbgpu_fragment_assign_t()
    with Handle(annot, hits, compat, key) as H:
        rc = L.sbgpu_fragment_assign_host(H.h, compat.ctypes.data, 1, F.ctypes.data, None, None, None, None, C.byref(s))
        assert rc == _lib.SBGPU_EINVAL and "theta is needed" in L.sbgpu_last_error().decode()
        assert L.sbgpu_fragment_assign_host(None, compat.ctypes.data, 1, F.ctypes.data, theta.ctypes.data, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        with pytest.raises(_lib.SbgpuError, match="holds no weights"):
            assign.fragment_assign_host(H.h, compat, theta)
        # per-hit arrays of another length than the handle's hits: refused before anything is written
        short = np.full(1, 7, np.int32)
        s.map_iso, s.n_hits = short.ctypes.data, 1
        rc = L.sbgpu_fragment_assign_host(H.h, compat.ctypes.data, 1, F.ctypes.data, theta.ctypes.data, None, None, None, C.byref(s))
        assert rc == _lib.SBGPU_EINVAL and "n_hits" in L.sbgpu_last_error().decode() and short.tolist() == [7]
    # a handle that holds no hit -> bin
    none, a, h = _lib.sbgpu_hits_t(), annot._struct(), C.c_void_p()
    _lib.check(L.sbgpu_bins_create(C.byref(a), C.byref(none), None, 1, 1, None, None, C.byref(h)), "sbgpu_bins_create")
    try:
        with pytest.raises(_lib.SbgpuError, match="holds no hit -> bin"):
            assign.fragment_assign_host(h, np.zeros((0, 1), np.uint32), theta, F=F)
    finally:
        L.sbgpu_bins_destroy(h)

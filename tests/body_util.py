"""What the tests of the transcript-body coverage profile share (sbgpu_body_profile_*): the independent restatement
of include/sbgpu.h's rule, the sample, the bounds and the comparisons.

by_hand() is written from the header's text with Python floats, Python ints and ascending loops.  The posterior is
coverage_util.posteriors' theta_j * (F / c_j), not the library's order of the multiplications.  A base's bin is t * P // L on
Python ints: base by base over every S_MATCH base (per_base=True: the toys and the hand-made loci), or -- elsewhere -- from the
closed form of an interval's overlap with bin q, [ceil(q L / P), ceil((q + 1) L / P) - 1], also on Python ints; every feature is
held against every exon (no merge walk, no running bin).  It shares no code with the library.

The bounds (every term is non-negative, so the rounding of a sum of T terms is at most T * 2^-52 relative in any order):
  body_bases   two forms of the library add the same products, bit for bit, in another order: T <= the locus' hits, and the
               device flush adds a few: (hits + 8) * 2^-52.  Against by_hand(), whose posterior is formed differently:
               (2 hits + niso + 16) * 2^-52, what exon_bases is held to against its restatement.
  body_total   a further ascending sum of P such entries: + P * 2^-52.
  class_profile  a term bases_p / total carries its bin's bound, its total's and one rounding; the sum over the class' class_n
               isoforms (+ the device's flush) adds (class_n + 8) * 2^-52: the largest term bound of the class + that.
  body_center  numerator: P products of a bin and an exact small integer (one rounding each), summed: the bins' bound + (P + 1);
               denominator: the total's bound + 1; the quotient 1: bins' + total's + (P + 4) * 2^-52.  Always far below the value.
  body_cv      first order through sqrt(V) / m: with b1 = the bins' bound + (P + 3) * 2^-52 (a depth is a bin over an exact
               width; m a sum of at most P of them over their count), a deviation d_p = depth_p - m is off by at most
               (depth_p + m) * b1, so V = mean d_p^2 by dV = mean(2 |d_p| (depth_p + m)) * b1 + (P + 3) * 2^-52 * V, and
               cv by cv * (dV / (2 V) + b1 + 2 * 2^-52).  Where that exceeds a quarter of the value -- a nearly uniform profile,
               where V is the difference of nearly equal numbers -- the entry is not compared (and where V is 0 on both sides
               it is compared exactly).
Zeros, -1.0 and class_n are compared exactly."""
import functools
import math

import numpy as np

import coverage_util as CU
import retained_util as R
from strawberry_amd import body
from strawberry_amd import exonbin as eb

EPS = 2.0 ** -52
MATCH = 0
NAMES = body.NAMES
EDGES = (1000, 2000, 4000)
TAIL = 3                # loci body_sample() appends


def by_hand(bins, annot, hits, compat, F, theta, keep=None, status=None, mass=None, strand=None, n_pos=20, per_base=False):
    """-> dict: the six arrays (body_bases as [n_iso][P] lists) and what the tests ask of a sample:
    length [n_iso], multi [n_hits] (assigned with several candidates), assigned [n_hits], pairs / pairs_several_bins: the
    (hit, candidate) pairs with a base inside the candidate, and those of them that touch more than one bin."""
    posterior = CU.posteriors(bins, hits.hit_locus, compat, F, theta, keep, status)
    P = int(n_pos)
    n_iso, nh = int(annot.iso_off[-1]), hits.n_hits
    iso_off, exon_off = [int(x) for x in annot.iso_off], [int(x) for x in annot.exon_off]
    xl, xr = [int(x) for x in annot.exon_left], [int(x) for x in annot.exon_right]
    foff, code = [int(x) for x in hits.feat_off], [int(x) for x in hits.feat_code]
    fl, fr = [int(x) for x in hits.feat_left], [int(x) for x in hits.feat_right]
    locus = [int(x) for x in hits.hit_locus]
    length = [sum(xr[e] - xl[e] + 1 for e in range(exon_off[i], exon_off[i + 1])) for i in range(n_iso)]
    bases = [[0.0] * P for _ in range(n_iso)]
    assigned, multi = [False] * nh, [False] * nh
    pairs = several = 0
    for h in range(nh):
        if posterior[h] is None:
            continue
        assigned[h], multi[h] = True, len(posterior[h]) > 1
        m = 1.0 if mass is None else float(mass[h])
        feats = [(fl[q], fr[q]) for q in range(foff[h], foff[h + 1]) if code[q] == MATCH]
        for j in sorted(posterior[h]):
            w = m * posterior[h][j]
            i = iso_off[locus[h]] + j
            L = length[i]
            n = {}
            pre = 0
            for e in range(exon_off[i], exon_off[i + 1]):
                for a, b in feats:
                    lo, hi = max(a, xl[e]), min(b, xr[e])
                    if hi < lo:
                        continue
                    t0, t1 = pre + lo - xl[e], pre + hi - xl[e]
                    if per_base:
                        for t in range(t0, t1 + 1):
                            q = t * P // L
                            n[q] = n.get(q, 0) + 1
                        continue
                    for q in range(t0 * P // L, t1 * P // L + 1):
                        first, last = -(-q * L // P), -(-(q + 1) * L // P) - 1
                        k = min(t1, last) - max(t0, first) + 1
                        if k > 0:
                            n[q] = n.get(q, 0) + k
                pre += xr[e] - xl[e] + 1
            if n:
                pairs += 1
                several += len(n) > 1
            s = 0 if strand is None else int(strand[i])
            for q in sorted(n):
                bases[i][P - 1 - q if s == 2 else q] += w * float(n[q])
    total, center, cv = [0.0] * n_iso, [-1.0] * n_iso, [-1.0] * n_iso
    profile, class_n = [[0.0] * P for _ in range(4)], [0] * 4
    for i in range(n_iso):
        total[i], center[i], cv[i] = iso_stats(bases[i], length[i], 0 if strand is None else int(strand[i]))
        if total[i] == 0.0:
            continue
        k = sum(length[i] >= e for e in EDGES)
        for p in range(P):
            profile[k][p] += bases[i][p] / total[i]
        class_n[k] += 1
    return dict(body_bases=bases, body_total=total, body_center=center, body_cv=cv, class_profile=profile, class_n=class_n, length=length,
                assigned=assigned, multi=multi, pairs=pairs, pairs_several_bins=several)


def iso_stats(row, L, s):
    """(total, center, cv) of one isoform from its P bins in reported order, as include/sbgpu.h words them: Python floats, one
    operation after the other, ascending p.  Applied to a form's OWN bins it gives that form's bits."""
    P = len(row)
    row = [float(x) for x in row]
    t = 0.0
    for p in range(P):
        t += row[p]
    if t == 0.0:
        return 0.0, -1.0, -1.0
    c = 0.0
    for p in range(P):
        c += row[p] * float(2 * p + 1)
    depth = []
    for p in range(P):
        q = P - 1 - p if s == 2 else p
        wd = -(-(q + 1) * L // P) - -(-q * L // P)
        if wd:
            depth.append(row[p] / float(wd))
    mean = 0.0
    for d in depth:
        mean += d
    mean /= float(len(depth))
    v = 0.0
    for d in depth:
        v += (d - mean) * (d - mean)
    return t, c / (float(2 * P) * t), math.sqrt(v / float(len(depth))) / mean


def stats_of_own_bins(t, annot, strand, what):
    """body_total, body_center and body_cv of BodyProfile t are the rule's functions of t's OWN body_bases, bit for bit"""
    length = body.iso_lengths(annot)
    own = np.array([iso_stats(t.body_bases[i], int(length[i]), 0 if strand is None else int(strand[i])) for i in range(t.body_bases.shape[0])]).reshape(-1, 3)
    for k, name in enumerate(("body_total", "body_center", "body_cv")):
        np.testing.assert_array_equal(getattr(t, name).view(np.uint64), np.ascontiguousarray(own[:, k]).view(np.uint64), err_msg="%s %s" % (what, name))


def strands_of(annot):
    """iso_strand for a sample that has none of its own: by locus, 0 / 1 / 2 in turns (all of a locus' isoforms on one strand)"""
    return np.repeat(np.arange(annot.n_loci) % 3, np.diff(annot.iso_off)).astype(np.uint8)


@functools.lru_cache(maxsize=2)
def body_sample(n_small, grid=2048, oracle=None):
    """retained_util.edge_sample(n_small) -- whose longest isoform has 2400 bases -- and TAIL loci behind it whose isoforms reach
    beyond 4000 bases, so that all four length classes hold expressed isoforms.  edge_layout(n_small) stays what it was.
    -> (Annotation, Hits)"""
    annot, hits = R.edge_sample(n_small, grid=grid, oracle=oracle)
    rng = np.random.default_rng(R.SEED + 2)
    loci, locus_of, feats = [], [], []
    for k in range(TAIL):
        base = 10000 + R.STRIDE * (annot.n_loci + k)
        ex = [(base + 900 * e, base + 900 * e + 599) for e in range(8 + k)]                # 4800, 5400, 6000 bases
        isos = [ex, ex[:2] + ex[3:], ex[:1] + ex[5:]]
        own = set()
        for lb, rb in R.sampled_pairs(rng, isos, 120):
            f = eb.hit_features(list(lb), list(rb))
            if f is not None:
                own.add((f[1][0], f[2][-1], tuple(map(tuple, f))))
        loci.append(isos)
        for key in sorted(own):
            locus_of.append(annot.n_loci + k)
            feats.append(key[2])
    tail = eb.Hits(locus_of, feats)
    tail.mass = np.ascontiguousarray(R.MASSES[rng.integers(0, R.MASSES.size, tail.n_hits)])
    both = eb.Hits.from_arrays(np.concatenate([hits.hit_locus, tail.hit_locus]), np.concatenate([hits.feat_off, tail.feat_off[1:] + hits.feat_off[-1]]),
                               np.concatenate([hits.feat_code, tail.feat_code]), np.concatenate([hits.feat_left, tail.feat_left]),
                               np.concatenate([hits.feat_right, tail.feat_right]), np.concatenate([hits.mass, tail.mass]))
    return eb.Annotation.concat([annot, eb.Annotation(loci)]), both


def sample_conditions(annot, want, strand, n_pos):
    """What a sample must hold for the profile tests on it to mean something.  -> the figures"""
    assigned, multi = np.asarray(want["assigned"], bool), np.asarray(want["multi"], bool)
    fig = dict(assigned=int(assigned.sum()), multi=float((assigned & multi).sum() / max(int(assigned.sum()), 1)),
               several_bins=want["pairs_several_bins"] / max(want["pairs"], 1), class_n=list(want["class_n"]), n_pos=n_pos)
    assert fig["assigned"] > 0 and fig["multi"] >= 0.25, fig
    if n_pos == 20:
        assert fig["several_bins"] >= 0.20, fig
    expressed = np.asarray(want["body_total"]) > 0.0
    s = np.asarray(strand)
    fig["expressed_by_strand"] = [int((expressed & (s == k)).sum()) for k in range(3)]
    assert fig["expressed_by_strand"][1] > 0 and fig["expressed_by_strand"][2] > 0, fig
    assert all(n > 0 for n in want["class_n"]), fig
    return fig


def shape(annot, hit_locus):
    nl = annot.n_loci
    hits_of = np.bincount(np.asarray(hit_locus, np.int64), minlength=nl) if len(hit_locus) else np.zeros(nl, np.int64)
    niso = np.diff(np.asarray(annot.iso_off, np.int64))
    return hits_of, niso, np.repeat(np.arange(nl), niso)


def bins_bound(annot, hit_locus, against_by_hand):
    """[n_iso]: the relative bound of an isoform's bins"""
    hits_of, niso, iso_locus = shape(annot, hit_locus)
    per_locus = (2.0 * hits_of + niso + 16.0) * EPS if against_by_hand else (hits_of + 8.0) * EPS
    return per_locus[iso_locus]


def as_arrays(x, n_pos):
    """an object with the six arrays, or by_hand()'s dict -> dict of numpy arrays"""
    get = (lambda k: x[k]) if isinstance(x, dict) else (lambda k: getattr(x, k))
    out = {k: np.asarray(get(k), np.int64 if k == "class_n" else np.float64) for k in NAMES}
    out["body_bases"], out["class_profile"] = out["body_bases"].reshape(-1, n_pos), out["class_profile"].reshape(4, n_pos)
    return out


def within(g, w, bound, what):
    """every entry of g within bound * w of w, zeros exactly -> the worst share of the bound"""
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert (g >= 0.0).all() and (w >= 0.0).all(), what
    np.testing.assert_array_equal(g[w == 0.0], 0.0, err_msg="%s: zeros are exact" % what)
    err = np.abs(g - w)
    share = err / np.where(w > 0.0, bound * w, 1.0)
    worst = float(share.max(initial=0.0))
    print("%s: worst share of its bound %.3f" % (what, worst))
    assert (err <= bound * w).all(), (what, int(np.argmax(share)), worst)
    return worst


def compare(got, want, annot, hit_locus, against_by_hand, what, n_pos, strand=None, loci=None, classes=True):
    """got: a BodyProfile; want: another, or by_hand()'s dict.  Every entry within its bound (this file's head), zeros, -1.0 and
    class_n exactly.  loci: bool [n_loci], the loci to compare (the classes are the whole sample's: compared only without it).
    -> name -> the worst share of its bound"""
    P = n_pos
    g, w = as_arrays(got, P), as_arrays(want, P)
    _, _, iso_locus = shape(annot, hit_locus)
    pick = np.ones(iso_locus.size, bool) if loci is None else np.asarray(loci, bool)[iso_locus]
    b = bins_bound(annot, hit_locus, against_by_hand)
    worst = {}
    worst["body_bases"] = within(g["body_bases"][pick], w["body_bases"][pick], b[pick][:, None], what + " body_bases")
    worst["body_total"] = within(g["body_total"][pick], w["body_total"][pick], b[pick] + P * EPS, what + " body_total")
    empty = w["body_total"] == 0.0
    for k in ("body_center", "body_cv"):
        np.testing.assert_array_equal(g[k][pick & empty], -1.0, err_msg="%s %s: -1.0 where the total is 0.0" % (what, k))
        np.testing.assert_array_equal(w[k][pick & empty], -1.0, err_msg="%s %s: -1.0 where the total is 0.0" % (what, k))
    some = pick & ~empty
    worst["body_center"] = within(g["body_center"][some], w["body_center"][some], 2.0 * b[some] + (2 * P + 4) * EPS, what + " body_center")
    # body_cv: first order through sqrt(V) / m, from `want`'s own bins
    wd = body.bin_widths(body.iso_lengths(annot), P, strand)[some].astype(np.float64)
    on = wd > 0
    depth = np.divide(w["body_bases"][some], wd, out=np.zeros_like(wd), where=on)
    nz = on.sum(axis=1)
    m = depth.sum(axis=1) / nz
    d = np.where(on, depth - m[:, None], 0.0)
    V = (d * d).sum(axis=1) / nz
    b1 = b[some] + (P + 3) * EPS
    dV = (2.0 * np.abs(d) * np.where(on, depth + m[:, None], 0.0)).sum(axis=1) / nz * b1 + (P + 3) * EPS * V
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(V > 0.0, dV / (2.0 * V), np.inf) + b1 + 2 * EPS
    gcv, wcv = g["body_cv"][some], w["body_cv"][some]
    flat = (wcv == 0.0) & (gcv == 0.0)
    ok = rel <= 0.25
    worst["body_cv"] = within(gcv[ok], wcv[ok], rel[ok], what + " body_cv")
    print("%s body_cv: %d of %d compared under the bound, %d exactly 0.0 on both sides" % (what, int(ok.sum()), int(some.sum()), int(flat.sum())))
    assert (ok | flat).sum() * 2 >= some.sum(), (what, "body_cv: too few entries could be compared")
    if classes and loci is None:
        np.testing.assert_array_equal(g["class_n"], w["class_n"], err_msg=what + " class_n")
        length = body.iso_lengths(annot)
        cls = (length >= 1000).astype(int) + (length >= 2000) + (length >= 4000)
        term = 2.0 * b + (P + 1) * EPS
        for c in range(4):
            inside = (cls == c) & ~empty
            bound = (term[inside].max(initial=0.0) + (float(w["class_n"][c]) + 8.0) * EPS)
            worst["class_profile_%d" % c] = within(g["class_profile"][c], w["class_profile"][c], bound, what + " class_profile[%d]" % c)
    return worst


def bitwise(a, b, what, n_pos, names=NAMES):
    x, y = as_arrays(a, n_pos), as_arrays(b, n_pos)
    for k in names:
        if k == "class_n":
            np.testing.assert_array_equal(x[k], y[k], err_msg="%s %s" % (what, k))
        else:
            np.testing.assert_array_equal(x[k].view(np.uint64), y[k].view(np.uint64), err_msg="%s %s" % (what, k))

"""What the tests of the isoform-resolved coverage share (sbgpu_isoform_coverage_*): the independent restatement of
include/sbgpu.h's rule, the bounds, and the comparisons.

by_hand() is written from the header's text with Python floats and ascending loops: the posterior is theta_j * (F / c_j), not
the library's order of the multiplications, and every overlap is a loop over all of a hit's features against all of a
candidate's exons (no merge walk).  It shares no code with the library."""
import numpy as np

EPS = 2.0 ** -52
ROW_EPS = 1e-5          # include/sbgpu.h: SBGPU_EM_ROW_EPS
INIT_EMPTY = 1          # include/sbgpu.h: SBGPU_EM_INIT_EMPTY
MATCH, INTRON = 0, 1
NAMES = ("exon_bases", "junction_mass", "iso_bases", "unexplained_bases")


def posteriors(bins, hit_locus, compat, F, theta, keep=None, status=None):
    """The fragment assignment's rule as include/sbgpu.h words it, hit by hit -> per hit {candidate j: p(j|h)}, or None for an
    unassigned hit.  kept(j): keep[j] != 0 outside INIT_EMPTY loci; a bin is live when one of its weights exceeds ROW_EPS; c_j is
    the column's sum over the live bins in ascending order; num_j = theta_j * (F[b][j] / c_j), 0 where c_j == 0; den their sum in
    ascending j; unassigned without a bin, in a dead bin, without a candidate, or when den is not > 0."""
    nl, n_iso = bins.n_loci, int(bins.iso_off[-1])
    iso_off, row_off, f_off = [int(x) for x in bins.iso_off], [int(x) for x in bins.row_off], [int(x) for x in bins.f_off]
    Fl = [float(x) for x in F]
    kept, live, scale = [False] * n_iso, [False] * bins.n_bins, [0.0] * n_iso
    for l in range(nl):
        i0, niso, b0, nb, f0 = iso_off[l], iso_off[l + 1] - iso_off[l], row_off[l], row_off[l + 1] - row_off[l], f_off[l]
        started = status is None or int(status[l]) != INIT_EMPTY
        for j in range(niso):
            kept[i0 + j] = started and (keep is None or int(keep[i0 + j]) != 0)
        for b in range(nb):
            live[b0 + b] = any(Fl[f0 + b * niso + j] > ROW_EPS for j in range(niso))
        for j in range(niso):
            c = 0.0
            for b in range(nb):
                if live[b0 + b]:
                    c += Fl[f0 + b * niso + j]
            scale[i0 + j] = c
    out = [None] * len(hit_locus)
    for h in range(len(hit_locus)):
        l = int(hit_locus[h])
        i0, niso = iso_off[l], iso_off[l + 1] - iso_off[l]
        b = int(bins.hit_bin[h])
        if b < 0 or not live[b]:
            continue
        words = [int(x) for x in compat[h]]
        cand = [j for j in range(niso) if (words[j >> 5] >> (j & 31)) & 1 and kept[i0 + j]]
        num, den = {}, 0.0
        for j in cand:
            c = scale[i0 + j]
            num[j] = float(theta[i0 + j]) * (Fl[f_off[l] + (b - row_off[l]) * niso + j] / c if c != 0.0 else 0.0)
            den += num[j]
        if cand and den > 0.0:
            out[h] = {j: num[j] / den for j in cand}
    return out


def by_hand(bins, annot, hits, compat, F, theta, keep=None, status=None, mass=None):
    """-> dict: the four arrays as lists, and what the tests ask of a sample:
    matched [n_loci]        sum of m_h * matchlen(h) over ALL hits of the locus,
    outside [n_loci]        an assigned hit of the locus has matched bases outside a candidate's exons,
    assigned, spliced, multi  per hit: has a posterior; owns an S_INTRON feature; has several candidates,
    supporters              exon index -> the number of assigned hits that support its junction (absent: none)."""
    posterior = posteriors(bins, hits.hit_locus, compat, F, theta, keep, status)
    nl, n_iso, nh = annot.n_loci, int(annot.iso_off[-1]), hits.n_hits
    iso_off, exon_off = [int(x) for x in annot.iso_off], [int(x) for x in annot.exon_off]
    xl, xr = [int(x) for x in annot.exon_left], [int(x) for x in annot.exon_right]
    foff, code = [int(x) for x in hits.feat_off], [int(x) for x in hits.feat_code]
    fl, fr = [int(x) for x in hits.feat_left], [int(x) for x in hits.feat_right]
    locus = [int(x) for x in hits.hit_locus]
    n_exon = exon_off[n_iso]
    exon_bases, junction_mass = [0.0] * n_exon, [0.0] * n_exon
    unexplained, matched, outside = [0.0] * nl, [0.0] * nl, [False] * nl
    assigned, spliced, multi = [False] * nh, [False] * nh, [False] * nh
    supporters = {}
    for h in range(nh):
        l = locus[h]
        m = 1.0 if mass is None else float(mass[h])
        feats = [(code[q], fl[q], fr[q]) for q in range(foff[h], foff[h + 1])]
        matchlen = 0
        for c, a, b in feats:
            if c == MATCH:
                matchlen += b - a + 1
        matched[l] += m * float(matchlen)
        spliced[h] = any(c == INTRON for c, _, _ in feats)
        if posterior[h] is None:
            unexplained[l] += m * float(matchlen)
            continue
        assigned[h], multi[h] = True, len(posterior[h]) > 1
        for j in sorted(posterior[h]):
            w = m * posterior[h][j]
            i = iso_off[l] + j
            inside = 0
            for e in range(exon_off[i], exon_off[i + 1]):
                ov = 0
                for c, a, b in feats:
                    if c == MATCH:
                        ov += max(0, min(xr[e], b) - max(xl[e], a) + 1)
                exon_bases[e] += w * float(ov)
                inside += ov
                if e + 1 < exon_off[i + 1]:
                    for c, a, b in feats:
                        if c == INTRON and a == xr[e] + 1 and b == xl[e + 1] - 1:
                            junction_mass[e] += w
                            supporters[e] = supporters.get(e, 0) + 1
            if inside != matchlen:
                outside[l] = True
    iso_bases = [0.0] * n_iso
    for i in range(n_iso):
        s = 0.0
        for e in range(exon_off[i], exon_off[i + 1]):
            s += exon_bases[e]
        iso_bases[i] = s
    return dict(exon_bases=exon_bases, junction_mass=junction_mass, iso_bases=iso_bases, unexplained_bases=unexplained, matched=matched,
                outside=outside, assigned=assigned, spliced=spliced, multi=multi, supporters=supporters)


def shape(annot, hit_locus):
    """-> (hits of every locus, the locus of every isoform, the locus of every exon, exons of every isoform)"""
    nl = annot.n_loci
    iso_off, exon_off = np.asarray(annot.iso_off, np.int64), np.asarray(annot.exon_off, np.int64)
    hits_of = np.bincount(np.asarray(hit_locus, np.int64), minlength=nl) if len(hit_locus) else np.zeros(nl, np.int64)
    iso_locus = np.repeat(np.arange(nl), np.diff(iso_off))
    exons_of_iso = np.diff(exon_off)
    return hits_of, iso_locus, np.repeat(iso_locus, exons_of_iso), exons_of_iso


def bounds(annot, hit_locus, against_by_hand):
    """name -> the relative bound of every entry.
    Two forms of the library (the same terms, bit for bit, in another order): two orderings of a sum of T non-negative terms
    differ by at most T * 2^-52 relative, T <= the locus' hits, and the device flush adds a few: (hits + 8) * 2^-52; iso_bases is
    a further sum over the isoform's exons: (hits + exons of the isoform + 8) * 2^-52.
    Either form against by_hand(), whose posterior is formed differently: (2 hits + niso + 16) * 2^-52, what post_mass is held
    to against its restatement."""
    hits_of, iso_locus, exon_locus, exons_of_iso = shape(annot, hit_locus)
    niso = np.diff(np.asarray(annot.iso_off, np.int64))
    if against_by_hand:
        per_locus = (2.0 * hits_of + niso + 16.0) * EPS
        return dict(exon_bases=per_locus[exon_locus], junction_mass=per_locus[exon_locus], iso_bases=per_locus[iso_locus], unexplained_bases=per_locus)
    per_locus = (hits_of + 8.0) * EPS
    return dict(exon_bases=per_locus[exon_locus], junction_mass=per_locus[exon_locus], iso_bases=per_locus[iso_locus] + exons_of_iso * EPS,
                unexplained_bases=per_locus)


def masks(annot, loci):
    """loci: bool [n_loci] -> name -> the entries of those loci"""
    _, iso_locus, exon_locus, _ = shape(annot, [])
    return dict(exon_bases=loci[exon_locus], junction_mass=loci[exon_locus], iso_bases=loci[iso_locus], unexplained_bases=loci)


def last_exons(annot):
    """bool [n_exon]: the exon is its isoform's last"""
    exon_off = np.asarray(annot.exon_off, np.int64)
    last = np.zeros(int(exon_off[-1]), bool)
    last[exon_off[1:][np.diff(exon_off) > 0] - 1] = True
    return last


def compare(got, want, annot, hit_locus, against_by_hand, what, loci=None):
    """got: an IsoformCoverage; want: another, or by_hand()'s dict.  Every entry within its bound -- so a zero is matched exactly
    -- and the last exons' junctions exactly 0.0 on both sides.  -> name -> the worst share of its bound."""
    b = bounds(annot, hit_locus, against_by_hand)
    pick = masks(annot, np.ones(annot.n_loci, bool) if loci is None else loci)
    worst = {}
    for k in NAMES:
        g = np.asarray(getattr(got, k), np.float64)[pick[k]]
        w = np.asarray(want[k] if isinstance(want, dict) else getattr(want, k), np.float64)[pick[k]]
        bound = b[k][pick[k]]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert (g >= 0.0).all() and (w >= 0.0).all(), (what, k)
        np.testing.assert_array_equal(g[w == 0.0], 0.0, err_msg="%s %s: zeros are exact" % (what, k))
        err = np.abs(g - w)
        share = err / np.where(w > 0.0, bound * w, 1.0)
        worst[k] = float(share.max(initial=0.0))
        print("%s %s: worst share of its bound %.3f" % (what, k, worst[k]))
        assert (err <= bound * w).all(), (what, k, int(np.argmax(share)), worst[k])
    last = last_exons(annot)
    assert (np.asarray(got.junction_mass)[last] == 0.0).all(), (what, "the last exon of an isoform has no junction")
    return worst


def bitwise(a, b, what, loci=None, annot=None):
    pick = masks(annot, loci) if loci is not None else None
    for k in NAMES:
        x, y = np.asarray(getattr(a, k), np.float64), np.asarray(getattr(b, k), np.float64)
        if pick is not None:
            x, y = x[pick[k]], y[pick[k]]
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg="%s %s" % (what, k))


def iso_bases_of(exon_bases, annot):
    """the ascending sum of exon_bases over every isoform's exons, in doubles one after the other"""
    exon_off = [int(x) for x in annot.exon_off]
    x = [float(v) for v in exon_bases]
    out = np.zeros(len(exon_off) - 1)
    for i in range(len(exon_off) - 1):
        s = 0.0
        for e in range(exon_off[i], exon_off[i + 1]):
            s += x[e]
        out[i] = s
    return out


def conservation(cov, want, annot, hit_locus, what, most_left_out=0.05):
    """Per locus, sum_j iso_bases[j] + unexplained_bases[l] == sum_h m_h matchlen(h), for every locus with hits but those where
    by_hand() found an assigned hit with matched bases outside a candidate's exons (at most 5 % of them).
    The right side is by_hand()'s, so the bound is the one either form is held to against by_hand(): (2 hits + niso + 16) * 2^-52."""
    hits_of, iso_locus, exon_locus, _ = shape(annot, hit_locus)
    iso_off = np.asarray(annot.iso_off, np.int64)
    with_hits = hits_of > 0
    out = np.asarray(want["outside"], bool) & with_hits
    share = out.sum() / max(int(with_hits.sum()), 1)
    print("%s conservation: %d of %d loci with hits left out (%.2f %%)" % (what, int(out.sum()), int(with_hits.sum()), 100.0 * share))
    assert share <= most_left_out, (what, share)
    bound = (2.0 * hits_of + np.diff(iso_off) + 16.0) * EPS
    worst = 0.0
    for l in np.nonzero(with_hits & ~out)[0]:
        total = 0.0
        for i in range(int(iso_off[l]), int(iso_off[l + 1])):
            total += float(cov.iso_bases[i])
        total += float(cov.unexplained_bases[l])
        m = float(want["matched"][l])
        assert abs(total - m) <= bound[l] * m, (what, int(l), total, m)
        worst = max(worst, abs(total - m) / (bound[l] * m) if m > 0.0 else 0.0)
    print("%s conservation: worst share of its bound %.3f" % (what, worst))
    return share


def sample_conditions(annot, hits, want, nobin_locus=None):
    """What a sample must hold for the coverage tests on it to mean something.  -> the figures"""
    assigned, spliced, multi = (np.asarray(want[k], bool) for k in ("assigned", "spliced", "multi"))
    n = int(assigned.sum())
    assert n > 0
    fig = dict(assigned=n, spliced=float((assigned & spliced).sum() / n), multi=float((assigned & multi).sum() / n))
    assert fig["spliced"] >= 0.20, fig
    assert fig["multi"] >= 0.25, fig
    # annotated junctions: without support; and one intron, annotated in several isoforms of a locus, supported in several of them
    last = last_exons(annot)
    jm = np.asarray(want["junction_mass"])
    fig["junctions"] = int((~last).sum())
    fig["junctions_without_support"] = int(((jm == 0.0) & ~last).sum())
    assert fig["junctions_without_support"] >= 1, fig
    _, _, exon_locus, _ = shape(annot, [])
    seen, shared = {}, 0
    for e in np.nonzero((jm > 0.0) & ~last)[0]:
        key = (int(exon_locus[e]), int(annot.exon_right[e]), int(annot.exon_left[e + 1]))
        seen[key] = seen.get(key, 0) + 1
    shared = sum(1 for v in seen.values() if v > 1)
    fig["introns_supported_in_several_isoforms"] = shared
    assert shared >= 1, fig
    if nobin_locus is not None:
        assert want["unexplained_bases"][nobin_locus] > 0.0
    fig["loci_with_unexplained_bases"] = int((np.asarray(want["unexplained_bases"]) > 0.0).sum())
    assert fig["loci_with_unexplained_bases"] >= 1, fig
    return fig

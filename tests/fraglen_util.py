"""Pass 1 of the reference's default mode restated in numpy, and hand-built loci that drive every route of the device's
fraglen_hist_kernel (strawberry_amd/csrc/fraglen_device.h).

Sample::fragLenDist (/root/reference/src/alignments.cpp:1363-1410): every hit with features that is compatible with
EXACTLY ONE isoform of its locus contributes Contig::exonic_overlaps_len(isoform, hit.left(), hit.right())
(/root/reference/src/contig.cpp:412-426) -- the isoform's exonic bases between the hit's first left end and last right
end.  reference() does that from the compat words alone (the exon-bin kernel's, pinned bit-exact by test_exonbin_*),
with Python's and numpy's integers; it never calls sbgpu_frag_lens_host.
"""
import numpy as np

from strawberry_amd import exonbin as eb

MATCH, INTRON, GAP = eb.MATCH, eb.INTRON, eb.GAP
LDS_BINS = 8192         # kFragLenLdsBins: lengths from here on go to the global histogram
WAVE = 64
TABLE_ISO, TABLE_EXONS = 63, 64   # a locus' table fits a wave's registers up to these


def popcount32(x):
    x = np.asarray(x, np.uint64)
    x = x - ((x >> np.uint64(1)) & np.uint64(0x55555555))
    x = (x & np.uint64(0x33333333)) + ((x >> np.uint64(2)) & np.uint64(0x33333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F)
    return ((x * np.uint64(0x01010101)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)


def hit_ends(hits):
    """-> (has features, first left end, last right end) per hit (0, 0 for a hit without features)"""
    off = hits.feat_off
    has = off[1:] > off[:-1]
    left = np.zeros(hits.n_hits, np.int64)
    right = np.zeros(hits.n_hits, np.int64)
    left[has] = hits.feat_left[off[:-1][has]]
    right[has] = hits.feat_right[off[1:][has] - 1]
    return has, left, right


def unique_isoform(annot, hits, compat):
    """-> (number of compatible isoforms of the hit's locus, the one's index in the locus or -1) per hit"""
    compat = np.asarray(compat, np.uint32).reshape(hits.n_hits, -1)
    niso = np.diff(annot.iso_off)[hits.hit_locus.astype(np.int64)]
    count = np.zeros(hits.n_hits, np.int64)
    mark = np.full(hits.n_hits, -1, np.int64)
    for w in range(compat.shape[1]):
        left = niso - 32 * w
        mask = np.where(left >= 32, 0xFFFFFFFF, (np.int64(1) << np.clip(left, 0, 31)) - 1).astype(np.uint64)
        bits = compat[:, w].astype(np.uint64) & mask
        c = popcount32(bits).astype(np.int64)
        count += c
        one = c == 1
        mark[one] = 32 * w + np.log2(bits[one].astype(np.float64)).astype(np.int64)   # (powers of two: exact)
    mark[count != 1] = -1
    return count, mark


def exonic_overlaps_len(annot, iso, left, right):
    """Contig::exonic_overlaps_len for each (global isoform, left, right), int64"""
    e0 = annot.exon_off[iso]
    ne = annot.exon_off[iso + 1] - e0
    xl_all, xr_all = annot.exon_left.astype(np.int64), annot.exon_right.astype(np.int64)
    out = np.zeros(len(iso), np.int64)
    for k in range(int(ne.max(initial=0))):
        v = k < ne
        e = np.where(v, e0 + k, 0)
        xl, xr = xl_all[e], xr_all[e]
        ov = v & (xl <= right) & (left <= xr)   # GenomicFeature::overlap_len_in_genome
        out += np.where(ov, np.minimum(xr, right) - np.maximum(xl, left) + 1, 0)
    return out


def reference(annot, hits, compat):
    """-> dict(keep, mark, lens (kept hits, hit order), hist (np.bincount of lens), count)"""
    has, left, right = hit_ends(hits)
    count, mark = unique_isoform(annot, hits, compat)
    keep = has & (count == 1)
    iso = annot.iso_off[hits.hit_locus.astype(np.int64)[keep]] + mark[keep]
    lens = exonic_overlaps_len(annot, iso, left[keep], right[keep])
    return {"keep": keep, "mark": mark, "count": count, "lens": lens, "hist": np.bincount(lens) if len(lens) else np.zeros(0, np.int64)}


def law_of(hist):
    """(start_offset, histogram from there to the last non-zero entry) of a histogram indexed by length"""
    nz = np.flatnonzero(hist)
    return int(nz[0]), np.asarray(hist[nz[0]:nz[-1] + 1], np.int64)


def routes(annot, hits, ref):
    """Which of the kernel's routes the kept hits take.  The kernel gives a workgroup whole tiles of 1024 hits, so a
    wave holds the hits [64 k, 64 k + 64): it is uniform when they share one locus; a uniform wave keeps its locus'
    table in registers when the locus has <= 63 isoforms and <= 64 exon entries."""
    n = hits.n_hits
    loc = hits.hit_locus.astype(np.int64)
    starts = np.arange(0, n, WAVE)
    uniform = (np.minimum.reduceat(loc, starts) == np.maximum.reduceat(loc, starts)) if n else np.zeros(0, bool)
    uni = np.repeat(uniform, WAVE)[:n]
    niso = np.diff(annot.iso_off)
    nex = annot.exon_off[annot.iso_off[1:]] - annot.exon_off[annot.iso_off[:-1]]
    small = ((niso <= TABLE_ISO) & (nex <= TABLE_EXONS))[loc]
    k = ref["keep"]
    lens = np.zeros(n, np.int64)
    lens[k] = ref["lens"]
    mark = ref["mark"]
    return {
        "table": int((k & uni & small).sum()),
        "scalar": int((k & uni & ~small).sum()),
        "straddle": int((k & ~uni).sum()),
        "straddle_big": int((k & ~uni & ~small).sum()),
        "word_1_plus": int((k & (mark >= 32)).sum()),
        "table_last_lane": int((k & uni & small & (mark == TABLE_ISO - 1)).sum()),   # readlane(t_eoff, j + 1) at j = 62
        "global": int((k & (lens >= LDS_BINS)).sum()),
        "lds": int((k & (lens < LDS_BINS)).sum()),
        "zero_compat": int((ref["count"] == 0).sum()),
        "multi_compat": int((ref["count"] >= 2).sum()),
        "no_features": int((hits.feat_off[1:] == hits.feat_off[:-1]).sum()),
        # (isoforms of the locus, the unique isoform's index) of the kept hits
        "marks": set(zip(niso[loc[k]].tolist(), mark[k].tolist())),
    }


# ---- hand-built loci ------------------------------------------------------------------------------------------------------

def isoform(start, n_exons, exon_len, intron_len):
    step = exon_len + intron_len
    return [(start + k * step, start + k * step + exon_len - 1) for k in range(n_exons)]


def make_locus(start, shapes, gap=500):
    """Isoforms one after the other, disjoint: a hit inside one isoform's exons is compatible with it alone.
    shapes: per isoform (n_exons, exon_len, intron_len); None: an isoform without exons; "dup": a copy of the isoform
    before it (every hit of one is compatible with both).  -> (isoforms, first free position behind the locus)"""
    isos, pos = [], start
    for s in shapes:
        if s is None:
            isos.append([])
        elif s == "dup":
            isos.append(list(isos[-1]))
        else:
            isos.append(isoform(pos, *s))
            pos = isos[-1][-1][1] + 1 + gap
    return isos, pos


class HitSet:
    """Hits collected chunk by chunk: per hit its locus and features (code, left, right as CSR)."""

    def __init__(self):
        self.loc, self.nf, self.code, self.left, self.right = [], [], [], [], []

    def add(self, loc, nf, code, left, right):
        n = len(nf)
        self.loc.append(np.broadcast_to(np.asarray(loc, np.int64), (n,)).copy())
        self.nf.append(np.asarray(nf, np.int64))
        self.code.append(np.asarray(code, np.uint8))
        self.left.append(np.asarray(left, np.int64))
        self.right.append(np.asarray(right, np.int64))

    def add_blocks(self, loc, blocks):
        """one hit per entry of `blocks`: single-mate hits made of the given aligned blocks (introns between them)"""
        for b in blocks:
            c, l, r = eb.mate_features(b)
            self.add(loc, [len(c)], c, l, r)

    def add_featureless(self, loc, n):
        self.add(loc, np.zeros(n, np.int64), [], [], [])

    def add_pairs(self, rng, annot, loc, targets, n, mate=75, edge=0.25):
        """n hits inside the exons of isoforms drawn from `targets` (indices in locus `loc`): a pair of mates with a gap
        between them when its ends fall in two exons, one block when in one.  With probability `edge` an end sits on
        an exon's first or last base."""
        if n == 0:
            return
        iso = annot.iso_off[loc] + rng.choice(np.asarray(targets, np.int64), n)
        e0 = annot.exon_off[iso]
        ne = annot.exon_off[iso + 1] - e0
        assert (ne > 0).all()
        a, b = rng.integers(0, ne), rng.integers(0, ne)
        a, b = e0 + np.minimum(a, b), e0 + np.maximum(a, b)
        xl, xr = annot.exon_left.astype(np.int64), annot.exon_right.astype(np.int64)
        left = xl[a] + (rng.random(n) * (xr[a] - xl[a] + 1)).astype(np.int64)
        right = xl[b] + (rng.random(n) * (xr[b] - xl[b] + 1)).astype(np.int64)
        pick = rng.random(n)
        left = np.where(pick < edge / 2, xl[a], np.where(pick < edge, xr[a], left))
        pick = rng.random(n)
        right = np.where(pick < edge / 2, xr[b], np.where(pick < edge, xl[b], right))
        same = a == b
        lo, hi = np.where(same, np.minimum(left, right), left), np.where(same, np.maximum(left, right), right)
        m1r = np.minimum(lo + mate - 1, xr[a])
        m2l = np.maximum(hi - mate + 1, xl[b])
        nf = np.where(same, 1, 3)
        code = np.zeros((n, 3), np.uint8)
        code[:, 1] = GAP
        L = np.stack([lo, m1r + 1, m2l], 1)
        R = np.stack([m1r, m2l - 1, hi], 1)
        L[same, 0], R[same, 0] = lo[same], hi[same]
        take = np.arange(3)[None, :] < nf[:, None]
        self.add(loc, nf, code[take], L[take], R[take])

    def add_intronic(self, rng, annot, loc, n, mate=20):
        """n single-block hits inside the locus' introns (isoforms of >= 2 exons, introns longer than `mate`): compatible
        with no isoform of the locus made by make_locus"""
        lefts = []
        for j in range(annot.iso_off[loc], annot.iso_off[loc + 1]):
            e = range(annot.exon_off[j], annot.exon_off[j + 1])
            for k0, k1 in zip(e[:-1], e[1:]):
                if annot.exon_left[k1] - annot.exon_right[k0] - 1 > mate:
                    lefts.append(int(annot.exon_right[k0]) + 1)
        assert lefts
        left = rng.choice(np.asarray(lefts, np.int64), n)
        self.add(loc, np.ones(n, np.int64), np.zeros(n, np.uint8), left, left + mate - 1)

    def hits(self):
        """-> eb.Hits grouped by locus, sorted by (locus, left end, right end) inside it (HitCluster's order)"""
        loc = np.concatenate(self.loc)
        nf = np.concatenate(self.nf)
        code, left, right = (np.concatenate(x) for x in (self.code, self.left, self.right))
        off = np.concatenate([[0], np.cumsum(nf)])
        has = nf > 0
        lk = np.zeros(len(nf), np.int64)
        rk = np.zeros(len(nf), np.int64)
        lk[has], rk[has] = left[off[:-1][has]], right[off[1:][has] - 1]
        order = np.lexsort((rk, lk, loc))
        nf2 = nf[order]
        off2 = np.concatenate([[0], np.cumsum(nf2)])
        src = np.repeat(off[:-1][order] - off2[:-1], nf2) + np.arange(off2[-1])
        return eb.Hits.from_arrays(loc[order], off2, code[src], left[src], right[src])

"""One sample for the two stages that read what a resident call keeps -- the `-f` table (csrc/context_device.h) and the fragment
assignment (csrc/assign_device.h) -- at the shapes where their kernels take another path: more loci and more work items than
twice the grid, more loci than two rounds of the row scan, split loci of several isoforms, a locus beyond 256 isoforms, and a
locus on either side of every threshold.  tests/test_retained_edges.py checks the sample itself and the host forms on the CPU,
tests/test_retained_edges_gpu.py the device forms."""
import functools

import numpy as np

from strawberry_amd import exonbin as eb

RL = 75
MASSES = np.array([1.0, 1.0 / 2.0, 1.0 / 3.0, 1.0 / 4.0, 1.0 / 5.0], np.float32)
MIN_ISOFORM_FRAC = 0.002        # (0.05 erases all of locus C's isoforms)
LAW = (150.0, 60.0)             # fragments are drawn 151 .. 400 bases long: the long ones' bins are dead (weight <= 1e-5)
ITEM_HITS = 16384               # csrc/assign_device.h: kAsgItemHits, csrc/context_device.h: kCtxItemHits
SCAN_ROUND = 4096               # loci per round of ctx_scan_kernel
GRID_PER_CU = 8                 # both stages' grids are capped at 8 x CU count
RUN_CAP = 48                    # csrc/bins_device.h: kBinsRunCap -- fragments of one bin that start at one position (fractional masses)
STRIDE = 20000                  # bases from one locus' start to the next one's
SEED = 14                       # (a seed under which no two posteriors of a hit tie: the tests assert the gap)
# the loci that are not small, in the order they are spread through the list (so that A, B and C, and the two sides of every
# threshold, fall into different passes of a 2048-workgroup grid); EXACT_BINS: their bin counts; WIDTH: their isoforms
SPECIAL = ("T8", "T1024", "T33", "A", "T257", "C", "B", "T9", "T256", "EMPTY", "T1025", "T32", "NOBIN")
EXACT_BINS = {"T256": 256, "T257": 257, "T1024": 1024, "T1025": 1025}
WIDTH = {"A": 6, "B": 40, "C": 300, "T8": 8, "T9": 9, "T32": 32, "T33": 33, "T256": 3, "T257": 3, "T1024": 4, "T1025": 4, "EMPTY": 2, "NOBIN": 2}


def edge_layout(n_small):
    """name -> locus index of the loci that are not small; they are spread evenly through the n_small + len(SPECIAL) loci."""
    n = n_small + len(SPECIAL)
    return {name: (k + 1) * n // (len(SPECIAL) + 1) for k, name in enumerate(SPECIAL)}


def small_width(l, grid):
    """Isoforms of the small locus at position l: 2 and 3 in turns, and the turn shifts by one every `grid` loci, so that the
    loci one workgroup takes one after the other (l, l + grid, l + 2 grid) differ."""
    return 2 + ((l + l // grid) & 1)


def tx_blocks(ex, t0, t1):
    """transcript interval [t0, t1) of the isoform with exons ex -> genomic blocks"""
    out, off = [], 0
    for (a, b) in ex:
        if off >= t1:
            break
        ln = b - a + 1
        lo, hi = max(t0, off), min(t1, off + ln)
        if lo < hi:
            out.append((a + lo - off, a + hi - off - 1))
        off += ln
    return out


def exon_subsets(rng, exons, n, p=0.6):
    """n distinct isoforms over `exons` that keep the first and the last one; the first of them has every exon"""
    isos = [list(exons)]
    while len(isos) < n:
        pick = [e for k, e in enumerate(exons) if k in (0, len(exons) - 1) or rng.random() < p]
        if pick not in isos:
            isos.append(pick)
    return isos


def sampled_pairs(rng, isos, n, weights=None, fl_lo=151, fl_hi=400):
    """n draws of (isoform, fragment of fl_lo .. fl_hi bases on it): the fragment's two mates of RL bases as genomic blocks"""
    which = rng.choice(len(isos), size=n, p=weights)
    fls = rng.integers(fl_lo, fl_hi + 1, size=n)
    u = rng.random(n)
    lens = [sum(b - a + 1 for a, b in ex) for ex in isos]
    out = set()
    for k in range(n):
        ex, L = isos[which[k]], lens[which[k]]
        fl = min(int(fls[k]), L)
        st = int(u[k] * (L - fl + 1))
        rl = min(RL, fl)
        out.add((tuple(tx_blocks(ex, st, st + rl)), tuple(tx_blocks(ex, st + fl - rl, st + fl))))
    return sorted(out)


def ladder_pairs(rng, ex, n_combos, per):
    """tests/test_context_table_gpu.py::wide_sample's wide locus: reads over exons i .. i + a and j .. j + b of a ladder of short
    exons -- every (i, a, j, b) is a bin of its own -- `per` fragments of each"""
    n = len(ex)

    def mate(i, a, o1, o2):
        if a == 0:
            return ((ex[i][0] + o1, ex[i][1] - o2),)
        return ((ex[i][0] + o1, ex[i][1]),) + tuple(ex[k] for k in range(i + 1, i + a)) + ((ex[i + a][0], ex[i + a][1] - o2),)
    combos = set()
    while len(combos) < n_combos:
        i, a, gap, b = int(rng.integers(0, n - 10)), int(rng.integers(0, 3)), int(rng.integers(1, 6)), int(rng.integers(0, 3))
        if i + a + gap + b < n:
            combos.add((i, a, i + a + gap, b))
    out = set()
    for (i, a, j, b) in sorted(combos):
        for _ in range(per):
            out.add((mate(i, a, int(rng.integers(0, 12)), int(rng.integers(0, 6))), mate(j, b, int(rng.integers(0, 6)), int(rng.integers(0, 12)))))
    return sorted(out)


def build_locus(rng, name, base):
    """-> (isoforms, [(left blocks, right blocks), ...]) of one of the loci that are not small"""
    if name == "A":         # narrow and split: three work items; the sums in 32 copies, flushed by atomics
        ex = [(base + 700 * k, base + 700 * k + 399) for k in range(6)]
        isos = exon_subsets(rng, ex, 6)
        return isos, sampled_pairs(rng, isos, 37000)
    if name == "B":         # two compat words and split: one LDS copy, flushed by atomics; a quarter of its isoforms is never drawn from
        ex = [(base + 400 * k, base + 400 * k + 199) for k in range(8)]
        isos = exon_subsets(rng, ex, 40)
        w = np.where(np.arange(40) % 4 == 3, 0.0, 1.0)
        return isos, sampled_pairs(rng, isos, 19500, weights=w / w.sum())
    if name == "C":         # ten compat words; the column pass strides and reads F through the L2
        ex = [(base + 400 * k, base + 400 * k + 119) for k in range(12)]
        isos = exon_subsets(rng, ex, 300, p=0.5)
        return isos, sampled_pairs(rng, isos, 4000)
    if name in ("T8", "T9", "T32", "T33"):
        ex = [(base + 400 * k, base + 400 * k + 199) for k in range(8)]
        isos = exon_subsets(rng, ex, WIDTH[name])
        return isos, sampled_pairs(rng, isos, 700)
    if name in EXACT_BINS:  # more bins than wanted; edge_sample() drops the hits of the surplus ones
        ex = [(base + 130 * k, base + 130 * k + 29) for k in range(70)]
        skips = ((), (20,), (45,)) if WIDTH[name] == 3 else ((), (17,), (35,), (52,))
        isos = [[e for k, e in enumerate(ex) if k not in s] for s in skips]
        want = EXACT_BINS[name]
        return isos, ladder_pairs(rng, ex, want + want // 8 + 8, 6 if want < 1000 else 5)
    two = [[(base, base + 99), (base + 200, base + 299)], [(base, base + 99), (base + 400, base + 499)]]
    if name == "EMPTY":
        return two, []
    assert name == "NOBIN"  # reads inside both isoforms' first intron: compatible with neither, in no bin
    return two, [(((base + 110 + 3 * k, base + 150 + 3 * k),), ()) for k in range(6)]


def build_small(rng, niso, base, n_hits):
    # (exons of three lengths: isoforms of one length would have equal weights, and tie wherever the EM leaves theta at its start)
    e0, e1, e2 = (base, base + 199), (base + 500, base + 659), (base + 1000, base + 1239)
    isos = [[e0, e1, e2], [e0, e2], [e0, e1]][:niso]
    return isos, sampled_pairs(rng, isos, n_hits, fl_hi=350)


def select_hits(hits, idx):
    """the hits `idx` (ascending) of `hits` as Hits of their own"""
    idx = np.asarray(idx, np.int64)
    n = np.diff(hits.feat_off)[idx]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    at = np.repeat(hits.feat_off[idx] - off[:-1], n) + np.arange(off[-1])
    return eb.Hits.from_arrays(hits.hit_locus[idx], off, hits.feat_code[at], hits.feat_left[at], hits.feat_right[at], hits.mass[idx])


def bins_by_first_appearance(compat, key, lo, hi):
    """hits lo .. hi - 1 of one locus -> per hit the number of its bin (-1: compatible with nothing), bins numbered as they appear"""
    seen, out = {}, []
    for h in range(lo, hi):
        out.append(seen.setdefault(key[h].tobytes(), len(seen)) if compat[h].any() else -1)
    return np.asarray(out, np.int64)


@functools.lru_cache(maxsize=2)
def edge_sample(n_small, grid=2048, oracle=None):
    """-> (Annotation, Hits): n_small loci of 2 and 3 isoforms with 12 .. 18 hits each, and spread among them the loci of SPECIAL
    (edge_layout(n_small) says where).  Hits unique, grouped by locus, sorted by (left, right); masses from MASSES."""
    if oracle is None:
        from oracle import OracleLib, build
        build(with_ref=False)
        oracle = OracleLib()
    rng = np.random.default_rng(SEED)
    where = {l: name for name, l in edge_layout(n_small).items()}
    loci, keyed = [], set()
    for l in range(n_small + len(SPECIAL)):
        base = 10000 + STRIDE * l
        if l in where:
            isos, pairs = build_locus(rng, where[l], base)
            n_want = len(pairs)
        else:
            n_want = int(rng.integers(12, 19))
            isos, pairs = build_small(rng, small_width(l, grid), base, n_want + 3)
            pairs = [pairs[k] for k in rng.permutation(len(pairs))]
        loci.append(isos)
        own = set()
        for lb, rb in pairs:
            if len(own) == n_want:
                break
            f = eb.hit_features(list(lb), list(rb))
            if f is not None:
                own.add((l, f[1][0], f[2][-1], tuple(map(tuple, f))))
        keyed |= own
    annot = eb.Annotation(loci)
    keyed = sorted(keyed)
    hits = eb.Hits([k[0] for k in keyed], [k[3] for k in keyed])
    # exact bin counts: the bins as the library numbers them (by first appearance), the hits of the surplus ones dropped
    compat, key = oracle.exonbin_batch(annot, hits)
    off = np.searchsorted(hits.hit_locus, np.arange(annot.n_loci + 1), side="left")
    drop = np.zeros(hits.n_hits, bool)
    for name, want in EXACT_BINS.items():
        l = edge_layout(n_small)[name]
        b = bins_by_first_appearance(compat, key, off[l], off[l + 1])
        assert b.max() + 1 >= want, (name, int(b.max()) + 1)
        drop[off[l]:off[l + 1]] = b >= want
    hits = select_hits(hits, np.nonzero(~drop)[0])
    hits.mass = np.ascontiguousarray(MASSES[np.random.default_rng(SEED + 1).integers(0, MASSES.size, hits.n_hits)])
    return annot, hits


def locus_ranges(offsets, l):
    return int(offsets[l]), int(offsets[l + 1])


def sample_conditions(annot, hits, bins, F, status, keep, n_cand, posterior, n_small):
    """What the sample must hold for the tests on it to mean something (asserted by every test module that uses it).
    bins: LocusBins with hit_bin; F: the bin weights; status / keep: the EM's and the epilogue's; n_cand, posterior: by_hand()'s.
    -> the figures, for the tests' own messages"""
    at = edge_layout(n_small)
    nl = annot.n_loci
    hit_off = np.searchsorted(hits.hit_locus, np.arange(nl + 1), side="left")
    hits_of = np.diff(hit_off)
    niso, nb = np.diff(annot.iso_off), np.diff(bins.row_off)
    assert nl == n_small + len(SPECIAL) and nl > 2 * SCAN_ROUND and hits.n_hits < 250000
    assert (np.diff(hits.hit_locus) >= 0).all() and set(np.unique(hits.mass).tolist()) == set(MASSES.tolist())
    for name, l in at.items():
        assert niso[l] == WIDTH[name], (name, niso[l])
    # A: three work items, the last one partial; B: two; both keep their sums in LDS, A in copies
    assert 2 * ITEM_HITS < hits_of[at["A"]] < 3 * ITEM_HITS and 2 <= niso[at["A"]] <= 8
    assert ITEM_HITS < hits_of[at["B"]] < 2 * ITEM_HITS and 33 <= niso[at["B"]] <= 64
    # C: the column loop strides, F is not staged; >= 9 compat words
    assert niso[at["C"]] > 256 and nb[at["C"]] * niso[at["C"]] > 4096 and annot.compat_words >= 9
    for name, want in EXACT_BINS.items():
        assert nb[at[name]] == want, (name, nb[at[name]])
    assert nb[at["T1024"]] * niso[at["T1024"]] == 4096 and nb[at["T1025"]] * niso[at["T1025"]] > 4096
    # the locus without hits between two that have some; the locus whose hits are in no bin
    e, n = at["EMPTY"], at["NOBIN"]
    assert hits_of[e] == 0 and hits_of[e - 1] > 0 and hits_of[e + 1] > 0
    assert hits_of[n] > 0 and (np.asarray(bins.hit_bin)[hit_off[n]:hit_off[n + 1]] == -1).all() and nb[n] == 0
    small = np.ones(nl, bool)
    small[list(at.values())] = False
    assert set(niso[small].tolist()) == {2, 3} and hits_of[small].min() >= 12 and hits_of[small].max() <= 18
    # the device grouping's condition under fractional masses: at most RUN_CAP fragments of one bin start at one position
    binned = np.nonzero(np.asarray(bins.hit_bin) >= 0)[0]
    first_left = hits.feat_left[hits.feat_off[:-1]].astype(np.int64)
    _, per_run = np.unique(np.stack([np.asarray(bins.hit_bin)[binned], first_left[binned]]), axis=1, return_counts=True)
    assert per_run.max() <= RUN_CAP, per_run.max()
    # dead bins (every weight <= 1e-5)
    dead = 0
    for l in np.nonzero(nb > 0)[0]:
        f0, f1 = locus_ranges(bins.f_off, l)
        dead += int((np.asarray(F[f0:f1]).reshape(nb[l], niso[l]).max(axis=1) <= 1e-5).sum())
    assert dead > 0
    i0, i1 = locus_ranges(annot.iso_off, at["B"])
    erased_b = int((np.asarray(keep[i0:i1]) == 0).sum())
    assert 0 < erased_b < i1 - i0, erased_b
    c0, c1 = locus_ranges(annot.iso_off, at["C"])
    assert (np.asarray(keep[c0:c1]) != 0).any()
    ok = float((np.asarray(status) == 0).mean())
    assert ok >= 0.9, ok
    n_cand = np.asarray(n_cand)
    multi = {}
    for name in ("A", "B", "C"):
        h0, h1 = locus_ranges(hit_off, at[name])
        multi[name] = float((n_cand[h0:h1] > 1).mean())
    assert multi["B"] > 0.25 and multi["C"] > 0.25 and multi["A"] > 0.0, multi
    gap = 1.0
    for h, p in enumerate(posterior):
        if p is not None and len(p) > 1:
            top = sorted(p.values())[-2:]
            gap = min(gap, top[1] - top[0])
    assert gap >= 1e-6, gap         # no MAP decision rests on a rounding
    return dict(hits=hits.n_hits, loci=nl, items=n_items(hits_of), hits_A=int(hits_of[at["A"]]), hits_B=int(hits_of[at["B"]]),
                hits_C=int(hits_of[at["C"]]), bins_C=int(nb[at["C"]]), most_candidates=int(n_cand.max()), dead_bins=dead, erased_B=erased_b,
                em_ok=ok, multi=multi, smallest_gap=gap, longest_run=int(per_run.max()), hits_of=hits_of, hit_off=hit_off)


def device_conditions(figures, cu_count):
    """... and what only the device decides: more loci and more work items than two passes of the grid"""
    grid = GRID_PER_CU * cu_count
    assert figures["loci"] > 2 * SCAN_ROUND and figures["loci"] > 2 * grid and figures["items"] > 2 * grid, (figures["loci"], figures["items"], grid)
    return grid


def n_small_for(cu_count):
    """What the GPU tests build: more loci than two rounds of the row scan and than twice the grid"""
    return max(8200, 2 * GRID_PER_CU * cu_count + 100)


def n_items(hits_of_locus):
    """work items of either stage: a locus' hits in ranges of at most ITEM_HITS (a locus without hits has none)"""
    h = np.asarray(hits_of_locus, np.int64)
    return int((-(-h // ITEM_HITS)).sum())

"""Helpers for the device bin grouping's tests (csrc/bins_device.h driven by sbgpu_bins_create_device).

restate(): the grouping rule a second time, in plain numpy / Python, written from include/sbgpu.h and the comments of
csrc/locus_bins.cpp and not from its code.  Per locus: a hit enters when its compat and its key words are both nonzero; a bin
is keyed by the key words; bins are numbered by first appearance; a bin's compat is the OR over its members; its count is the
sum -- sequential, in np.float32, truncated to int32 -- of the masses of its distinct fragments in Contig::operator< order
(the (offset, length) lists compared as tuples: a proper prefix first), of equal fragments the first one's mass.

The seeded case builders (SYNTHETIC, GENUINE) sit on the limits of the kernels: table capacities +-1, the run cap, the scans' tile, the
pair kernels' switches.  Two kinds of words.  Synthetic: the annotation lets every isoform hold every exon, so any key is
consistent; a hit's words are a function of the bin the builder gives it, fragments are distinct unless copied on purpose, and
a copy carries its original's words (the single-pass kernels rest on "equal fragments have equal words").  Genuine: made from
the fragments by the exon-bin kernel (GPU) or the oracle (CPU); the pair arrays are compared on those.

Form selection (csrc/bins_schedule.h): compat and key of up to two words each take the single-pass kernels ("single": 20
isoforms, 40 segments); three key words the two-pass kernel ("two": 80 segments; "two_cw3": 70 isoforms too, which keeps a
bin's count and compat in global memory)."""
import ctypes as C

import numpy as np

import exonbin_util as XU
from strawberry_amd import exonbin as eb

SMALL_HITS, MAX_SMALL, MAX_LIGHT, MAX_MID, MAX_BIG = 256, 256, 512, 1400, 5600   # hits / bins per locus the tables hold
RUN_CAP, SCAN_TILE, HEAVY_FLOOR = 48, 4096, 8192
FORMS = {"single": (20, 40), "two": (20, 80), "two_cw3": (70, 80)}               # form -> (isoforms, segments)

TABLE_FULL = "more bins than the LDS table holds"
RUN_TOO_LONG = "more than 48 fragments of one bin starting at one position"
UNSORTED = "not sorted by (left, right)"
FRACTIONAL_TOO = "fractional hit masses next to another obstacle"
MASS_OVERFLOW = "a bin's mass reaches 2^24"
NOT_UNDER = "does not sit under an isoform"


# ------------------------------------------------------------------ moved here from tests/test_exonbin_gpu.py
def bins_arrays(b):
    return [b.row_off, b.f_off, b.count, b.bin_key, b.bin_compat, np.asarray(b.hit_bin), b.pair_seg_off, b.pair_seg_lens,
            b.pair_implicit_mask, b.pair_iso_len, b.pair_out_index]


def bins_arrays_no_pairs(b):
    return [b.row_off, b.f_off, b.count, b.bin_key, b.bin_compat, np.asarray(b.hit_bin)]


def group_both_ways(ctx, annot, hits, compat, key, want_hit_bin=True, host=None, with_host=True):
    """(device bins or None, host bins) for arbitrary word arrays (they need not come from the kernel).
    want_hit_bin=False: the device form is not asked for hit -> bin (its hit_bin stays None); host: bins made earlier;
    with_host=False: the host form is not run (None stands for its bins)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = {k: up(getattr(hits, k).view(np.int32) if getattr(hits, k).dtype == np.uint32 else getattr(hits, k))
         for k in ("hit_locus", "feat_off", "feat_code", "feat_left", "feat_right")}
    d_mass, d_compat, d_key = up(hits.mass), up(compat.view(np.int32)), up(key.view(np.int32))
    d_hit_bin = torch.zeros(hits.n_hits, dtype=torch.int64, device=dev)
    from strawberry_amd import _lib
    ht = _lib.sbgpu_hits_t(hits.n_hits, d["hit_locus"].data_ptr(), d["feat_off"].data_ptr(), d["feat_code"].data_ptr(),
                           d["feat_left"].data_ptr(), d["feat_right"].data_ptr())
    bd = eb.LocusBins.on_device(ctx, annot, hits, ht, d_mass.data_ptr(), compat.shape[1], key.shape[1], d_compat.data_ptr(),
                                d_key.data_ptr(), d_hit_bin.data_ptr() if want_hit_bin else None,
                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if bd is not None and want_hit_bin:
        bd.hit_bin = d_hit_bin.cpu().numpy()
    if host is None and with_host:
        host = eb.LocusBins(annot, hits, compat, key)
    return bd, host


def group_on_device(ctx, case, want_hit_bin):
    """-> (device bins or None, why the device form declined)"""
    from strawberry_amd import _lib
    bd, _ = group_both_ways(ctx, case.annot, case.hits, case.compat, case.key, want_hit_bin=want_hit_bin, with_host=False)
    return bd, "" if bd is not None else _lib.load().sbgpu_last_error().decode()


# ------------------------------------------------------------------ the restatement
class Restated:
    pass


def restate(annot, hits, compat, key):
    """-> Restated with row_off, f_off, count, bin_key, bin_compat, hit_bin, n_hits_used, dup (per hit: an equal fragment of
    its bin came earlier), and per bin: hit_order_count (the same masses added in hit order), naive_count (every member's mass,
    duplicates included, in double), float_sum (the float32 sum before truncation), members (hits in the bin)."""
    nl, nh = annot.n_loci, hits.n_hits
    loc = hits.hit_locus
    assert nh == 0 or (np.diff(loc) >= 0).all()
    off = np.searchsorted(loc, np.arange(nl + 1), side="left")
    enters = (compat != 0).any(axis=1) & (key != 0).any(axis=1) if nh else np.zeros(0, bool)
    left = hits.feat_left.tolist()
    width = (hits.feat_right - hits.feat_left).astype(np.uint32).tolist()
    fo = hits.feat_off.tolist()
    key_rows = [tuple(r) for r in key.tolist()]
    mass = hits.mass.astype(np.float32)
    hit_bin, dup = np.full(nh, -1, np.int64), np.zeros(nh, bool)
    row_off, f_off = np.zeros(nl + 1, np.int64), np.zeros(nl + 1, np.int64)
    counts, hit_order, naive, fsum, n_members, bin_key, bin_compat = [], [], [], [], [], [], []
    zero32 = np.float32(0.0)
    for l in range(nl):
        first = {}                     # key words -> bin of the locus
        frags, comp, every, members = [], [], [], []
        base = len(counts)
        for h in range(int(off[l]), int(off[l + 1])):
            if not enters[h]:
                continue
            b = first.get(key_rows[h])
            if b is None:
                b = first[key_rows[h]] = len(frags)
                frags.append({})
                comp.append(np.zeros(compat.shape[1], np.uint32))
                every.append(0.0)
                members.append(0)
                bin_key.append(key[h])
            comp[b] |= compat[h]
            every[b] += float(mass[h])
            members[b] += 1
            hit_bin[h] = base + b
            f = tuple(zip(left[fo[h]:fo[h + 1]], width[fo[h]:fo[h + 1]]))
            if f in frags[b]:
                dup[h] = True          # std::set: the first one inserted stays
            else:
                frags[b][f] = mass[h]
        for b, fr in enumerate(frags):
            s = zero32
            for f in sorted(fr):       # Contig::operator<
                s = np.float32(s + fr[f])
            t = zero32
            for m in fr.values():      # (dicts keep insertion order: the hits' order)
                t = np.float32(t + m)
            fsum.append(float(s))
            counts.append(int(s) if s < 2.0 ** 31 else -1)      # (beyond int32 the conversion is undefined: never compared)
            hit_order.append(int(t) if t < 2.0 ** 31 else -1)
        naive += every
        n_members += members
        bin_compat += comp
        row_off[l + 1] = row_off[l] + len(frags)
        f_off[l + 1] = f_off[l] + len(frags) * int(annot.iso_off[l + 1] - annot.iso_off[l])
    r = Restated()
    r.row_off, r.f_off = row_off, f_off
    r.count = np.asarray(counts, np.int64).astype(np.int32)
    r.bin_key = np.asarray(bin_key, np.uint32).reshape(len(counts), key.shape[1])
    r.bin_compat = np.asarray(bin_compat, np.uint32).reshape(len(counts), compat.shape[1])
    r.hit_bin, r.dup, r.n_hits_used = hit_bin, dup, int(enters.sum())
    r.hit_order_count = np.asarray(hit_order, np.int64).astype(np.int32)
    r.naive_count, r.float_sum, r.members = np.asarray(naive), np.asarray(fsum), np.asarray(n_members, np.int64)
    return r


def restated_arrays(r):
    return [r.row_off, r.f_off, r.count, r.bin_key, r.bin_compat, r.hit_bin]


def locus_classes(hits_per_locus):
    """csrc/bins_schedule.h restated: small loci (up to 256 hits), heavy ones (at least max(8192, 3 x the mean)), the rest."""
    n = np.asarray(hits_per_locus, np.int64)
    heavy = max(HEAVY_FLOOR, 3 * (int(n.sum()) // max(len(n), 1)))
    small = n <= SMALL_HITS
    return small, ~small & (n >= heavy), ~small & (n < heavy)


def longest_run(case, r):
    """The most distinct fragments of one bin that start at one position."""
    h = case.hits
    keep = (r.hit_bin >= 0) & ~r.dup
    first_left = h.feat_left[h.feat_off[:-1][keep]].astype(np.int64)
    _, n = np.unique(np.stack([r.hit_bin[keep], first_left]), axis=1, return_counts=True)
    return int(n.max())


# ------------------------------------------------------------------ cases
class Case:
    """annot, hits, compat, key; decline: None, or the texts the device form's refusal must hold; host: sbgpu_bins_create
    takes the input and defines the answer; props(case, r): the property the case exists for, asserted on the restatement."""

    def __init__(self, name, annot, hits, compat, key, decline=None, host=True, genuine=False, props=None, **meta):
        self.name, self.annot, self.hits = name, annot, hits
        self.compat, self.key = np.ascontiguousarray(compat, np.uint32), np.ascontiguousarray(key, np.uint32)
        self.decline, self.host, self.genuine, self.props, self.meta = decline, host, genuine, props, meta

    def per_locus(self):
        return np.bincount(self.hits.hit_locus, minlength=self.annot.n_loci)


def synth_annotation(form, n_loci):
    n_iso, n_seg = FORMS[form]
    loci = [[[(1000000 * (l + 1) + 100 * k, 1000000 * (l + 1) + 100 * k + 49) for k in range(n_seg)]] * n_iso for l in range(n_loci)]
    a = eb.Annotation(loci)
    assert a.compat_words == (n_iso + 31) // 32 and a.key_words == (n_seg + 31) // 32
    return a


def words_of_bins(form, n_bins):
    """Synthetic words of a locus' bins 0 .. n_bins-1: distinct nonzero keys inside the form's segments (an odd multiplier is
    a bijection modulo a power of two), nonzero compats inside its isoforms."""
    n_iso, n_seg = FORMS[form]
    kw, cw = (n_seg + 31) // 32, (n_iso + 31) // 32
    key, compat = np.zeros((n_bins, kw), np.uint32), np.zeros((n_bins, cw), np.uint32)
    for i in range(n_bins):
        v = ((i + 1) * 0x9E3779B97F4A7C15) & ((1 << n_seg) - 1)
        c = (((i + 1) * 0x2545F4914F6CDD1D) & ((1 << n_iso) - 1)) | 1
        for w in range(kw):
            key[i, w] = (v >> (32 * w)) & 0xFFFFFFFF
        for w in range(cw):
            compat[i, w] = (c >> (32 * w)) & 0xFFFFFFFF
    assert len(set(map(tuple, key.tolist()))) == n_bins and (key != 0).any(axis=1).all()
    return key, compat


class SynthBatch:
    """Loci of one form, filled part by part; finish() sorts every locus by (left, right) -- a stable sort, so copies
    stay behind their originals -- and gives the hits their bins' words."""

    def __init__(self, form, n_loci, seed):
        self.form, self.n_loci, self.rng = form, n_loci, np.random.default_rng(seed)
        self.parts = [[] for _ in range(n_loci)]
        self.n_bins = [0] * n_loci

    def base(self, l):
        return 1000000 * (l + 1)

    def _add(self, l, nfeat, code, left, right, mass, bins, zero=None):
        n = len(nfeat)
        self.parts[l].append(dict(nfeat=np.asarray(nfeat, np.int64), code=np.asarray(code, np.uint8), left=np.asarray(left, np.int64),
                                  right=np.asarray(right, np.int64), mass=np.asarray(mass, np.float32), bins=np.asarray(bins, np.int64),
                                  zero=np.zeros(n, bool) if zero is None else zero))
        if n:
            self.n_bins[l] = max(self.n_bins[l], int(np.max(bins)) + 1)

    def plain(self, l, n_hits, n_bins, mass=None, zero_frac=0.0, first_bin=0, at=0, span=60000):
        """n_hits distinct single-block fragments over exactly n_bins bins (every bin has a hit that enters), in an order in
        which the bins' first hits are shuffled; whole-number masses 1-3 unless given; zero_frac: hits without a compatible
        isoform among those a bin does not need."""
        rng = self.rng
        assert n_hits >= n_bins and n_hits <= span
        pick = np.concatenate([np.arange(n_bins), rng.integers(0, max(n_bins, 1), n_hits - n_bins)]).astype(np.int64)
        zero = np.concatenate([np.zeros(n_bins, bool), rng.random(n_hits - n_bins) < zero_frac])
        order = rng.permutation(n_hits)
        left = self.base(l) + at + np.sort(rng.choice(span, n_hits, replace=False))
        m = rng.integers(1, 4, n_hits).astype(np.float32) if mass is None else np.broadcast_to(np.asarray(mass, np.float32), (n_hits,))
        self._add(l, np.ones(n_hits, np.int64), np.zeros(n_hits, np.uint8), left, left + 74, m, first_bin + pick[order], zero[order])

    def runs(self, l, bin_of_run, sizes, masses, at=100000, copies=()):
        """Per run k a bin and sizes[k] fragments that start at one position: fragment j is block [L, L+60-j], mate gap,
        block [L+100, L+150+j].  The hits' order (by right end) is j ascending, the set's order (by the first block's length)
        j descending.  masses: one per fragment, run after run.  copies: (run, j, mass) -- an equal fragment behind the
        original."""
        nfeat, code, left, right, mass, bins = [], [], [], [], [], []
        extra = {}
        for k, j, m in copies:
            extra.setdefault((k, j), []).append(m)
        at_mass = 0
        for k, (b, n) in enumerate(zip(bin_of_run, sizes)):
            assert n <= 50
            L = self.base(l) + at + 300 * k
            for j in range(n):
                for m in [masses[at_mass]] + extra.get((k, j), []):
                    nfeat.append(3)
                    code += [0, 2, 0]
                    left += [L, L + 61 - j, L + 100]
                    right += [L + 60 - j, L + 99, L + 150 + j]
                    mass.append(m)
                    bins.append(b)
                at_mass += 1
        self._add(l, nfeat, code, left, right, mass, bins)

    def finish(self, name, swap_last_two_of=None, **kw):
        form = self.form
        annot = synth_annotation(form, self.n_loci)
        loc, nfeat, code, left, right, mass, key, compat = [], [], [], [], [], [], [], []
        for l, parts in enumerate(self.parts):
            if not parts:
                continue
            p = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
            start = np.concatenate([[0], np.cumsum(p["nfeat"])])
            first_left, last_right = p["left"][start[:-1]], p["right"][start[1:] - 1]
            order = np.lexsort((last_right, first_left))            # stable
            if swap_last_two_of == l:
                order[-2:] = order[-2:][::-1]
                assert (first_left[order[-2]], last_right[order[-2]]) > (first_left[order[-1]], last_right[order[-1]])
            lens = p["nfeat"][order]
            idx = np.repeat(start[:-1][order] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
            tk, tc = words_of_bins(form, self.n_bins[l])
            k_l, c_l = tk[p["bins"][order]], tc[p["bins"][order]].copy()
            c_l[p["zero"][order]] = 0
            loc.append(np.full(len(order), l, np.int32)), nfeat.append(lens), code.append(p["code"][idx]), left.append(p["left"][idx])
            right.append(p["right"][idx]), mass.append(p["mass"][order]), key.append(k_l), compat.append(c_l)
        nfeat = np.concatenate(nfeat)
        hits = eb.Hits.from_arrays(np.concatenate(loc), np.concatenate([[0], np.cumsum(nfeat)]), np.concatenate(code), np.concatenate(left),
                                   np.concatenate(right), np.concatenate(mass))
        return Case(name, annot, hits, np.concatenate(compat), np.concatenate(key), **kw)


def neighbours(s, loci):
    """ordinary loci around the ones a case is about: small ones, one of a few hundred hits, hits that enter no bin"""
    for i, l in enumerate(loci):
        n = [40, 700, 120, 256, 9][i % 5]
        s.plain(l, n, max(1, n // 3), zero_frac=0.1)


# ---- capacities
def _bins_are(expect):
    def props(case, r):
        nb = np.diff(r.row_off)
        for l, n in expect.items():
            assert nb[l] == n, (l, nb[l], n)
    return props


def capacities(form):
    """One batch: loci on every table's limit, ordinary neighbours between them."""
    s = SynthBatch(form, 16, seed=11)
    neighbours(s, [0, 3, 6, 9, 12, 15])
    s.plain(1, 256, 256)                   # small table: every hit its own bin
    s.plain(2, 256, 1)                     # ... and one bin
    s.plain(4, 257, 257)                   # one hit more: the next table's (257 bins: the small one could not hold them)
    s.plain(5, 600, MAX_LIGHT)
    s.plain(7, 600, MAX_LIGHT + 1)
    s.plain(8, 9000 if form == "single" else 1500, MAX_MID)
    s.plain(10, 9000 if form == "single" else 1500, MAX_MID + 1)
    s.plain(11, 6000, MAX_BIG)
    expect = {1: 256, 2: 1, 4: 257, 5: MAX_LIGHT, 7: MAX_LIGHT + 1, 8: MAX_MID, 10: MAX_MID + 1, 11: MAX_BIG}

    def props(case, r):
        _bins_are(expect)(case, r)
        n = case.per_locus()
        small, heavy, mid = locus_classes(n)
        assert n[1] == n[2] == 256 and small[1] and small[2] and n[4] == 257 and mid[4] and mid[5] and mid[7] and mid[11]
        assert (heavy[8] and heavy[10] and n[8] >= HEAVY_FLOOR) if form == "single" else (mid[8] and mid[10])
    return s.finish("capacities_" + form, props=props)


def big_table_overflow(form):
    s = SynthBatch(form, 3, seed=12)
    neighbours(s, [0, 2])
    s.plain(1, 6000, MAX_BIG + 1)
    return s.finish("big_table_5601_" + form, decline=[TABLE_FULL], props=_bins_are({1: MAX_BIG + 1}))


# ---- fractional masses
def _thirds(rng, n):
    """sums of 1, 1/2, 1/3 (NH 1-3, collapsed copies)"""
    return (rng.choice(np.asarray([1.0, 0.5, 1.0 / 3.0], np.float32), n) * rng.integers(1, 4, n).astype(np.float32)).astype(np.float32)


def _run_masses(rng, n):
    """the same sums, mostly 1/3 and 1/3 + 1/3: totals that land next to whole numbers, where the order of the additions decides
    the last bit and the truncation shows it"""
    t = np.float32(1.0 / 3.0)
    tt = np.float32(t + t)
    return rng.choice(np.asarray([t, tt, 1.0, 0.5, np.float32(tt + tt)], np.float32), n, p=[0.45, 0.4, 0.05, 0.05, 0.05])


def _order_matters(case, r):
    differ = int((r.count != r.hit_order_count).sum())
    assert differ >= 20, differ


def fractional(form, seed=21):
    """Loci of more than 256 and more than 512 bins whose bins each hold a run of 3-12 fragments starting at one position,
    the set's order the reverse of the hits'; in the single-pass form the 513-bin locus is redone by the big table first.
    A copy with another fractional mass behind some fragments: the first one's mass counts."""
    s = SynthBatch(form, 5, seed=seed)
    rng = s.rng
    neighbours(s, [0, 2, 4])
    copies_made = 0
    for l, nb in ((1, 400), (3, MAX_LIGHT + 1)):
        sizes = rng.integers(3, 13, nb)
        copies = [(int(k), int(rng.integers(0, sizes[k])), float(_thirds(rng, 1)[0])) for k in rng.choice(nb, 40, replace=False)]
        copies_made += len(copies)
        s.runs(l, rng.permutation(nb), sizes, _run_masses(rng, int(sizes.sum())), copies=copies)
    for l in (0, 2, 4):      # the neighbours' masses are fractional too
        for p in s.parts[l]:
            p["mass"] = _thirds(rng, len(p["mass"]))

    def props(case, r):
        _bins_are({1: 400, 3: MAX_LIGHT + 1})(case, r)
        _order_matters(case, r)
        assert r.dup.sum() == copies_made
        assert (np.abs(r.naive_count - r.float_sum) > 0.2).sum() >= 20      # ... and the copies' masses would show
        assert longest_run(case, r) == 12
    return s.finish("fractional_" + form, props=props)


def run_cap(n, form="single"):
    """One bin with n distinct fragments starting at one position, fractional masses; other runs of the locus are short."""
    s = SynthBatch(form, 3, seed=22 + n)
    rng = s.rng
    neighbours(s, [0, 2])
    sizes = np.asarray([5, n, 7, 3])
    s.runs(1, [0, 1, 2, 1], sizes, _thirds(rng, int(sizes.sum())))

    def props(case, r):
        assert longest_run(case, r) == n
    return s.finish("run_of_%d_%s" % (n, form), decline=[RUN_TOO_LONG] if n > RUN_CAP else None, props=props)


def fractional_unsorted():
    s = SynthBatch("single", 3, seed=23)
    neighbours(s, [0, 2])
    s.plain(1, 300, 40, mass=_thirds(s.rng, 300))
    return s.finish("fractional_unsorted", swap_last_two_of=1, decline=[UNSORTED, FRACTIONAL_TOO])


# ---- mass limits
def mass_limit(form, which):
    """One bin whose 255, 256 or 512 hits of whole-number mass total 2^24 - 1, 2^24, 2^32 and 2^32 - 256.  With the 100 hits of
    its 30 other bins the locus has 355-612 hits: a light locus of the single-pass form, a middle one of the two-pass form;
    the neighbours are ordinary."""
    n, m = {"below": (255, 65793.0), "reaches": (256, 65536.0), "wrap_to_0": (512, 8388608.0), "wrap_negative": (256, 16777215.0)}[which]
    s = SynthBatch(form, 3, seed=31)
    neighbours(s, [0, 2])
    s.plain(1, n, 1, mass=m, span=4000)
    s.plain(1, 100, 30, first_bin=1, at=5000)

    def props(case, r):
        assert r.members[r.row_off[1]:r.row_off[2]].max() == n and float(np.float32(m)) == m and m < 2 ** 24
        assert r.naive_count[r.row_off[1]:r.row_off[2]].max() == {"below": 2 ** 24 - 1, "reaches": 2 ** 24, "wrap_to_0": 2 ** 32, "wrap_negative": 2 ** 32 - 256}[which]
    return s.finish("mass_%s_%s" % (which, form), decline=None if which == "below" else [MASS_OVERFLOW], host=which == "below", props=props)


# ---- declines
def unsorted_1025():
    s = SynthBatch("single", 3, seed=41)
    neighbours(s, [0, 2])
    s.plain(1, 1025, 90)
    return s.finish("unsorted_last_two_of_1025", swap_last_two_of=1, decline=[UNSORTED])


def not_under():
    """Synthetic words whose compat names an isoform that lacks the bin's segments: isoform 1 of locus 1 holds two exons only."""
    full = [(1000000 + 100 * k, 1000000 + 100 * k + 49) for k in range(40)]
    full2 = [(2000000 + 100 * k, 2000000 + 100 * k + 49) for k in range(40)]
    annot = eb.Annotation([[full] * 3, [full2, full2[:2], full2]])
    rng = np.random.default_rng(42)
    n = 80
    left = np.concatenate([1000000 + np.sort(rng.choice(3000, n, replace=False)), 2000000 + np.sort(rng.choice(3000, n, replace=False))])
    key = np.zeros((2 * n, 2), np.uint32)
    key[:, 0] = rng.integers(1, 2 ** 16, 2 * n) << 4           # segments 4 and up: isoform 1 of locus 1 has none of them
    compat = np.full((2 * n, 1), 5, np.uint32)
    compat[n + 7, 0] = 7                                        # one hit says isoform 1 too
    hits = eb.Hits.from_arrays(np.repeat([0, 1], n), np.arange(2 * n + 1), np.zeros(2 * n, np.uint8), left, left + 74)
    return Case("not_under_an_isoform", annot, hits, compat, key, decline=[NOT_UNDER], host=False)


def ordinary(form="single"):
    s = SynthBatch(form, 6, seed=43)
    neighbours(s, range(5))
    return s.finish("ordinary_" + form)


# ---- scans and strides
def scan_case(n_loci, n_two_iso, seed, redo=True, name=None):
    """n_loci loci of three exons and one isoform, n_two_iso of them (None: about half) with two; 0-3 hits per locus (a
    quarter of the loci are empty, the last one is not); with `redo`, one locus in the middle of 40 segments, 600 hits and
    513 bins, which the light table hands to the big one: its count is negative when the speculative scan runs."""
    rng = np.random.default_rng(seed)
    two = rng.random(n_loci) < 0.5 if n_two_iso is None else np.isin(np.arange(n_loci), rng.choice(n_loci, n_two_iso, replace=False))
    mid = n_loci // 2 if redo else -1
    loci = []
    for l in range(n_loci):
        ex = [(10000 * (l + 1) + 100 * k, 10000 * (l + 1) + 100 * k + 49) for k in range(40 if l == mid else 3)]
        loci.append([ex] * (2 if two[l] else 1))
    annot = eb.Annotation(loci)
    assert annot.key_words == (2 if redo else 1) and annot.compat_words == 1
    n = rng.integers(0, 4, n_loci)
    n[-1] = 3
    if redo:
        n[mid] = 600
    loc = np.repeat(np.arange(n_loci), n)
    rank = np.arange(len(loc)) - np.repeat(np.cumsum(n) - n, n)
    left = 10000 * (loc + 1) + 10 * rank
    key = np.zeros((len(loc), annot.key_words), np.uint32)
    key[:, 0] = rng.integers(1, 8, len(loc))                    # three segments
    compat = np.where(two[loc], rng.integers(1, 4, len(loc)), 1).astype(np.uint32).reshape(-1, 1)
    compat[rng.random(len(loc)) < 0.05] = 0
    mass = rng.integers(1, 4, len(loc)).astype(np.float32)
    if redo:
        tk, tc = words_of_bins("single", MAX_LIGHT + 1)
        pick = rng.permutation(np.concatenate([np.arange(MAX_LIGHT + 1), rng.integers(0, MAX_LIGHT + 1, 600 - MAX_LIGHT - 1)]))
        key[loc == mid] = tk[pick]
        compat[loc == mid, 0] = (tc[pick, 0] & (3 if two[mid] else 1)) | 1
    hits = eb.Hits.from_arrays(loc, np.arange(len(loc) + 1), np.zeros(len(loc), np.uint8), left, left + 74, mass)
    n_iso = int(annot.iso_off[-1])

    def props(case, r):
        nb = np.diff(r.row_off)
        assert case.annot.n_loci == n_loci and (n_two_iso is None or n_iso == n_loci + n_two_iso)
        assert (case.per_locus() == 0).sum() > n_loci // 8 and nb[-1] > 0 and (not redo or nb[mid] == MAX_LIGHT + 1)
        assert r.row_off[min(n_loci, SCAN_TILE) - 1] > 0
    return Case(name or "scan_%d_loci_%d_isoforms" % (n_loci, n_iso), annot, hits, compat, key, props=props, n_iso=n_iso)


def small_loci_past_two_grids(cus=256):
    """More than 2 x (4 x 8 x CUs) loci of 0-3 hits: the small step's grid and the pack kernel's are crossed twice."""
    base = scan_case(129, None, seed=57, redo=False, name="base")
    copies = -(-(2 * 4 * 8 * cus + 1) // 129)
    annot, hits = XU.tile(base.annot, base.hits, copies)

    def props(case, r):
        assert case.annot.n_loci > 2 * 4 * 8 * cus and case.per_locus().max() <= 3
    return Case("small_loci_past_two_grids", annot, hits, np.tile(base.compat, (copies, 1)), np.tile(base.key, (copies, 1)), props=props)


# ---- genuine words
class GeneBatch:
    """Genes of evenly spaced exons; isoform 0 holds every exon, isoform j drops one inner exon.  Fragments: a block inside
    an exon, two blocks with a mate gap between, blocks joined by introns."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.loci, self.exons, self.rows = [], [], []

    def gene(self, n_exons, n_iso, exon_len=100, step=200):
        base = 1000000 * (len(self.loci) + 1)
        ex = [(base + step * k, base + step * k + exon_len - 1) for k in range(n_exons)]
        self.loci.append([ex] + [[e for k, e in enumerate(ex) if k != 1 + (j % (n_exons - 2))] for j in range(n_iso - 1)])
        self.exons.append(ex)
        self.rows.append([])
        return len(self.loci) - 1

    def single(self, l, a, o, n=30):
        x = self.exons[l][a][0] + o
        return ([0], [x], [x + n - 1])

    def paired(self, l, a, b, o1, o2, n=20):
        x, y = self.exons[l][a][0] + o1, self.exons[l][b][0] + o2
        assert x + n < y
        return ([0, 2, 0], [x, x + n, y], [x + n - 1, y - 1, y + n - 1])

    def spliced(self, l, exon_list, o1, o2):
        """first exon from offset o1 to its end, the exons between whole, the last exon up to offset o2"""
        ex = [self.exons[l][a] for a in exon_list]
        code, left, right = [], [], []
        for i, (el, er) in enumerate(ex):
            if i:
                code.append(1), left.append(ex[i - 1][1] + 1), right.append(el - 1)
            code.append(0), left.append(el + o1 if i == 0 else el), right.append(el + o2 if i == len(ex) - 1 else er)
        return (code, left, right)

    def random_frags(self, l, n, exon_len=100):
        """n distinct fragments, sorted by (left, right)"""
        rng, ne, seen = self.rng, len(self.exons[l]), {}
        while len(seen) < n:
            u, a = rng.random(), int(rng.integers(0, ne))
            if u < 0.4:
                f = self.single(l, a, int(rng.integers(0, exon_len - 30)))
            elif u < 0.8:
                b = min(ne - 1, a + int(rng.integers(1, 4)))
                if b == a:
                    continue
                f = self.paired(l, a, b, int(rng.integers(0, exon_len - 20)), int(rng.integers(0, exon_len - 20)))
            else:
                b = a + int(rng.integers(1, 3))
                if b >= ne:
                    continue
                f = self.spliced(l, [a, b], int(rng.integers(0, exon_len - 10)), int(rng.integers(10, exon_len)))
            seen[tuple(map(tuple, f))] = f
        return sorted(seen.values(), key=lambda f: (f[1][0], f[2][-1]))

    def put(self, l, frags, masses=None):
        """the locus' hits, in this order"""
        m = self.rng.integers(1, 5, len(frags)).astype(np.float32) if masses is None else masses
        self.rows[l] = [(f, float(x)) for f, x in zip(frags, m)]

    def finish(self, name, words, sorted_hits=True, **kw):
        annot = eb.Annotation(self.loci)
        loc = [l for l, rows in enumerate(self.rows) for _ in rows]
        flat = [r for rows in self.rows for r in rows]
        if sorted_hits:
            for rows in self.rows:
                k = [(f[1][0], f[2][-1]) for f, _ in rows]
                assert k == sorted(k)
        hits = eb.Hits(loc, [f for f, _ in flat], mass=[m for _, m in flat])
        compat, key = words(annot, hits)
        return Case(name, annot, hits, compat, key, genuine=True, **kw)


GENUINE_FORMS = {"single": (12, 3), "two": (70, 3), "two_cw3": (70, 66)}      # form -> (exons, isoforms) of the genes


def _copy_behind(frags, masses, i, mass):
    frags.insert(i + 1, frags[i])
    masses.insert(i + 1, mass)


def _stride_run(frags, masses, at, lo):
    """Rearranges the sorted fragments so that a run of one (left, right) lies across local hit index at | at + 1:
    B1, B2, A | A, B3, B1 -- A one block, the B's its span as two blocks with a mate gap at three places (other sequences, the
    same exon, the same bin).  The second A finds the first at once; the second B1 has to walk back over the boundary, past
    hits of its span and other hashes.  Fragments from index lo on are dropped to bring a one-block fragment into place."""
    s = next(i for i in range(at + 5, len(frags)) if len(frags[i][0]) == 1)
    n_drop = s - (at - 2)
    assert lo + n_drop <= s - 3
    del frags[lo:lo + n_drop], masses[lo:lo + n_drop]
    A = frags[at - 2]
    x, y = A[1][0], A[2][0]
    assert y == x + 29
    B = [([0, 2, 0], [x, x + 4 + k, y - 3 - k], [x + 3 + k, y - 4 - k, y]) for k in (1, 2, 3)]
    frags[at - 2:at - 1] = [B[0], B[1], A, A, B[2], B[0]]
    masses[at - 2:at - 1] = [2.0, 3.0, masses[at - 2], 7.0, 4.0, 9.0]
    assert frags[at] == frags[at + 1] == A and frags[at + 3] == frags[at - 2] and len({(f[1][0], f[2][-1]) for f in frags[at - 2:at + 4]}) == 1


def _code_variants(g, l, form):
    """Hits of equal coordinates under other codes -- block to an exon's end, connector exactly over the isoform's intron,
    block from the next exon's start; the connector a mate gap (G) or an intron (I) -- in both orders.  They are one
    std::set element wherever they share a bin.  Over adjacent exons both enter with the same words; over exons a, a + 2 the
    intron fits only an isoform that drops exon a + 1 (other compat, the same key: still one bin), and where no isoform
    drops it the intron hit enters no bin (N) -- such a hit in front of an entering one must not make that one a duplicate.
    -> fragments, masses, and per hit whether it enters and whether it is a duplicate, in the locus' order."""
    ne, ni = GENUINE_FORMS[form]
    dropped = {1 + (j % (ne - 2)) for j in range(ni - 1)}
    kept = [a for a in range(ne - 2) if a + 1 not in dropped]
    skip = [a for a in range(ne - 2) if a + 1 in dropped]
    assert kept and skip
    code = {"G": 2, "I": 1, "N": 1}
    groups = []     # (a, b, kinds)
    for t, kinds in enumerate(["GI", "IG", "GIG", "IGI", "GI", "IG"] * 3):
        groups.append((t % (ne - 1), t % (ne - 1) + 1, kinds))                      # adjacent exons
    for t, kinds in enumerate(["GI", "IG", "IGG", "GII"] * 3):
        groups.append((skip[t % len(skip)], skip[t % len(skip)] + 2, kinds))        # the intron of an isoform that drops a + 1
    for t, kinds in enumerate(["NG", "NGG", "NNG", "GN", "NGN", "NG"] * 4):
        groups.append((kept[t % len(kept)], kept[t % len(kept)] + 2, kinds))        # no isoform has this intron
    rows = []
    for t, (a, b, kinds) in enumerate(groups):
        (al, ar), (bl, _) = g.exons[l][a], g.exons[l][b]
        o, k = 3 + 2 * (t % 40), 10 + (7 * t) % 60
        seen = False
        for q, c in enumerate(kinds):
            f = ([0, code[c], 0], [al + o, ar + 1, bl], [ar, bl - 1, bl + k])
            rows.append((f, 2.0 + 3 * q + t % 2, c != "N", c != "N" and seen))
            seen = seen or c != "N"
    rows.sort(key=lambda r: (r[0][1][0], r[0][2][-1]))      # (stable; groups differ in (left, right))
    assert len({(r[0][1][0], r[0][2][-1]) for r in rows}) == len(groups)
    return [r[0] for r in rows], [r[1] for r in rows], np.asarray([r[2] for r in rows]), np.asarray([r[3] for r in rows])


def duplicates(form, words):
    """Locus 1: runs of one (left, right) across local hit indices 255|256 and 1023|1024, an equal pair on either side of the
    boundary (_stride_run).  Locus 2: A, B, A with B of A's span but gapped; a GAP -> INTRON variant behind its original (off
    the exons' ends: it enters no bin); five equal fragments; random copies.  Locus 4: equal coordinates under other codes
    (_code_variants).  Ordinary genes around them."""
    ne, ni = GENUINE_FORMS[form]
    g = GeneBatch(seed=61)
    for _ in range(5):
        g.gene(ne, ni)
    g.put(0, g.random_frags(0, 150))
    frags = g.random_frags(1, 1300)
    masses = g.rng.integers(1, 5, len(frags)).astype(np.float32).tolist()
    _stride_run(frags, masses, 255, 0)
    _stride_run(frags, masses, 1023, 270)
    g.put(1, frags, masses)
    frags = g.random_frags(2, 400)
    masses = g.rng.integers(1, 5, len(frags)).astype(np.float32).tolist()
    n_gapped = 0
    for i in range(len(frags) - 1, -1, -1):          # (from the back: insertions leave the indices before them alone)
        f, u = frags[i], g.rng.random()
        if len(f[0]) == 1 and u < 0.2:                # A, B, A: B = A's span as two blocks with a mate gap, in the same exon
            x, y = f[1][0], f[2][0]
            frags[i + 1:i + 1] = [([0, 2, 0], [x, x + 10, y - 9], [x + 9, y - 10, y]), f]
            masses[i + 1:i + 1] = [2.0, 5.0]
            n_gapped += 1
        elif len(f[0]) == 3 and f[0][1] == 2 and u < 0.15:      # same coordinates, GAP turned INTRON
            frags.insert(i + 1, ([0, 1, 0], f[1], f[2]))
            masses.insert(i + 1, 3.0)
        elif u < 0.25:
            for k in range(4 if u < 0.2 else 1):      # five equal fragments, or two
                _copy_behind(frags, masses, i, 1.0 + k)
    g.put(2, frags, masses)
    g.put(3, g.random_frags(3, 257))
    vf, vm, v_enters, v_dup = _code_variants(g, 4, form)
    g.put(4, vf, vm)

    def props(case, r):
        assert n_gapped > 10 and r.dup.sum() > 60
        one = np.nonzero(case.hits.hit_locus == 1)[0]
        for at in (255, 1023):                        # B1, B2, A | A, B3, B1
            assert r.dup[one[at - 2:at + 4]].tolist() == [False, False, False, True, False, True]
            assert len(set(r.hit_bin[one[at - 2:at + 4]].tolist())) == 1 and r.hit_bin[one[at]] >= 0
        four = case.hits.hit_locus == 4
        np.testing.assert_array_equal(r.hit_bin[four] >= 0, v_enters)        # which variants enter a bin ...
        np.testing.assert_array_equal(r.dup[four], v_dup)                    # ... and which are duplicates
        assert (~v_enters).sum() >= 30 and v_dup.sum() >= 40 and (v_enters & ~v_dup).sum() >= 50
        assert (r.naive_count != r.count).sum() > 20                  # counting every hit would change counts
        assert np.diff(r.row_off).min() > 5
    return g.finish("duplicates_" + form, words, props=props)


def _all_pairs(ne):
    return [(a, b) for a in range(ne) for b in range(a + 1, ne)]


def duplicates_big_table(form, words):
    """A locus with more bins than the light (single-pass) or the middle (two-pass) table holds -- one fragment per pair of
    exons -- and equal fragments behind some of them: the big table's kernel applies the duplicate rule."""
    ne, ni = {"single": (40, 3), "two": (70, 3)}[form]
    want = (MAX_LIGHT if form == "single" else MAX_MID) + 40
    g = GeneBatch(seed=62)
    for _ in range(3):
        g.gene(ne, ni)
    g.put(0, g.random_frags(0, 120))
    g.put(2, g.random_frags(2, 300))
    pairs = [_all_pairs(ne)[i] for i in g.rng.choice(len(_all_pairs(ne)), want, replace=False)]
    frags = sorted([g.paired(1, a, b, 10 + (a + b) % 50, 5 + (3 * a + b) % 60) for a, b in pairs], key=lambda f: (f[1][0], f[2][-1]))
    masses = g.rng.integers(1, 5, len(frags)).astype(np.float32).tolist()
    for i in range(len(frags) - 1, -1, -7):
        _copy_behind(frags, masses, i, 6.0)
    g.put(1, frags, masses)

    def props(case, r):
        assert np.diff(r.row_off)[1] == want and r.dup.sum() > 50 and (r.naive_count != r.count).sum() > 50
    return g.finish("duplicates_big_table_" + form, words, props=props)


def pairs_64_65_isoforms(words):
    """Twin loci of 64 and 65 isoforms, the same exons and fragments: the wave kernel makes the pairs of the one, the thread
    kernel the other's."""
    g = GeneBatch(seed=71)
    a, b = g.gene(20, 64), g.gene(20, 65)
    fa = g.random_frags(a, 500)
    shift = g.exons[b][0][0] - g.exons[a][0][0]
    g.put(a, fa, np.ones(len(fa)))
    g.put(b, [(c, [x + shift for x in le], [x + shift for x in ri]) for c, le, ri in fa], np.ones(len(fa)))

    def props(case, r):
        assert np.diff(case.annot.iso_off).tolist() == [64, 65] and np.diff(r.row_off)[0] == np.diff(r.row_off)[1] > 64
        np.testing.assert_array_equal(r.count[:r.row_off[1]], r.count[r.row_off[1]:])
    return g.finish("pairs_64_65_isoforms", words, props=props)


def pairs_bins_per_locus(words):
    """Loci of exactly 64, 65, 128 and 129 bins (one key per exon or pair of exons): the wave's rounds of 64 bins."""
    g = GeneBatch(seed=72)
    want = [64, 65, 128, 129]
    for n in want:
        l = g.gene(20, 5)
        combos = ([(a, a) for a in range(20)] + _all_pairs(20))[:n]
        frags = []
        for a, b in combos:
            for o in (3, 17, 40):
                frags.append(g.single(l, a, o) if a == b else g.paired(l, a, b, o, o + 5))
        g.put(l, sorted(frags, key=lambda f: (f[1][0], f[2][-1])))
    return g.finish("pairs_64_65_128_129_bins", words, props=_bins_are(dict(enumerate(want))))


def pairs_wide(apart, words):
    """An isoform of 72 single-exon segments (a wave-kernel locus; one of 65 such isoforms besides: the thread kernel's) and
    fragments whose two blocks sit `apart` isoform segments from each other: 31 gives pairs of 32 segments with the 30 inner
    ones implicit, 32 pairs of 33 -- no segments, not an error.  And a bin that holds segments 63, 64, 65."""
    g = GeneBatch(seed=73)
    for n_iso in (1, 65):
        l = g.gene(72, 1, exon_len=50, step=100)
        g.loci[l] = g.loci[l] * n_iso
        frags = [g.paired(l, a, a + apart, 5, 9, n=15) for a in range(0, 72 - apart, 3)]
        frags += [g.paired(l, a, a + 2, 5, 9, n=15) for a in range(0, 70, 5)]
        frags.append(g.spliced(l, [63, 64, 65], 10, 20))
        g.put(l, sorted(frags, key=lambda f: (f[1][0], f[2][-1])))

    def props(case, r):
        assert np.diff(case.annot.seg_off).tolist() == [72, 72] and case.annot.key_words == 3
        k = r.bin_key[:r.row_off[1]]
        lo = np.asarray([min(i for i in range(96) if (int(row[i >> 5]) >> (i & 31)) & 1) for row in k])
        hi = np.asarray([max(i for i in range(96) if (int(row[i >> 5]) >> (i & 31)) & 1) for row in k])
        assert (hi - lo == apart).sum() >= 10 and (hi - lo).max() == apart
        assert ((k[:, 1] >> 31) & 1 & k[:, 2] & (k[:, 2] >> 1)).any()         # segments 63, 64 and 65 in one bin
    return g.finish("pairs_%d_segments_apart" % apart, words, props=props)


def unsorted_genuine(words):
    """what LocusQuantifier gets in the decline test: the last two hits of a 1025-hit locus swapped"""
    g = GeneBatch(seed=74)
    g.gene(12, 3), g.gene(12, 3)
    g.put(0, g.random_frags(0, 200))
    frags = g.random_frags(1, 1025)
    frags[-2:] = frags[-2:][::-1]
    g.put(1, frags)
    return g.finish("unsorted_genuine", words, sorted_hits=False, decline=[UNSORTED])


SYNTHETIC = {}
for _form in ("single", "two"):
    SYNTHETIC["capacities_" + _form] = lambda f=_form: capacities(f)
    SYNTHETIC["big_table_5601_" + _form] = lambda f=_form: big_table_overflow(f)
    SYNTHETIC["fractional_" + _form] = lambda f=_form: fractional(f)
for _form in ("single", "two", "two_cw3"):
    for _which in ("below", "reaches", "wrap_to_0", "wrap_negative"):
        SYNTHETIC["mass_%s_%s" % (_which, _form)] = lambda f=_form, w=_which: mass_limit(f, w)
SYNTHETIC.update({
    "run_of_48_single": lambda: run_cap(48), "run_of_49_single": lambda: run_cap(49), "fractional_unsorted": fractional_unsorted,
    "unsorted_last_two_of_1025": unsorted_1025, "not_under_an_isoform": not_under,
    "scan_4095_loci_4096_isoforms": lambda: scan_case(4095, 1, seed=51), "scan_4095_loci_4097_isoforms": lambda: scan_case(4095, 2, seed=52),
    "scan_4096_loci": lambda: scan_case(4096, None, seed=53, name="scan_4096_loci"), "scan_4097_loci": lambda: scan_case(4097, None, seed=54, name="scan_4097_loci"),
    "scan_8193_loci": lambda: scan_case(2 * SCAN_TILE + 1, None, seed=55, name="scan_8193_loci"),
})
GENUINE = {"pairs_64_65_isoforms": pairs_64_65_isoforms, "pairs_64_65_128_129_bins": pairs_bins_per_locus,
           "pairs_31_segments_apart": lambda w: pairs_wide(31, w), "pairs_32_segments_apart": lambda w: pairs_wide(32, w)}
for _form in ("single", "two", "two_cw3"):
    GENUINE["duplicates_" + _form] = lambda w, f=_form: duplicates(f, w)
for _form in ("single", "two"):
    GENUINE["duplicates_big_table_" + _form] = lambda w, f=_form: duplicates_big_table(f, w)
MASS_WRAPS = [n for n in SYNTHETIC if n.startswith(("mass_wrap", "mass_reaches"))]

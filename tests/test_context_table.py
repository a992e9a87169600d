"""The `-f` fragment-context table as arrays: sbgpu_context_table_host (csrc/context_host.cpp), the CPU statement of what the
device form computes, against output.py::context_table (the per-hit walk the drivers used to write out by hand) and the
reference's own ctx.tsv files.

No GPU here: the hits' compat / key words and the bin weights come from the oracle's restatement, as in the other CPU
tests (sbgpu_exonbin_host and sbgpu_binweight_host take host BUFFERS but run the kernels; tests/test_context_table_gpu.py
runs the same directories through them)."""
import ctypes as C
import os

import numpy as np
import pytest

import e2e_util as U
import exonbin_util as XU
from strawberry_amd import _lib, context
from strawberry_amd import exonbin as eb
from strawberry_amd.output import context_table

MEAN, SD, RL = 250.0, 30.0, 75
NINE = ["E2E", "E2E_LONG", "E2E_MASS", "E2E_FILTER", "E2E_EMP", "E2E_SINGLE", "E2E_LONGREAD", "E2E_MINUS", "E2E_CHROMS"]


class Handle:
    """An sbgpu_bins_t from sbgpu_bins_create that lives as long as the test needs it (LocusBins destroys its own)."""

    def __init__(self, annot, hits, compat, key):
        self.L = _lib.load()
        self.compat = np.ascontiguousarray(compat, np.uint32).reshape(hits.n_hits, -1)
        key = np.ascontiguousarray(key, np.uint32).reshape(hits.n_hits, -1)
        a, h = annot._struct(), hits._struct()
        self.h = C.c_void_p()
        _lib.check(self.L.sbgpu_bins_create(C.byref(a), C.byref(h), hits.mass.ctypes.data, self.compat.shape[1], key.shape[1],
                                            self.compat.ctypes.data, key.ctypes.data, C.byref(self.h)), "sbgpu_bins_create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.sbgpu_bins_destroy(self.h)


def arrays_by_hand(bins, compat, F, keep, status=None):
    """output.py::context_table's walk, kept as arrays instead of printed: (locus_row_off, locus_hits, row_bin, row_hits, rows' probabilities)."""
    keep = np.asarray(keep) != 0
    n_in_bin, last_hit = np.zeros(bins.n_bins, np.int64), np.full(bins.n_bins, -1, np.int64)
    hit_locus = np.searchsorted(bins.row_off, bins.hit_bin, side="right") - 1
    for h in np.nonzero(bins.hit_bin >= 0)[0]:
        l = hit_locus[h]
        if status is not None and status[l] == _lib.EM_INIT_EMPTY:
            continue
        i0, niso = int(bins.iso_off[l]), int(bins.iso_off[l + 1] - bins.iso_off[l])
        if any((int(compat[h][j >> 5]) >> (j & 31)) & 1 and keep[i0 + j] for j in range(niso)):
            n_in_bin[bins.hit_bin[h]] += 1
            last_hit[bins.hit_bin[h]] = h
    off, lhits, rbin, rhits, probs = [0], [], [], [], []
    for l in range(bins.n_loci):
        b0, b1 = int(bins.row_off[l]), int(bins.row_off[l + 1])
        niso = int(bins.iso_off[l + 1] - bins.iso_off[l])
        coords = bins.bin_coords(l)
        lhits.append(int(n_in_bin[b0:b1].sum()) & 0xffffffff)
        Fl = np.asarray(F[bins.f_off[l]:bins.f_off[l + 1]]).reshape(b1 - b0, niso)
        for b in sorted(range(b1 - b0), key=lambda k: coords[k]):
            if n_in_bin[b0 + b]:
                words = compat[last_hit[b0 + b]]
                rbin.append(b0 + b)
                rhits.append(int(n_in_bin[b0 + b]))
                probs.append([Fl[b, j] if (int(words[j >> 5]) >> (j & 31)) & 1 else 0.0 for j in range(niso)])
        off.append(len(rbin))
    return off, lhits, rbin, rhits, probs


def check_arrays(t, bins, want):
    off, lhits, rbin, rhits, probs = want
    assert t.n_rows == len(rbin)
    assert t.locus_row_off.tolist() == off and t.locus_hits.tolist() == lhits
    assert t.row_bin.tolist() == rbin and t.row_hits.tolist() == rhits
    for l in range(bins.n_loci):
        for r in range(off[l], off[l + 1]):
            assert t.row(l, r, bins.iso_off, bins.f_off).tolist() == probs[r], (l, r)     # exact: copies of F, or 0.0


def oracle_weights(oracle, bins, ins, long_read):
    F = np.zeros(bins.n_elem)
    for p in range(bins.n_pairs):
        if long_read:       # estimate.cpp:236-247: 1 / L_j, no table
            F[bins.pair_out_index[p]] = 1.0 / int(bins.pair_iso_len[p])
            continue
        s = slice(bins.pair_seg_off[p], bins.pair_seg_off[p + 1])
        imp = [k for k in range(32) if (int(bins.pair_implicit_mask[p]) >> k) & 1]
        F[bins.pair_out_index[p]] = oracle.bin_weight(bins.pair_seg_lens[s], imp, int(bins.pair_iso_len[p]), RL, ins)
    return F


def toy_inputs(oracle, which):
    """One toy directory up to the table's inputs, all on the CPU: words, bins, weights, the oracle's EM and epilogue."""
    from strawberry_amd.binweight import InsertSize
    d = getattr(U, which)
    ordered, rows, gtf, _ = U.load(d)
    annot, hits, names, _ = XU.e2e_inputs(d, ordered)
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    if which == "E2E_EMP":
        fl = eb.frag_lens(annot, hits, compat)
        law = InsertSize.from_frag_lens(fl)
        ins = oracle.make_insert(law.mean, law.sd, frag_lens=fl)
    else:
        ins = oracle.make_insert(200.0, 80.0) if which in ("E2E_SINGLE", "E2E_LONGREAD") else oracle.make_insert(MEAN, SD)
    F = oracle_weights(oracle, bins, ins, which == "E2E_LONGREAD")
    theta, status, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    ab = oracle.abundance(bins.iso_off, theta, status, bins.iso_len, hits.total_mapped,
                          min_isoform_frac=0.05 if which == "E2E_FILTER" else 0.0)
    return d, ordered, rows, annot, hits, names, compat, key, bins, F, status, ab


@pytest.mark.parametrize("which", NINE)
def test_host_form_on_the_toy_directories(oracle, which):
    """The host form's arrays == the per-hit walk's, exactly; its text == output.py::context_table's == the reference's file."""
    d, ordered, rows, annot, hits, names, compat, key, bins, F, status, ab = toy_inputs(oracle, which)
    with Handle(annot, hits, compat, key) as H:
        t = context.context_table_host(H.h, compat, F=F, keep=ab["keep"], status=status)
    check_arrays(t, bins, arrays_by_hand(bins, compat, F, ab["keep"], status))
    assert t.n_rows == len(rows)
    tx = [[n for n, _ in ordered[g]] for g in names]
    coords = [c for l in range(bins.n_loci) for c in bins.bin_coords(l)]
    text = context.format_table(t, "toy", hits.total_mapped, names, tx, bins.row_off, bins.iso_off, bins.f_off, lambda b: coords[b],
                                ab["fpkm"], ab["frac"], keep=ab["keep"])
    assert text == context_table("toy", hits.total_mapped, names, tx, bins, compat, F, ab["fpkm"], ab["frac"], keep=ab["keep"])
    assert text == open(os.path.join(d, "ctx.tsv")).read()


def test_the_last_hit_of_a_bin_decides_its_columns(oracle):
    """Isoform A = [1-100],[201-300], isoform B = [1-300].  X: a pair, blocks [50-90] and [210-250], the mate gap between
    them -- compatible with both.  Y: one spliced read [80-100] + [201-220] -- its intron [101-200] exists in A only
    (Contig::is_compatible, contig.cpp:577-582).  Both overlap exactly the segments [1-100] and [201-300]: one bin.  The
    row's column for B is F when X is the bin's last hit and 0.0 when Y is (eb_prob_map is overwritten hit by hit)."""
    annot = eb.Annotation([[[(1, 100), (201, 300)], [(1, 300)]]])
    assert annot.segments(0) == [(1, 100), (101, 200), (201, 300)]
    X = eb.hit_features([(50, 90)], [(210, 250)])
    Y = eb.hit_features([(80, 100), (201, 220)], [])
    for order, b_column_is_f in (((Y, X), True), ((X, Y), False)):
        hits = eb.Hits([0, 0], list(order))
        compat, key = oracle.exonbin_batch(annot, hits)
        cx, cy = (int(compat[1, 0]), int(compat[0, 0])) if b_column_is_f else (int(compat[0, 0]), int(compat[1, 0]))
        assert cx == 0b11 and cy == 0b01                 # X fits A and B, Y fits A only
        assert key[0].tolist() == key[1].tolist() == [0b101]  # the same two segments: the same bin
        bins = eb.LocusBins(annot, hits, compat, key)
        assert bins.n_bins == 1 and bins.hit_bin.tolist() == [0, 0]
        F = np.array([0.25, 0.125])
        with Handle(annot, hits, compat, key) as H:
            t = context.context_table_host(H.h, compat, F=F)
        assert t.n_rows == 1 and t.row_hits.tolist() == [2] and t.locus_hits.tolist() == [2] and t.row_bin.tolist() == [0]
        assert t.row(0, 0, bins.iso_off, bins.f_off).tolist() == ([0.25, 0.125] if b_column_is_f else [0.25, 0.0])
        check_arrays(t, bins, arrays_by_hand(bins, compat, F, [1, 1]))


def key_sets(rng, nseg, n_random):
    """Random segment sets over nseg segments, and for each of them S every S + {one segment above max(S)}: the pairs the
    prefix rule decides."""
    sets = set()
    for _ in range(n_random):
        k = int(rng.integers(1, min(nseg, 6) + 1))
        sets.add(frozenset(int(x) for x in rng.choice(nseg, size=k, replace=False)))
    for S in list(sets):
        for h in range(max(S) + 1, nseg):
            sets.add(S | {h})
    return sorted(sets, key=lambda s: sorted(s))[::-1]     # (any order but the expected one)


def keyed_locus(nseg, sets):
    """One locus of one isoform with nseg exons (= nseg segments) and one hit per key set, its key words set by hand."""
    annot = eb.Annotation([[[(1000 * s + 1, 1000 * s + 500) for s in range(nseg)]]])
    assert len(annot.segments(0)) == nseg
    kw = annot.key_words
    key = np.zeros((len(sets), kw), np.uint32)
    for i, S in enumerate(sets):
        for s in S:
            key[i, s >> 5] |= np.uint32(1 << (s & 31))
    feats = [([0], [1000 * min(S) + 1 + i % 400], [1000 * min(S) + 60 + i % 400]) for i, S in enumerate(sets)]   # (distinct fragments)
    hits = eb.Hits([0] * len(sets), feats)
    return annot, hits, np.ones((len(sets), 1), np.uint32), key


@pytest.mark.parametrize("nseg", [1, 2, 31, 32, 33, 64, 65, 96, 97, 130])
def test_rows_come_in_the_order_of_the_coordinate_sets(nseg):
    """1 .. 5 key words: the library's order of a locus' rows == Python's order of the bins' coordinate tuples."""
    rng = np.random.default_rng(100 + nseg)
    sets = key_sets(rng, nseg, 40)
    annot, hits, compat, key = keyed_locus(nseg, sets)
    assert annot.key_words == (nseg + 31) // 32
    segs = annot.segments(0)
    with Handle(annot, hits, compat, key) as H:
        info = (C.c_int64 * 8)()
        _lib.check(H.L.sbgpu_bins_info(H.h, info), "sbgpu_bins_info")
        assert info[2] == len(sets)     # one bin per key, numbered by first appearance: bin i = sets[i]
        t = context.context_table_host(H.h, compat, F=np.ones(len(sets)))
    assert t.n_rows == len(sets) and (t.row_hits == 1).all()
    got = [tuple(segs[s] for s in sorted(sets[b])) for b in t.row_bin.tolist()]
    assert got == sorted(got)
    if nseg > 2:
        assert any(a == b[:len(a)] for a, b in zip(got, got[1:]))   # the prefix rule was exercised


def test_the_expression_filter_drops_bins_and_loci(oracle):
    """keep with erased isoforms: a bin whose hits all fit erased isoforms only has no row; a locus with nothing kept, or
    whose EM never started, has none; locus_hits counts the qualifying hits only."""
    # locus 0 and 1: isoforms A = [1-100],[201-300] and C = [1-100],[401-500]; locus 2: the same again
    iso = [[(1, 100), (201, 300)], [(1, 100), (401, 500)]]
    shift = lambda ex, d: [(a + d, b + d) for a, b in ex]  # noqa: E731
    annot = eb.Annotation([[shift(e, 10000 * l) for e in iso] for l in range(3)])
    feats, loc = [], []
    for l in range(3):
        d = 10000 * l
        feats += [eb.hit_features([(d + 220, d + 260)], []),   # A only
                  eb.hit_features([(d + 230, d + 270)], []),   # A only, the same bin
                  eb.hit_features([(d + 420, d + 460)], []),   # C only
                  eb.hit_features([(d + 10, d + 50)], [])]     # A and C
        loc += [l] * 4
    hits = eb.Hits(loc, feats)
    compat, key = oracle.exonbin_batch(annot, hits)
    assert compat[:4, 0].tolist() == [1, 1, 2, 3]
    bins = eb.LocusBins(annot, hits, compat, key)
    assert np.diff(bins.row_off).tolist() == [3, 3, 3]
    F = np.arange(1, bins.n_elem + 1) / 64.0
    keep = np.array([0, 1, 0, 0, 1, 1], np.int32)          # locus 0: A erased; locus 1: nothing kept; locus 2: all kept ...
    status = np.array([0, 0, _lib.EM_INIT_EMPTY], np.int32)  # ... but its EM never started
    with Handle(annot, hits, compat, key) as H:
        t = context.context_table_host(H.h, compat, F=F, keep=keep, status=status)
        t_all = context.context_table_host(H.h, compat, F=F)
    assert t.locus_row_off.tolist() == [0, 2, 2, 2] and t.locus_hits.tolist() == [2, 0, 0]
    assert t.row_hits.tolist() == [1, 1]            # the bin of the two A-only hits is gone
    assert sorted(t.row_bin.tolist()) == [1, 2]      # (bins by first appearance: 0 the A-only hits, 1 C only, 2 both)
    check_arrays(t, bins, arrays_by_hand(bins, compat, F, keep, status))
    assert t_all.locus_row_off.tolist() == [0, 3, 6, 9] and t_all.locus_hits.tolist() == [4, 4, 4]
    check_arrays(t_all, bins, arrays_by_hand(bins, compat, F, np.ones(6)))


def test_host_form_reports_what_is_missing(oracle):
    annot = eb.Annotation([[[(1, 100)]]])
    hits = eb.Hits([0], [eb.hit_features([(10, 50)], [])])
    compat, key = oracle.exonbin_batch(annot, hits)
    with Handle(annot, hits, compat, key) as H:
        with pytest.raises(_lib.SbgpuError, match="holds no weights"):
            context.context_table_host(H.h, compat)
        s = _lib.sbgpu_context_table_t()
        assert H.L.sbgpu_context_table_host(H.h, None, 1, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL
        assert H.L.sbgpu_context_table_host(None, None, 1, None, None, None, C.byref(s)) == _lib.SBGPU_EINVAL

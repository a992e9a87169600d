"""CPU tests of the samples behind tests/test_binweight_edges_gpu.py: conditions on the reference (the oracle's restatement
of the bin-weight model) alone -- that the samples reach what they are there to reach, so that the GPU comparisons are not
`0 == 0` -- and the helpers that build hand-made laws."""
import numpy as np

import binweight_util as U


def test_exact_sample_reaches_every_width_and_block_edge(oracle):
    """Every segment count 1..32 has non-zero effective lengths, both kinds of implicit set have thousands at >= 5 segments,
    blocks touch either edge of the inner segments and bit 30 of the mask, no effective length is negative."""
    U.exact_conditions(oracle)
    ref, cases = U.exact_reference(oracle)
    segs, imps = U.exact_sample()
    nseg = np.array([len(s) for s in segs])
    nz = sum((E != 0).sum(axis=0) for E in ref.values())
    print("cases", cases, "non-zero per segment count, min over 5..32:", min(int(nz[nseg == n].sum()) for n in range(5, 33)))


def test_exact_reference_is_gated_by_the_pair_range(oracle):
    """Rows of the reference outside a pair's [max(rl, inner), lmax] are 0 by construction; inside, they are the oracle's."""
    ref, _ = U.exact_reference(oracle)
    segs, imps = U.exact_sample()
    for rl, E in ref.items():
        assert E.shape == (max(int(s.sum()) for s in segs) + 1, len(segs))
        for p in range(0, len(segs), 7):
            lo, hi = U.fl_range(segs[p], rl)
            assert (E[:max(lo, 0), p] == 0).all() and (E[hi + 1:, p] == 0).all()
            for fl in range(lo, hi + 1, 5):
                assert E[fl, p] == oracle.effective_len(segs[p], imps[p], fl, rl)


def test_weight_sample_has_weights_to_compare(oracle):
    """Per segment count 5..32 at least 20 reference weights above 1e-30 under every law, 30 % overall, at most 2 000
    non-negative terms per weight (the bound behind the 1e-12 tolerance), closed-form pairs in nearly every batch."""
    U.weight_conditions(oracle)
    names = [n for n, _, _ in U.weight_laws()]
    assert len(names) == 5
    (_, rl_a, law_a), (_, rl_b, law_b) = U.weight_laws()[3:]
    assert law_a[1].min() < rl_a and law_b[1].min() > rl_b   # the start offset below and above the read length


def test_outlier_law_has_a_tiny_density_inside_its_support(oracle):
    """10^6 lengths from N(200, 25) and one of 1400: the oracle's own table has non-zero entries below 1e-280 strictly
    between entries at or above it (pdf_support[4] of the kernel), and the library builds the same table."""
    ins, o_ins = U.outlier_laws(oracle)
    assert ins.total_reads == 10 ** 6 + 1 and ins.end_offset == U.OUTLIER
    tab = np.array([oracle.insert_pdf(o_ins, fl) for fl in range(U.OUTLIER + 1)])
    small = np.nonzero((tab != 0) & (tab < U.TINY))[0]
    big = np.nonzero(tab >= U.TINY)[0]
    assert len(small) >= 10 and big[0] < small.min() and small.max() < big[-1] == U.OUTLIER
    assert U.tiny_inside(tab) and not U.tiny_inside(tab[:small.min()])
    assert ((tab == 0) | (tab >= U.DBL_MIN)).all()
    np.testing.assert_allclose(ins.pdf_table(U.OUTLIER + 1), tab, rtol=1e-14, atol=0)
    # the sample: ordinary pairs, pairs across the tiny densities, pairs up to the outlier, pairs left with tiny terms only
    segs, imps, lens = U.outlier_sample()
    rng_of = [U.fl_range(s, ins.start_offset) for s in segs]
    assert sum(hi <= 400 for _, hi in rng_of) >= 50
    assert sum(lo < small.min() and small.max() < hi < U.OUTLIER for lo, hi in rng_of) >= 50
    assert sum(hi >= U.OUTLIER for _, hi in rng_of) >= 50
    # the gap swallows all inner segments: fl >= inner + 2 rl, beyond the last density of 1e-280 from 946 bases on
    only_tiny = [p for p, s in enumerate(segs) if len(s) >= 3 and len(imps[p]) == len(s) - 2 and
                 U.inner_len(s) + 2 * U.OUTLIER_RL > big[big < small.min()].max() and int(s.sum()) < U.OUTLIER]
    ref = U.oracle_weights(oracle, segs, imps, lens, U.OUTLIER_RL, o_ins)
    assert len(only_tiny) >= 10 and (ref[only_tiny] != 0).sum() >= 5 and (ref[only_tiny] < 1e-270).all()
    assert (ref > 1e-30).sum() >= 100 and (ref == 0).sum() >= 5


def test_tiny_inside_definition():
    assert not U.tiny_inside([0, 0, 0]) and not U.tiny_inside([0, 1e-3, 0, 1e-3])
    assert U.tiny_inside([1e-3, 1e-300, 1e-3]) and not U.tiny_inside([1e-300, 1e-3, 1e-3, 1e-290])
    assert not U.tiny_inside([1e-3, 1e-280, 1e-3])


def test_hand_insert_is_the_table(oracle):
    """The oracle's density under hand_insert(table) is the table, entry by entry, and 0 beyond it; its weights flush a
    subnormal quotient to 0 like the reference's FTZ arithmetic (what the kernel's flushing loop mirrors)."""
    for name, t, off in U.hand_tables():
        ins = U.hand_insert(t, off)
        got = np.array([oracle.insert_pdf(ins, fl) for fl in range(len(t) + 5)])
        np.testing.assert_array_equal(got[:len(t)], t)
        assert (got[len(t):] == 0).all()
        assert U.tiny_inside(t) == (name in ("tiny_between", "tiny_only")), name
    t = np.zeros(50)
    t[10] = 2.5e-308
    ins = U.hand_insert(t, 0)
    assert oracle.bin_weight([10], [], 10, 5, ins) == 2.5e-308          # fl 10: effective length 1, L - fl + 1 == 1
    assert oracle.bin_weight([10], [], 1009, 5, ins) == 0.0             # 2.5e-308 / 1000 is subnormal: flushed
    segs, imps, lens = U.hand_sample()
    nseg = np.array([len(s) for s in segs])
    assert set(nseg) == set(range(1, 33))
    for name, t, off in U.hand_tables():
        ref = U.oracle_weights(oracle, segs, imps, lens, 50, U.hand_insert(t, off))
        if name == "all_zero":
            assert (ref == 0).all()
        elif name in ("first_entry", "last_entry"):
            assert 1 <= (ref != 0).sum() < len(ref) // 2, name
        elif name == "tiny_only":   # weights made of tiny terms alone, some of them flushed away entirely
            assert ((ref != 0) & (ref < 1e-290)).sum() >= 100 and (ref == 0).sum() >= 20 and (ref > 1e-30).sum() >= 20
            assert ((ref != 0) & (ref < 1e-290))[nseg >= 5].sum() >= 50
        else:
            assert (ref[nseg >= 5] > 1e-30).sum() >= 50 and (ref[nseg <= 4] > 1e-30).sum() >= 20, name


def test_batch_and_probe_samples(oracle):
    segs, imps, lens = U.batch_sample()
    assert len(segs) == 4099 and len(segs) % 64 != 0
    nseg = np.array([len(s) for s in segs])
    for b in range(0, len(segs), 64):
        assert (nseg[b:b + 64] <= 4).any() and (nseg[b:b + 64] >= 5).any()
    (nsegs, nimps, nlens), p12, p2 = U.probe_neighbours()
    assert len(nsegs) == 63 and all((len(s) <= 4) == (k % 2 == 0) for k, s in enumerate(nsegs))
    assert len(p12[0][0]) == 12 and U.block_kind(12, p12[1][0]) == U.KIND_BLOCK and len(p2[0][0]) == 2
    o_ins = oracle.make_insert(320.0, 60.0)
    for s, i, L in (p12, p2):
        assert oracle.bin_weight(s[0], i[0], L[0], 75, o_ins) > 1e-30

"""CPU checks of tests/fraglen_util.py: the numpy restatement of Sample::fragLenDist == the library's host form
(sbgpu_frag_lens_host) on the oracle's compat words, and the hand-built hits are what the GPU cases take them for."""
import numpy as np
import pytest

import fraglen_util as FU


def cases():
    from strawberry_amd import exonbin as eb
    rng = np.random.Generator(np.random.PCG64(12))
    big, pos = FU.make_locus(5000, [(2, 130, 90)] * 30 + [None, (3, 200, 150), "dup", (1, 9000, 0)] + [(1, 100, 0)] * 36)
    long, pos = FU.make_locus(pos + 5000, [(1, 10000, 0), (30, 500, 300), (3, 12000, 2000)])
    annot = eb.Annotation([big, [[(1, 50)]], long])
    hs = FU.HitSet()
    hs.add_pairs(rng, annot, 0, [j for j, x in enumerate(big) if x], 1500)
    hs.add_pairs(rng, annot, 0, [69], 20)
    hs.add_intronic(rng, annot, 0, 25)
    hs.add_featureless(0, 5)
    x0 = long[0][0][0]
    hs.add_blocks(2, [[(x0, x0 + L - 1)] for L in (8191, 8192, 8193)])
    hs.add_pairs(rng, annot, 2, [0, 1, 2], 600)
    return annot, hs.hits()


def test_reference_equals_host_form(oracle):
    from strawberry_amd import exonbin as eb
    annot, hits = cases()
    assert annot.compat_words == 3
    compat, _ = oracle.exonbin_batch(annot, hits)
    ref = FU.reference(annot, hits, compat)
    np.testing.assert_array_equal(ref["lens"], eb.frag_lens(annot, hits, compat))
    np.testing.assert_array_equal(ref["hist"], np.bincount(eb.frag_lens(annot, hits, compat)))
    rt = FU.routes(annot, hits, ref)
    assert (70, 69) in rt["marks"] and rt["word_1_plus"] > 0 and rt["scalar"] > 1000
    assert rt["no_features"] == 5 and rt["zero_compat"] >= 30 and rt["multi_compat"] > 0
    assert rt["global"] > 100 and {8191, 8192, 8193} <= set(ref["lens"].tolist())
    # the hits are grouped by locus and sorted by (left, right) inside it
    has, left, right = FU.hit_ends(hits)
    key = hits.hit_locus.astype(np.int64) * 2**40 + left * 2**20 + right
    assert (np.diff(hits.hit_locus) >= 0).all() and (np.diff(key) >= 0).all()


def test_exonic_overlap_by_hand():
    from strawberry_amd import exonbin as eb
    annot = eb.Annotation([[[(10, 19), (30, 39), (50, 59)], []]])
    iso = np.zeros(6, np.int64)
    left = np.array([10, 15, 20, 10, 35, 1])
    right = np.array([59, 35, 29, 10, 55, 100])
    np.testing.assert_array_equal(FU.exonic_overlaps_len(annot, iso, left, right), [30, 11, 0, 1, 11, 30])
    assert FU.exonic_overlaps_len(annot, np.array([1]), np.array([10]), np.array([59]))[0] == 0


@pytest.mark.parametrize("niso", [1, 31, 32, 33, 64, 65])
def test_unique_isoform_masks_the_last_word(niso):
    """bits past the locus' isoforms do not count (the kernel's mask of the last word)"""
    from strawberry_amd import exonbin as eb
    annot = eb.Annotation([[[(100 * j + 1, 100 * j + 50)] for j in range(niso)]])
    hits = eb.Hits([0, 0], [([0], [1], [10]), ([0], [1], [10])])
    cw = 3
    compat = np.full((2, cw), 0xFFFFFFFF, np.uint32)
    compat[0] = 0
    compat[0, (niso - 1) // 32] = 1 << ((niso - 1) % 32)
    if niso < 32 * cw:
        compat[1] = 0
        compat[1, niso // 32] |= np.uint32(1 << (niso % 32))    # a bit past the last isoform only: no isoform
    count, mark = FU.unique_isoform(annot, hits, compat)
    assert count[0] == 1 and mark[0] == niso - 1
    if niso < 32 * cw:
        assert count[1] == 0 and mark[1] == -1

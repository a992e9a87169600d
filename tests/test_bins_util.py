"""The device grouping's edge cases (tests/bins_util.py) without a GPU: the restatement of the grouping rule equals the host
form (sbgpu_bins_create) on every array, for every case the host form takes, and every case has the property it exists for --
bin counts exactly on a table's limit or one past it, loci in the class the schedule gives them, runs of 48 and 49, masses whose
summation order shows after truncation, duplicates that would change counts.  Genuine words come from the oracle here."""
import numpy as np
import pytest

import bins_util as B
from strawberry_amd import exonbin as eb


def check(case):
    r = B.restate(case.annot, case.hits, case.compat, case.key)
    if case.props:
        case.props(case, r)
    if not case.host:
        return r
    h = eb.LocusBins(case.annot, case.hits, case.compat, case.key)
    assert h.n_hits_used == r.n_hits_used
    for x, y in zip(B.restated_arrays(r), B.bins_arrays_no_pairs(h)):
        np.testing.assert_array_equal(x, y)
    return r


@pytest.mark.parametrize("name", sorted(B.SYNTHETIC))
def test_restatement_equals_host_form_on_synthetic_words(name):
    case = B.SYNTHETIC[name]()
    assert case.name == name
    check(case)


@pytest.mark.parametrize("name", sorted(B.GENUINE))
def test_restatement_equals_host_form_on_genuine_words(oracle, name):
    case = B.GENUINE[name](oracle.exonbin_batch)
    assert case.name == name and case.genuine
    r = check(case)
    assert r.n_hits_used > 0.5 * case.hits.n_hits


def test_small_loci_past_two_grids():
    check(B.small_loci_past_two_grids(cus=256))


def test_unsorted_hits_are_the_same_bins_as_sets(oracle):
    """the input of the quantifier's decline test: the host form takes it"""
    case = B.unsorted_genuine(oracle.exonbin_batch)
    h = eb.LocusBins(case.annot, case.hits, case.compat, case.key)
    assert h.n_bins > 20 and case.per_locus()[1] == 1025


def test_wide_pairs_have_the_masks_they_are_about(oracle):
    """32 segments: mask bits 1..30; 33: a pair without segments.  From the host form's pair arrays."""
    for apart, want_mask in ((31, 0x7FFFFFFE), (32, None)):
        case = B.pairs_wide(apart, oracle.exonbin_batch)
        h = eb.LocusBins(case.annot, case.hits, case.compat, case.key)
        n = np.diff(h.pair_seg_off)
        if want_mask is not None:
            assert (h.pair_implicit_mask[n == 32] == want_mask).sum() >= 20 and n.max() == 32
        else:
            assert (n == 0).sum() >= 20 and n.max() <= 3
        assert ((n == 3) & (h.pair_implicit_mask == 0)).sum() >= 2      # the bin of segments 63, 64, 65: nothing implicit


def test_the_restatement_on_a_case_worked_by_hand():
    """two bins; a duplicate (first copy's mass), a proper prefix before its extension, truncation"""
    annot = eb.Annotation([[[(100, 199), (300, 399)]] * 2])
    feats = [([0], [100], [150]), ([0, 2, 0], [100, 120, 300], [119, 299, 350]), ([0], [100], [150]), ([0], [100], [119]),
             ([0], [310], [350]), ([0], [320], [350])]
    hits = eb.Hits([0] * 6, feats, mass=[0.5, 1.0 / 3.0, 4.0, 1.0 / 3.0, 2.0, 1.0])
    key = np.asarray([[1], [1], [1], [1], [2], [0]], np.uint32)
    compat = np.asarray([[1], [2], [1], [1], [0], [3]], np.uint32)
    compat[4] = 1
    r = B.restate(annot, hits, compat, key)
    assert r.row_off.tolist() == [0, 2] and r.f_off.tolist() == [0, 4] and r.hit_bin.tolist() == [0, 0, 0, 0, 1, -1]
    assert r.dup.tolist() == [False, False, True, False, False, False] and r.n_hits_used == 5
    assert r.bin_compat[:, 0].tolist() == [3, 1] and r.bin_key[:, 0].tolist() == [1, 2]
    # set order: (100, 19) < (100, 19)(120, 179)(300, 50) < (100, 50)
    want = np.float32(np.float32(np.float32(1.0 / 3.0) + np.float32(1.0 / 3.0)) + np.float32(0.5))
    assert r.float_sum[0] == float(want) and r.count.tolist() == [1, 2]

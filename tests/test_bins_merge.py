"""The bin-table merge on the host (sbgpu_bins_merge_shapes_host / _fill_host, csrc/merge_host.cpp; merge.py) against
tests/merge_util.py::by_hand, bit for bit: the five EM goldens at three key widths with and without X; loci without bins;
identical and disjoint samples; idempotence; every refusal; and the merged tables as inputs of the unchanged differential rule
(diff.em_diff_host with the oracle's EM against diff_util.by_hand, under diff_util.compare's bound)."""
import numpy as np
import pytest

import diff_util as DU
import fit_util as FU
import merge_util as MU
from strawberry_amd import _lib, merge

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]


def within_limits(b):
    idx = np.nonzero((np.diff(b.row_off) <= 5632) & (np.diff(b.iso_off) <= 4096))[0]
    return b if len(idx) == b.n_loci else FU.select_loci(b, idx)


_cache = {}


def pair(golden, name, kw):
    if (name, kw) not in _cache:
        a = MU.sample_of_batch(within_limits(golden(name)[0]), kw, 11 + kw)
        _cache[(name, kw)] = MU.second_sample(a, 5 + kw)
    return _cache[(name, kw)]


@pytest.mark.parametrize("with_X", [True, False])
@pytest.mark.parametrize("kw", [1, 2, 3])
@pytest.mark.parametrize("name", GOLDENS)
def test_host_form_is_by_hands_bit_for_bit(golden, name, kw, with_X):
    a, b = pair(golden, name, kw)
    if not with_X:
        a, b = a.without_X(), b.without_X()
    want = MU.by_hand(a, b)
    t = merge.merge_host(a, b)
    MU.assert_same(t, want, "%s kw=%d" % (name, kw))
    assert (t.row_a < 0).any() and (t.row_b < 0).any() and ((t.row_a >= 0) & (t.row_b >= 0)).any()
    assert t.n_bins == len(want["row_a"]) and t.n_elem == len(want["F_a"])


def test_want_names_the_arrays():
    rng = np.random.default_rng(0)
    a, b = MU.one_locus_pair(*MU.split_keys(MU.distinct_keys(rng, 9, 2), 3, 3, rng), 4, rng)
    t = merge.merge_host(a, b, want=("row_b", "F_a"))
    want = MU.by_hand(a, b)
    assert t.row_a is None and t.count_a is None and t.F_b is None
    np.testing.assert_array_equal(t.row_b, want["row_b"])
    np.testing.assert_array_equal(t.F_a, want["F_a"])
    with pytest.raises(ValueError):
        merge.merge_host(a, b, want=("nope",))


def test_loci_without_bins():
    rng = np.random.default_rng(1)
    k = MU.distinct_keys(rng, 12, 2)
    none = np.zeros((0, 2), np.uint32)
    pairs = [MU.one_locus_pair(none, k[:4], 3, rng), MU.one_locus_pair(k[:5], none, 2, rng), MU.one_locus_pair(none, none, 3, rng),
             MU.one_locus_pair(k[:3], k[2:6], 0, rng), MU.one_locus_pair(*MU.split_keys(k, 4, 4, rng), 5, rng)]
    a, b = MU.concat(pairs)
    t = merge.merge_host(a, b)
    MU.assert_same(t, MU.by_hand(a, b))
    np.testing.assert_array_equal(np.diff(t.row_off), [4, 5, 0, 6, 12])
    assert (t.row_a[:4] == -1).all() and (t.row_b[4:9] == -1).all() and (t.count_a[:4] == 0).all()
    # a NULL-X sample takes the other's own weights
    np.testing.assert_array_equal(merge.merge_host(a.without_X(), b.without_X()).F_a[:12], b.F[:12])


def test_identical_samples_give_identity_maps():
    rng = np.random.default_rng(2)
    a, _ = MU.concat([MU.one_locus_pair(MU.distinct_keys(rng, n, 3), MU.distinct_keys(rng, 1, 3), K, rng) for n, K in ((7, 3), (1, 1), (30, 6))])
    b = MU.Sample(a.iso_off, a.row_off, a.key, a.count, a.F, rng.random(len(a.F)))
    a = MU.Sample(a.iso_off, a.row_off, a.key, a.count, a.F, rng.random(len(a.F)))
    t = merge.merge_host(a, b)
    np.testing.assert_array_equal(t.row_a, np.arange(len(a.count)))
    np.testing.assert_array_equal(t.row_b, np.arange(len(a.count)))
    for x in "ab":
        np.testing.assert_array_equal(getattr(t, "count_" + x), a.count)
        np.testing.assert_array_equal(getattr(t, "F_" + x).view(np.uint64), a.F.view(np.uint64))
    np.testing.assert_array_equal(t.row_off, a.row_off)


def test_disjoint_samples_stack():
    rng = np.random.default_rng(3)
    k = MU.distinct_keys(rng, 40, 2)
    a, b = MU.one_locus_pair(k[:17], k[17:], 4, rng)
    t = merge.merge_host(a, b)
    MU.assert_same(t, MU.by_hand(a, b))
    assert t.n_bins == 40 and (t.row_b[:17] == -1).all() and (t.row_a[17:] == -1).all()
    np.testing.assert_array_equal(t.row_b[17:], np.arange(23))
    np.testing.assert_array_equal(t.F_a[17 * 4:].view(np.uint64), a.X.view(np.uint64))
    np.testing.assert_array_equal(t.F_b[:17 * 4].view(np.uint64), b.X.view(np.uint64))


def test_merging_the_merged_tables_changes_nothing(golden):
    a, b = pair(golden, "em_c2_64", 2)
    t = merge.merge_host(a, b)
    union_key = np.where((t.row_a >= 0)[:, None], a.key[np.maximum(t.row_a, 0)], b.key[np.maximum(t.row_b, 0)])
    ua = MU.Sample(a.iso_off, t.row_off, union_key, t.count_a, t.F_a, np.full(t.n_elem, -1.0))
    ub = MU.Sample(a.iso_off, t.row_off, union_key, t.count_b, t.F_b, np.full(t.n_elem, -2.0))
    again = merge.merge_host(ua, ub)
    np.testing.assert_array_equal(again.row_a, np.arange(t.n_bins))
    np.testing.assert_array_equal(again.row_b, np.arange(t.n_bins))
    for k in ("row_off", "f_off", "count_a", "count_b"):
        np.testing.assert_array_equal(getattr(again, k), getattr(t, k))
    for k in ("F_a", "F_b"):
        np.testing.assert_array_equal(getattr(again, k).view(np.uint64), getattr(t, k).view(np.uint64))


def refusal(a, b, code, text):
    with pytest.raises(_lib.SbgpuError) as e:
        merge.merge_host(a, b)
    assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)


def test_refusals():
    rng = np.random.default_rng(4)
    k = MU.distinct_keys(rng, 20, 2)
    first = MU.one_locus_pair(k[:3], k[2:5], 2, rng)
    good = MU.one_locus_pair(*MU.split_keys(k, 6, 6, rng), 3, rng)
    dup = k[:8].copy()
    dup[6] = dup[1]
    for which in (0, 1):
        bad = MU.one_locus_pair(dup, k[8:14], 3, rng) if which == 0 else MU.one_locus_pair(k[8:14], dup, 3, rng)
        a, b = MU.concat([first, bad, good])
        refusal(a, b, _lib.SBGPU_EINVAL, "a duplicate bin key in locus 1")
    a, b = good
    # key_words, n_loci, iso_off
    b3 = MU.Sample(b.iso_off, b.row_off, np.concatenate([b.key, b.key[:, :1]], axis=1), b.count, b.F)
    refusal(a.without_X(), b3, _lib.SBGPU_EINVAL, "key_words")
    a2, b2 = MU.concat([first, good])
    refusal(a.without_X(), b2.without_X(), _lib.SBGPU_EINVAL, "n_loci")
    wide = MU.Sample([0, 4], b.row_off, b.key, b.count, np.zeros(4 * len(b.count)))
    refusal(a.without_X(), wide, _lib.SBGPU_EINVAL, "iso_off")
    # a union over the limit; the same loci one row shallower pass
    deep = MU.distinct_keys(rng, 5633, 2)
    a, b = MU.concat([(first[0].without_X(), first[1].without_X()), MU.one_locus_pair(deep[:3000], deep[2000:], 1, rng, with_X=False)])
    refusal(a, b, _lib.SBGPU_ESHAPE, "the union of locus 1 has more than 5632 bins")
    a, b = MU.one_locus_pair(deep[:3000], deep[2000:5632], 1, rng, with_X=False)
    assert merge.merge_host(a, b).n_bins == 5632
    a, b = MU.one_locus_pair(deep, deep[:2], 1, rng, with_X=False)
    refusal(a, b, _lib.SBGPU_ESHAPE, "more than 5632 bins")


@pytest.mark.parametrize("name", ["em_c2_64", "em_edge"])
def test_merged_tables_are_inputs_of_the_unchanged_rule(oracle, golden, name):
    """diff.em_diff_host on the merged batches with the oracle's EM against diff_util.by_hand on the same batches, under
    diff_util.compare's bound: zero-count rows and inherited weights are legal inputs of the rule as it stands."""
    from strawberry_amd import diff
    a, b = pair(golden, name, 2)
    t = merge.merge_host(a, b)
    ma, mb = t.batches()
    assert (ma.count[t.row_a < 0] == 0).all() and (t.row_a < 0).any()
    d = diff.em_diff_host(ma, mb, None, None, oracle.em_batch)
    _, subs = DU.sub_problems(ma, mb, None, None)
    thetas, st, it = DU.solve_each(oracle, subs)
    want = DU.by_hand(ma, mb, None, None, thetas, st, it)
    share, left_out, _, _ = DU.compare(d, want, name)
    assert left_out == 0
    print(name, DU.census(d), "worst share of the bound %.4f" % share)
    assert (d.diff_status == DU.OK).sum() >= 5

"""The device bin grouping (csrc/bins_device.h behind sbgpu_bins_create_device) on its limits: table capacities +-1, the
fractional-mass kernel's bin rounds and run cap, a bin's mass at 2^24 and wrapped past it, the duplicate rule across a
thread's batch and in every kernel that applies it, the prefix scans at their tile, the grids of the small step and the pack
kernel crossed twice, the pair kernels' switches (64 isoforms, 64 bins a round, 32 segments, the third key word), and every
decline.  The cases are tests/bins_util.py's; tests/test_bins_util.py shows on the CPU that each has the property it is there for.

Every case goes through sbgpu_bins_create_device twice: with hit -> bin asked for, and without (the call that launches the
middle kernels before the counts are back and again after a fix-up).  Integers and bit words: every array equals the host
form's (sbgpu_bins_create) and the restatement's, the pair arrays included; a declined input names its reason, and the context
then serves an ordinary batch.

Not covered: the grid-stride loops of the light step (more than 32 768 loci of more than 256 hits) and of the two pair kernels
(more than 65 536 loci, more than 2 x 10^6 isoforms)."""
import numpy as np
import pytest

import bins_util as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.fixture(scope="module")
def words(ctx):
    from strawberry_amd import exonbin as eb
    return lambda annot, hits: eb.compat_and_keys(annot, hits, ctx)


_ORDINARY = {}


def serves_an_ordinary_batch(ctx):
    if not _ORDINARY:
        from strawberry_amd import exonbin as eb
        case = B.ordinary()
        _ORDINARY["case"], _ORDINARY["host"] = case, eb.LocusBins(case.annot, case.hits, case.compat, case.key)
    bd, why = B.group_on_device(ctx, _ORDINARY["case"], want_hit_bin=True)
    assert bd is not None, why
    for x, y in zip(B.bins_arrays(bd), B.bins_arrays(_ORDINARY["host"])):
        np.testing.assert_array_equal(x, y)


def both_calls_agree_or_decline(ctx, case):
    from strawberry_amd import exonbin as eb
    r = B.restate(case.annot, case.hits, case.compat, case.key)
    if case.props:
        case.props(case, r)
    host = eb.LocusBins(case.annot, case.hits, case.compat, case.key) if case.host else None
    for want_hit_bin in (True, False):
        bd, why = B.group_on_device(ctx, case, want_hit_bin)
        if case.decline:
            assert bd is None
            for text in case.decline:
                assert text in why, (text, why)
            serves_an_ordinary_batch(ctx)
            continue
        assert bd is not None, why
        assert bd.n_hits_used == r.n_hits_used
        got = B.bins_arrays(bd)
        if not want_hit_bin:
            assert bd.hit_bin is None
            got[5] = r.hit_bin
        for x, y in zip(got[:6], B.restated_arrays(r)):
            np.testing.assert_array_equal(x, y)
        assert host.n_hits_used == bd.n_hits_used
        for x, y in zip(got, B.bins_arrays(host)):
            np.testing.assert_array_equal(x, y)
    return r, host


@pytest.mark.parametrize("name", sorted(B.SYNTHETIC))
def test_synthetic_words(ctx, name):
    both_calls_agree_or_decline(ctx, B.SYNTHETIC[name]())


@pytest.mark.parametrize("name", sorted(B.GENUINE))
def test_genuine_words(ctx, words, oracle, name):
    case = B.GENUINE[name](words)
    oc, ok = oracle.exonbin_batch(case.annot, case.hits)
    np.testing.assert_array_equal(case.compat, oc)
    np.testing.assert_array_equal(case.key, ok)
    _, host = both_calls_agree_or_decline(ctx, case)
    assert host.n_pairs > 0
    n = np.diff(host.pair_seg_off)
    if name == "pairs_31_segments_apart":      # 32 segments, the 30 inner ones implicit -- from both pair kernels
        assert n.max() == 32 and (host.pair_implicit_mask[n == 32] == 0x7FFFFFFE).sum() >= 20
    if name == "pairs_32_segments_apart":      # 33: a pair without segments
        assert (n == 0).sum() >= 20 and n.max() <= 3


def test_small_loci_past_two_grids(ctx):
    import torch
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    both_calls_agree_or_decline(ctx, B.small_loci_past_two_grids(cus))


def test_the_quantifier_takes_the_host_form_on_a_declined_input(ctx, words):
    from strawberry_amd import exonbin as eb
    from strawberry_amd.quantify import InsertSize, LocusQuantifier
    case = B.unsorted_genuine(words)
    q = LocusQuantifier(case.annot, case.hits, InsertSize(250.0, 30.0), 75, ctx=ctx, device_bins=True)
    b = q.assign_bins()
    assert not q.bins_on_device and not b.grouped_on_device
    host = eb.LocusBins(case.annot, case.hits, case.compat, case.key)
    assert host.n_bins > 20
    for x, y in zip(B.bins_arrays(b), B.bins_arrays(host)):
        np.testing.assert_array_equal(x, y)
    serves_an_ordinary_batch(ctx)

"""The schedule and splicing logic of tests/stream_util.py (what tests/test_front_stream_gpu.py pushes through the chunked record
stream), on the CPU: cut points fall on whole records, every schedule pushes every record exactly once and in order, and
the spliced streams stay in coordinate order."""
import numpy as np
import pytest

import bam_util as B
import e2e_util as U
import exonbin_util as XU
import stream_util as S


def toy_records(which):
    from strawberry_amd import bam
    d = getattr(U, which)
    ordered, _, _, _ = U.load(d)
    _, _, names, _ = XU.e2e_inputs(d, ordered)
    raw, chroms, clusters = B.toy_run_as_bam_records(d, names)
    return raw, bam.index(raw), chroms, clusters


def test_from_cuts_covers_every_record_once():
    assert S.from_cuts(5, []) == [(0, 5)]
    assert S.from_cuts(5, [0, 2, 2, 5]) == [(0, 0), (0, 2), (2, 2), (2, 5), (5, 5)]
    with pytest.raises(AssertionError):
        S.from_cuts(5, [6])


@pytest.mark.parametrize("which", ["E2E", "E2E_CHROMS", "E2E_SINGLE", "E2E_LONGREAD"])
def test_schedules_cut_whole_records_and_cover_every_record_once(which):
    from strawberry_amd import bam
    raw, off, chroms, (c_ref, c_left, c_right, _) = toy_records(which)
    n = off.size - 1
    keys = S.record_keys(raw, off)
    assert (np.diff(keys) >= 0).all() and (keys >> 32).max() == len(chroms) - 1
    first, past = S.cluster_edges(keys, c_ref, c_left, c_right)
    assert (first <= past).all() and (np.diff(past) >= 0).all() and past[-1] == n
    sch = S.schedules(n, first, past, seed=1)
    names = [k for k, _ in sch]
    assert len(set(names)) == len(names) and sum(k.startswith("random") for k in names) == 20
    assert {"one", "each", "starts", "ends", "ends-1", "ends+1", "completes-none", "empty-first-middle-last", "all-then-empty"} <= set(names)
    assert S.schedules(n, first, past, seed=1) == sch and S.schedules(n, first, past, seed=2) != sch     # seeded, deterministic
    for name, pushes in sch:
        S.check_schedule(n, pushes)
        chunk = S.chunk_bytes_for(off, pushes, past)
        for a, b in pushes:
            part = raw[off[a]:off[b]]
            assert part.size <= chunk
            # whole records: the chunk's own index is the caller's offsets, re-based
            np.testing.assert_array_equal(bam.index(part), off[a:b + 1] - off[a], err_msg=name)
    d = dict(sch)
    assert len(d["each"]) == n and d["one"] == [(0, n)]
    assert d["empty-first-middle-last"][0] == (0, 0) and d["empty-first-middle-last"][-1] == (n, n)
    assert sum(a == b for a, b in d["empty-first-middle-last"]) == 3 and d["all-then-empty"] == [(0, n), (n, n)]
    a, b = d["completes-none"][1]
    k = int(np.argmax(past - first))
    assert first[k] < a < b < past[k]


def test_splice_keeps_coordinate_order_and_every_kind():
    raw, off, chroms, (c_ref, c_left, c_right, _) = toy_records("E2E_CHROMS")
    out, o2, kinds = S.splice(raw, c_ref, c_left, c_right, len(chroms), seed=7)
    keys = S.record_keys(out, o2)
    assert (np.diff(keys) >= 0).all()
    assert o2.size - 1 == len(kinds) and sum(k is None for k in kinds) == off.size - 1
    assert {"unmapped-mate", "secondary", "qcfail", "intergenic", "no-cluster-ref", "unmapped-tail"} == set(k for k in kinds if k)
    assert all(k == "unmapped-tail" for k in kinds[-4:])
    # the run's own records, in their order, byte for byte
    own = [i for i, k in enumerate(kinds) if k is None]
    np.testing.assert_array_equal(np.concatenate([out[o2[i]:o2[i + 1]] for i in own]), raw)
    # the intergenic pairs lie between clusters, the no-cluster reference behind every cluster
    for i, k in enumerate(kinds):
        if k == "intergenic":
            ref, pos = keys[i] >> 32, keys[i] & 0xFFFFFFFF
            same = np.asarray(c_ref) == ref
            assert not ((np.asarray(c_left)[same] <= pos + 40) & (pos <= np.asarray(c_right)[same])).any()
        if k == "no-cluster-ref":
            assert keys[i] >> 32 == len(chroms)


def test_chunk_bytes_cover_the_largest_carry():
    off = np.arange(0, 1001, 100, dtype=np.int64) * 1000        # ten records of 100 000 bytes
    past = np.array([3, 7, 10])
    assert S.chunk_bytes_for(off, [(0, 1)], past) == 400_000                # records 3 .. 6 (cluster 1's)
    assert S.chunk_bytes_for(off, [(0, 5)], past) == 500_000                # a push larger than any carry
    acc = np.ones(10, bool)
    acc[3:5] = False                                                         # the records behind cluster 0 are dropped:
    assert S.chunk_bytes_for(off, [(0, 1)], past, acc) == 500_000           # cluster 0 completes at record 5 only
    assert S.chunk_bytes_for(off, [(0, 1)], np.array([3]), acc) == 700_000  # the reads behind the last cluster, carried
    assert S.chunk_bytes_for(off[:2] // 100, [(0, 1)], np.array([1])) == S.MIN_CHUNK

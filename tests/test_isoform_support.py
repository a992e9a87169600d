"""The drop-one isoform support on the host (sbgpu_em_loo_shapes_host / _expand_host / _stat_host, csrc/loo_host.cpp; support.py)
against tests/support_util.py::by_hand: the shapes and the expansion bit for bit on the five EM goldens; the whole host pipeline
with the oracle's EM as the solver, where the same solver on the same bytes makes every integer, theta and heir exact and the
finite statistics differ by the fit's summation only; closed forms; the packed offsets; every refusal."""
import ctypes as C

import numpy as np
import pytest

import fit_util as FU
import support_util as SU
from strawberry_amd import _lib, support

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]


def within_limits(b):
    lim = support.limits()
    idx = np.nonzero((np.diff(b.row_off) <= lim["max_bins"]) & (np.diff(b.iso_off) <= lim["max_iso"]))[0]
    return b if len(idx) == b.n_loci else FU.select_loci(b, idx)


def solve_each(oracle, subs):
    """the oracle's EM on every sub-problem by itself -> thetas, status, iters"""
    res = [oracle.em_locus(n, F) for _, _, _, n, F in subs]
    return [r[0] for r in res], np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32)


def check_pipeline(oracle, b, keep, label):
    t = support.em_loo_host(b, keep, oracle.em_batch)
    _, subs = SU.sub_problems(b, keep)
    thetas, st, it = solve_each(oracle, subs)
    want = SU.by_hand(b, keep, thetas, st, it)
    SU.compare_exact(t, want, label)
    for k in ("heir", "status_without", "iters_without", "status_base", "iters_base"):
        np.testing.assert_array_equal(getattr(t, k), want[k], err_msg="%s %s" % (label, k))
    for k in ("theta_refit", "heir_gain"):
        np.testing.assert_array_equal(getattr(t, k).view(np.uint64), want[k].view(np.uint64), err_msg="%s %s" % (label, k))
    iso_off = np.asarray(b.iso_off)
    for i, w in want["without"].items():
        l = int(np.searchsorted(iso_off, i, side="right") - 1)
        got = t.theta_without(l, i - int(iso_off[l]))
        kept = [j for j in range(int(iso_off[l + 1] - iso_off[l])) if j != i - iso_off[l] and (keep is None or keep[iso_off[l] + j])]
        np.testing.assert_array_equal(got[kept], w, err_msg=label)
        assert np.count_nonzero(got) == np.count_nonzero(w)
    share = SU.compare_stat(t, want, label)
    print(label, SU.census(t), "worst share of the bound %.4f" % share)
    return t, want


@pytest.mark.parametrize("name", GOLDENS)
def test_shapes_and_expansion_are_by_hands_bit_for_bit(golden, name):
    b = within_limits(golden(name)[0])
    rng = np.random.default_rng(7)
    for keep in (None, (rng.random(int(b.iso_off[-1])) < 0.7).astype(np.int32)):
        status, subs = SU.sub_problems(b, keep)
        sh = support.shapes_host(b.row_off, b.iso_off, keep)
        np.testing.assert_array_equal(sh["loo_status"], status)
        np.testing.assert_array_equal(sh["sub_locus"], [s[0] for s in subs])
        np.testing.assert_array_equal(sh["sub_drop"], [s[1] for s in subs])
        want = SU.sub_batch(subs)
        for k in ("row_off", "iso_off", "f_off"):
            np.testing.assert_array_equal(sh[k], getattr(want, k))
        count, F = support.expand_host(b, keep)
        np.testing.assert_array_equal(count, want.count)
        np.testing.assert_array_equal(F.view(np.uint64), np.asarray(want.F).view(np.uint64))
        np.testing.assert_array_equal(support.offsets(b.iso_off, keep), _without_off(b, keep, status))


def _without_off(b, keep, status):
    out = [0]
    iso_off = np.asarray(b.iso_off)
    for l in range(len(iso_off) - 1):
        kept = [keep is None or int(keep[i]) != 0 for i in range(int(iso_off[l]), int(iso_off[l + 1]))]
        K = sum(kept)
        for k in kept:
            out.append(out[-1] + (K - 1 if k and status[l] == 0 and K >= 2 else 0))
    return np.array(out, np.int64)


@pytest.mark.parametrize("name", GOLDENS)
def test_host_pipeline_against_by_hand_on_the_goldens(oracle, golden, name):
    b = within_limits(golden(name)[0])
    t, _ = check_pipeline(oracle, b, None, name)
    assert (t.support == SU.TESTED).sum() > 50


def test_erased_isoforms_on_a_golden(oracle, golden):
    b = within_limits(golden("em_c2_64")[0])
    keep = (np.random.default_rng(3).random(int(b.iso_off[-1])) < 0.6).astype(np.int32)
    t, want = check_pipeline(oracle, b, keep, "em_c2_64 with 40 % erased")
    assert (t.support[keep == 0] == SU.NOT_KEPT).all() and (t.theta_refit[keep == 0] == 0.0).all()
    full = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)[0]
    assert (t.theta_refit[keep != 0] != full[keep != 0]).any()     # the base is the kept columns' own solve, not the unfiltered theta


def test_closed_forms(oracle):
    rng = np.random.default_rng(11)
    col = rng.random(12) + 0.1
    n = rng.integers(1, 50, 12)
    disjoint = np.zeros((9, 3))
    disjoint[:3, 0], disjoint[3:6, 1], disjoint[6:, 2] = 0.5, 0.25, 0.75
    nd = np.arange(1, 10)
    tiny = np.full((5, 2), 0.5)
    tiny[:, 1] = 1e-5
    loci = [(n, np.stack([col, col], 1)),                                       # 0: two identical columns
            (nd, disjoint),                                                     # 1: disjoint isoforms
            (n[:4], col[:4].reshape(4, 1)),                                     # 2: one isoform
            (np.arange(2, 7), tiny),                                            # 3: the other column is all <= 1e-5
            (np.zeros(6, np.int64), rng.random((6, 3)) + 0.1),                  # 4: all-zero counts
            (n[:5], rng.random((5, 4)) + 0.1),                                  # 5: nothing kept (below)
            (n[:6], rng.random((6, 3)) + 0.1)]                                  # 6: an ordinary one behind it
    b = FU.from_loci(loci)
    keep = np.ones(int(b.iso_off[-1]), np.int32)
    keep[int(b.iso_off[5]):int(b.iso_off[6])] = 0
    t, want = check_pipeline(oracle, b, keep, "closed forms")
    sl = lambda l: slice(int(b.iso_off[l]), int(b.iso_off[l + 1]))  # noqa: E731
    assert (np.abs(t.lr_stat[sl(0)]) <= want["bound"][sl(0)]).all() and (t.n_unique[sl(0)] == 0).all()
    assert list(t.heir[sl(0)]) == [1, 0]
    assert list(t.n_unique[sl(1)]) == [int(nd[:3].sum()), int(nd[3:6].sum()), int(nd[6:].sum())] and np.isposinf(t.lr_stat[sl(1)]).all()
    assert list(t.support[sl(2)]) == [SU.SOLE] and np.isposinf(t.lr_stat[sl(2)]).all() and t.n_unique[sl(2)][0] == n[:4].sum()
    assert t.status_without[sl(2)][0] == -1 and t.theta_without(2, 0) is None
    # dropping isoform 0 of locus 3 leaves a matrix without a live row: INIT_EMPTY, and every live fragment is isoform 0's
    assert t.status_without[sl(3)][0] == FU.INIT_EMPTY and t.n_unique[sl(3)][0] == np.arange(2, 7).sum() and np.isposinf(t.lr_stat[sl(3)][0])
    assert t.loo_status[4] == SU.OK and (t.n_unique[sl(4)] == 0).all() and (t.lr_stat[sl(4)] == 0.0).all()
    assert t.loo_status[5] == SU.EMPTY and (t.support[sl(5)] == SU.NOT_KEPT).all() and t.status_base[5] == -1 and t.loglik_base[5] == 0.0
    assert t.loo_status[6] == SU.OK and (t.support[sl(6)] == SU.TESTED).all()
    p = t.p_value()
    assert (p[np.isposinf(t.lr_stat)] == 0.0).all() and (p[t.lr_stat <= 0.0] == 1.0).all()
    fin = np.isfinite(t.lr_stat) & (t.lr_stat > 0)
    from math import erfc, sqrt
    np.testing.assert_allclose(p[fin], [0.5 * erfc(sqrt(x / 2)) for x in t.lr_stat[fin]], rtol=0, atol=0)
    rows = list(t.rows())
    assert len(rows) == int(b.iso_off[-1]) and rows[0][2] == "TESTED" and len(rows[0]) == 11


@pytest.mark.parametrize("K", [64, 65])
def test_64_and_65_kept_isoforms(oracle, K):
    rng = np.random.default_rng(K)
    F = rng.random((70, 66)) * (rng.random((70, 66)) < 0.3)
    b = FU.from_loci([(rng.integers(0, 30, 70), F), (rng.integers(1, 9, 8), rng.random((8, 2)) + 0.1)])
    keep = np.ones(68, np.int32)
    keep[rng.choice(66, 66 - K, replace=False)] = 0
    t, _ = check_pipeline(oracle, b, keep, "K = %d" % K)
    if K == 64:
        assert t.loo_status[0] == SU.OK and (t.support[:66] == SU.TESTED).sum() == 64
    else:
        assert t.loo_status[0] == SU.TOO_WIDE and (t.support[:66] == SU.LOCUS_SKIPPED).sum() == 65 and (t.lr_stat[:66] == 0.0).all()
    assert (t.support[66:] == SU.TESTED).all()      # the neighbour is untouched


def test_the_300_isoform_locus_of_em_edge_with_20_kept(oracle, golden):
    full = golden("em_edge")[0]
    l = int(np.nonzero(np.diff(full.iso_off) == 300)[0][0])
    b = FU.select_loci(full, [l])
    keep = np.zeros(300, np.int32)
    keep[np.random.default_rng(5).choice(300, 20, replace=False)] = 1
    t, _ = check_pipeline(oracle, b, keep, "300 isoforms, 20 kept")
    assert (t.support == SU.TESTED).sum() == 20 and t.loo_status[0] == SU.OK
    assert support.em_loo_host(b, None, oracle.em_batch).loo_status[0] == SU.TOO_WIDE


def test_refusals(oracle):
    L = _lib.load()
    b = FU.from_loci([(np.ones(3, np.int64), np.ones((3, 2)))])
    p = lambda a: np.ascontiguousarray(a).ctypes.data  # noqa: E731
    sizes = (C.c_int64 * 4)()
    bad = np.array([0, -1], np.int64)
    one = np.array([1, 3], np.int64)
    assert L.sbgpu_em_loo_offsets(None, None, 1, None) == -1 and b"null" in L.sbgpu_last_error()
    out = np.zeros(4, np.int64)
    assert L.sbgpu_em_loo_offsets(p(bad), None, 1, p(out)) == -1 and b"ascend" in L.sbgpu_last_error()
    assert L.sbgpu_em_loo_offsets(p(one), None, 1, p(out)) == -1 and b"begin at 0" in L.sbgpu_last_error()
    assert L.sbgpu_em_loo_offsets(p(b.iso_off), None, -1, p(out)) == -1
    assert L.sbgpu_em_loo_shapes_host(1, None, p(b.iso_off), None, sizes, *([None] * 6)) == -1
    assert L.sbgpu_em_loo_shapes_host(1, p(b.row_off), p(b.iso_off), None, None, *([None] * 6)) == -1
    assert L.sbgpu_em_loo_shapes_host(1, p(bad), p(b.iso_off), None, sizes, *([None] * 6)) == -1
    lim = support.limits()
    deep, wide = np.array([0, lim["max_bins"] + 1], np.int64), np.array([0, lim["max_iso"] + 1], np.int64)
    assert L.sbgpu_em_loo_shapes_host(1, p(deep), p(b.iso_off), None, sizes, *([None] * 6)) == -5 and b"5632 bins" in L.sbgpu_last_error()
    assert L.sbgpu_em_loo_shapes_host(1, p(b.row_off), p(wide), None, sizes, *([None] * 6)) == -5 and b"4096 isoforms" in L.sbgpu_last_error()
    assert L.sbgpu_em_loo_shapes_host(1, p(np.array([0, lim["max_bins"]], np.int64)), p(b.iso_off), None, sizes, *([None] * 6)) == 0
    assert list(sizes) == [3, 3 * lim["max_bins"], 4, 4 * lim["max_bins"]]
    cnt, F = np.zeros(16, np.int32), np.zeros(16)
    bt = _lib.sbgpu_batch_t(1, p(b.row_off), p(b.iso_off), p(b.f_off), p(b.count), p(b.F))
    assert L.sbgpu_em_loo_expand_host(None, None, p(cnt), p(F)) == -1
    assert L.sbgpu_em_loo_expand_host(C.byref(bt), None, None, p(F)) == -1 and b"sub_count" in L.sbgpu_last_error()
    neg = np.array([1, -1, 1], np.int32)
    bn = _lib.sbgpu_batch_t(1, p(b.row_off), p(b.iso_off), p(b.f_off), p(neg), p(b.F))
    assert L.sbgpu_em_loo_expand_host(C.byref(bn), None, p(cnt), p(F)) == -1 and b"negative" in L.sbgpu_last_error()
    bf = _lib.sbgpu_batch_t(1, p(b.row_off), p(b.iso_off), p(np.array([0, 5], np.int64)), p(b.count), p(b.F))
    assert L.sbgpu_em_loo_expand_host(C.byref(bf), None, p(cnt), p(F)) == -1 and b"rows x isoforms" in L.sbgpu_last_error()
    s = _lib.sbgpu_em_loo_t()
    z8, z4, zi = np.zeros(8), np.zeros(8, np.int32), np.zeros(8, np.int64)
    good = (p(z8), p(z4), p(z4), p(z8), p(zi), p(zi), p(zi))
    assert L.sbgpu_em_loo_stat_host(1, p(b.iso_off), None, *good, None) == -1
    assert L.sbgpu_em_loo_stat_host(1, p(b.iso_off), None, None, *good[1:], C.byref(s)) == -1 and b"null array" in L.sbgpu_last_error()
    s.theta_without = p(z8)
    assert L.sbgpu_em_loo_stat_host(1, p(b.iso_off), None, *good, C.byref(s)) == -1 and b"without_off" in L.sbgpu_last_error()
    wrong = np.array([0, 2, 3], np.int64)
    s.without_off = p(wrong)
    assert L.sbgpu_em_loo_stat_host(1, p(b.iso_off), None, *good, C.byref(s)) == -1 and b"sbgpu_em_loo_offsets" in L.sbgpu_last_error()
    s.without_off = p(support.offsets(b.iso_off))
    assert L.sbgpu_em_loo_stat_host(1, p(b.iso_off), None, *good, C.byref(s)) == 0
    np.testing.assert_array_equal(support.offsets(b.iso_off), [0, 1, 2])
    np.testing.assert_array_equal(support.offsets(b.iso_off, [1, 0]), [0, 0, 0])
    with pytest.raises(ValueError):
        support.offsets(b.iso_off, [1])
    with pytest.raises(ValueError):
        support.IsoformSupport(b.iso_off, want=("nonsense",))

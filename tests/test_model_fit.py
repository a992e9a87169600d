"""The model fit on the host: sbgpu_em_fit_host (csrc/fit_host.cpp), the CPU statement of what the device form computes, against
tests/fit_util.py::by_hand -- the rule of include/sbgpu.h restated with Python floats and plain loops -- under the bounds at the
head of fit_util.py (DESIGN 3.22 derives them); the reference's stopping rule seen through step_norm; the identities the rule
implies; hand-made loci with closed forms; the refusals.

No GPU here: theta / status are the oracle's, and the edge sample's bins and weights come from the oracle's restatement, as in
tests/test_isoform_coverage.py (sbgpu_quantify_host needs a device)."""
import ctypes as C
import types

import numpy as np
import pytest

import fit_util as FU
import retained_util as R
from strawberry_amd import _lib, fit
from strawberry_amd import exonbin as eb
from test_oracle import KATS

GOLDENS = ["em_random_256", "em_edge", "em_c2_64", "em_c3_400", "em_c4_assembled"]
U = FU.U


@pytest.fixture(scope="module")
def G(oracle, golden):
    """name -> (batch, the oracle's theta, status, iters, by_hand's dict): computed once"""
    out = {}
    for name in GOLDENS:
        b, _, _ = golden(name)
        theta, status, iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
        out[name] = (b, theta, status, iters, FU.by_hand(b, theta, None, status))
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_host_form_against_by_hand_on_the_goldens(G, name):
    b, theta, status, _, want = G[name]
    t = fit.em_fit_host(b, theta, status=status)
    share = FU.compare(t, want, b, True, name)
    print(name, "worst share of each bound:", share)
    np.testing.assert_array_equal(t.worst_bin, FU.worst_bin_of(t.resid, want["possible"], b.row_off))
    assert (t.n_live + t.n_dropped == np.add.reduceat(np.concatenate([b.count, [0]]), b.row_off[:-1]) * (np.diff(b.row_off) > 0)).all()
    # asked for alone, an array is the same; the others are not filled
    few = fit.em_fit_host(b, theta, status=status, want=("score", "dof"))
    assert few.expected is None and few.loglik is None
    np.testing.assert_array_equal(few.score, t.score)
    np.testing.assert_array_equal(few.dof, t.dof)
    rows = list(t.rows(theta=theta))
    assert len(rows) == b.n_loci and rows[0][0] == 0 and rows[-1][6] == t.pearson[-1] and len(rows[0]) == 11
    chi2 = t.reduced_chi2()
    ok = t.dof > 0
    np.testing.assert_array_equal(chi2[ok], t.pearson[ok] / t.dof[ok])
    assert np.isnan(chi2[~ok]).all()


@pytest.fixture(scope="module")
def S(oracle):
    from test_context_table import oracle_weights
    annot, hits = R.edge_sample(200, oracle=oracle)
    compat, key = oracle.exonbin_batch(annot, hits)
    bins = eb.LocusBins(annot, hits, compat, key)
    F = oracle_weights(oracle, bins, oracle.make_insert(*R.LAW), False)
    theta, status, _ = oracle.em_batch(bins.row_off, bins.iso_off, bins.f_off, bins.count, F)
    ab = oracle.abundance(bins.iso_off, theta, status, bins.iso_len, hits.n_hits, min_isoform_frac=R.MIN_ISOFORM_FRAC)
    batch = types.SimpleNamespace(row_off=bins.row_off, iso_off=bins.iso_off, f_off=bins.f_off, count=bins.count, F=F, n_loci=annot.n_loci)
    return batch, theta, np.asarray(ab["keep"], np.int32), status


def test_host_form_against_by_hand_on_the_edge_sample(S):
    batch, theta, keep, status = S
    want = FU.by_hand(batch, theta, keep, status)
    t = fit.em_fit_host(batch, theta, keep, status)
    print("edge sample, worst share of each bound:", FU.compare(t, want, batch, True, "edge sample"))
    # the sample holds what the rule distinguishes: dropped rows, an erased isoform, a locus that never started
    assert t.n_dropped.sum() > 0 and (keep == 0).any() and (np.asarray(status) == FU.INIT_EMPTY).any()
    empty = np.asarray(status) == FU.INIT_EMPTY
    assert (t.dof[empty] == 0).all() and (t.worst_bin[empty] == -1).all() and (t.n_live[empty] == 0).all()


@pytest.mark.parametrize("name", GOLDENS)
def test_the_reference_stopping_rule_seen_from_outside(G, name):
    """Every locus the reference stopped by its rule (status OK, at least 2 iterations) stands less than
    SBGPU_EM_THETA_CHANGE_LIMIT from its own next iterate."""
    b, theta, status, iters, want = G[name]
    t = fit.em_fit_host(b, theta, status=status)
    norm = t.step_norm(theta)
    rows, niso, _, _ = FU.shapes(b)
    ruled = (np.asarray(status) == 0) & (np.asarray(iters) >= 2)
    near = np.abs(want["step_norm"] - FU.THETA_CHANGE_LIMIT) <= (rows + niso + 16) * U * want["n_live"]
    left_out = ruled & near
    assert left_out.sum() <= 0.02 * b.n_loci, (name, int(left_out.sum()))
    check = ruled & ~near
    assert check.any() and (norm[check] < FU.THETA_CHANGE_LIMIT).all(), (name, float(norm[check].max()))
    capped = np.asarray(status) == 3
    print(name, "loci checked %d, left out %d, largest norm %.3e; MAXITER loci %d, their norms up to %.3e"
          % (check.sum(), left_out.sum(), norm[check].max(), capped.sum(), norm[capped].max() if capped.any() else 0.0))


@pytest.mark.parametrize("name", GOLDENS)
def test_identities_within_rounding(G, name):
    b, theta, status, _, want = G[name]
    t = fit.em_fit_host(b, theta, status=status)
    rows, niso, bin_locus, iso_locus = FU.shapes(b)
    M = (t.n_live - t.n_impossible).astype(np.float64)
    sum_e = np.bincount(bin_locus, weights=t.expected, minlength=b.n_loci)
    assert (np.abs(sum_e - M) <= (2 * (rows + 8) + 4) * U * M).all()
    # the M-step conserves the fragments it was given: sum_j theta_j score_j = M
    sum_ts = np.bincount(iso_locus, weights=theta[:len(iso_locus)] * t.score, minlength=b.n_loci)
    err = np.abs(sum_ts - M)
    assert (err <= (rows + 8 + 2 * (niso + 8) + 8) * U * M).all(), float((err / np.maximum(M, 1)).max())
    # a deviance is not negative, beyond its own rounding
    bound = (rows + FU.K) * U * want["abs_deviance"] + 2.0 * want["n_live"] * (rows + 12) * U
    assert (t.deviance >= -bound).all()
    print(name, "sum theta score = M within %.2e relative" % float((err / np.maximum(M, 1)).max()))


def kat(name):
    _, n, F, status, theta = next(k for k in KATS if k[0] == name)
    return FU.from_loci([(n, F)]), np.asarray(theta, np.float64), np.asarray([status], np.int32)


def test_closed_form_one_isoform():
    b, theta, status = kat("single_iso")
    t = fit.em_fit_host(b, theta, status=status)
    c = 0.2 + 0.05
    np.testing.assert_allclose(t.expected, [30 * 0.2 / c, 30 * 0.05 / c], rtol=8 * U)
    np.testing.assert_allclose(t.score, [30 / theta[0]], rtol=8 * U)
    assert t.n_live[0] == 30 and t.n_dropped[0] == 0 and t.n_impossible[0] == 0 and t.dof[0] == 1


def test_closed_form_disjoint_bins():
    """Every bin is one isoform's alone and theta_j = n_j: the model reproduces the counts."""
    n = [3, 11, 7, 20]
    F = np.diag([0.3, 0.07, 0.5, 0.011])
    b = FU.from_loci([(n, F)])
    t = fit.em_fit_host(b, np.asarray(n, np.float64))
    rows, n_live, r_e = 4, float(sum(n)), (4 + 12) * U
    assert t.dof[0] == 0 and t.n_live[0] == sum(n)
    assert abs(t.deviance[0]) <= 4.0 * n_live * r_e * (1.0 + (rows + FU.K) * U)
    assert 0.0 <= t.pearson[0] <= n_live * (r_e + 6 * U) ** 2 * (1.0 + (rows + 8) * U)
    np.testing.assert_allclose(t.score, 1.0, rtol=8 * U)
    np.testing.assert_allclose(t.expected, n, rtol=r_e)


@pytest.mark.parametrize("name", ["toy", "zero_col", "row_dropped", "denom_zero", "all_dropped", "single_row"])
def test_known_answer_loci(oracle, name):
    b, _, _ = kat(name)
    theta, status, _ = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F)
    t = fit.em_fit_host(b, theta, status=status)
    want = FU.by_hand(b, theta, None, status)
    FU.compare(t, want, b, True, name)
    if name == "row_dropped":
        assert t.n_dropped[0] == 7 and t.n_live[0] == 30
    if name == "zero_col":
        assert t.score[2] == 0.0 and t.score[0] > 0.0
    if name == "all_dropped":
        assert status[0] == FU.INIT_EMPTY and t.n_dropped[0] == 7 and t.n_live[0] == 0 and t.dof[0] == 0 and t.worst_bin[0] == -1
        assert not t.expected.any() and not t.resid.any() and not t.score.any() and t.loglik[0] == t.deviance[0] == t.pearson[0] == 0.0
    if name == "denom_zero":
        np.testing.assert_array_equal(theta, [2.5, 2.5])
        assert t.n_impossible[0] == want["n_impossible"][0] and t.n_impossible[0] in (0, 5)
    if name in ("toy", "zero_col", "row_dropped", "single_row"):
        assert status[0] == 0 and t.step_norm(theta)[0] < FU.THETA_CHANGE_LIMIT


def test_an_erased_isoform_that_was_a_bins_only_carrier():
    b = FU.from_loci([([5, 6, 7], [[.2, 0], [.1, .1], [0, .3]])])
    theta = np.array([11.0, 7.0])
    t = fit.em_fit_host(b, theta, keep=[1, 0])
    assert t.n_impossible[0] == 7 and t.n_live[0] == 18 and t.n_dropped[0] == 0
    assert t.expected[2] == 0.0 and t.resid[2] == 0.0 and t.score[1] == 0.0
    np.testing.assert_allclose(t.expected[:2].sum(), 11.0, rtol=8 * U)
    np.testing.assert_allclose(t.expected[:2], [11 * .2 / .3, 11 * .1 / .3], rtol=16 * U)
    assert t.dof[0] == 1 and t.worst_bin[0] in (0, 1)
    FU.compare(t, FU.by_hand(b, theta, [1, 0]), b, True, "erased")
    # with everything kept the bin is possible again
    assert fit.em_fit_host(b, theta).n_impossible[0] == 0


def test_a_tie_goes_to_the_lowest_index():
    b = FU.from_loci([([5, 8, 2, 8, 2], [[.2]] * 5)])
    t = fit.em_fit_host(b, [25.0])
    assert abs(t.resid[1]) == abs(t.resid[2]) == abs(t.resid[3]) == abs(t.resid[4]) > abs(t.resid[0])
    assert t.worst_bin[0] == 1


def raw_host(batch_struct, theta, out=None):
    L = _lib.load()
    s = out if out is not None else _lib.sbgpu_em_fit_t()
    rc = L.sbgpu_em_fit_host(C.byref(batch_struct) if batch_struct is not None else None, theta, None, None, C.byref(s))
    return rc, L.sbgpu_last_error().decode()


def test_every_refusal_with_its_text():
    L = _lib.load()
    row_off, iso_off, f_off = (np.array(a, np.int64) for a in ([0, 2], [0, 1], [0, 2]))
    count, F, theta = np.array([1, 2], np.int32), np.array([.2, .1]), np.array([3.0])

    def struct(row_off=row_off, iso_off=iso_off, f_off=f_off, count=count, F=F, n=1):
        return _lib.sbgpu_batch_t(n, row_off.ctypes.data, iso_off.ctypes.data, f_off.ctypes.data, None if count is None else count.ctypes.data,
                                  None if F is None else F.ctypes.data)
    assert raw_host(struct(), theta.ctypes.data)[0] == _lib.SBGPU_OK
    for bad, text in ((dict(count=np.array([1, -2], np.int32)), "a negative count"),
                      (dict(row_off=np.array([1, 2], np.int64)), "must begin at 0"),
                      (dict(row_off=np.array([0, -1], np.int64)), "do not ascend"),
                      (dict(f_off=np.array([0, 3], np.int64)), "is not rows x isoforms"),
                      (dict(count=None), "null count or F"),
                      (dict(n=-1), "bad n_loci")):
        rc, msg = raw_host(struct(**bad), theta.ctypes.data)
        assert rc == _lib.SBGPU_EINVAL and text in msg and msg.startswith("sbgpu_em_fit_host:"), (bad, rc, msg)
    rc, msg = raw_host(struct(), None)
    assert rc == _lib.SBGPU_EINVAL and "theta is needed" in msg
    rc, msg = raw_host(None, theta.ctypes.data)
    assert rc == _lib.SBGPU_EINVAL and "null argument" in msg
    assert L.sbgpu_em_fit_limits(None) == _lib.SBGPU_EINVAL
    with pytest.raises(_lib.SbgpuError, match="a negative count"):
        fit.em_fit_host(types.SimpleNamespace(row_off=row_off, iso_off=iso_off, f_off=f_off, count=[1, -2], F=F), theta)
    with pytest.raises(ValueError, match="theta holds 0 entries"):
        fit.em_fit_host(types.SimpleNamespace(row_off=row_off, iso_off=iso_off, f_off=f_off, count=count, F=F), [])
    with pytest.raises(ValueError, match="unknown arrays"):
        fit.ModelFit(row_off, iso_off, want=("chi2",))
    lim = fit.limits()
    assert lim["max_bins"] == 5632 and lim["max_iso"] == 4096 and lim["wave_vals"] < lim["stage_vals"] and lim["threads"] == lim["wave_loci"] * lim["wave"]

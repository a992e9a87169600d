"""tests/vb_util.py on its own (CPU, no library): the restatement's digamma against closed forms and -- where importable --
mpmath and scipy; the evidence bound non-decreasing in the iteration; the rule's edge cases as the restatement states them; and
what the samples must hold for the tests on them (tests/test_vb_cpp.py, tests/test_vb_gpu.py) to mean something."""
import math

import numpy as np
import pytest

import vb_util as V

EULER = 0.5772156649015328606


def psi_grid():
    return np.concatenate([np.logspace(-6, 9, 601), np.arange(1, 40) / 4.0, [9.999999, 10.0, 19.999999, 20.0, 1e-6 + 0.0025]])


def test_digamma_against_closed_forms():
    assert abs(V.digamma(1.0)[0] + EULER) < 2e-15
    assert abs(V.digamma(0.5)[0] + EULER + 2.0 * math.log(2.0)) < 4e-15
    h = 0.0
    for n in range(1, 60):               # psi(n + 1) = H_n - gamma
        h += 1.0 / n
        assert abs(V.digamma(n + 1.0)[0] - (h - EULER)) <= 4e-15 * max(1.0, h), n
    x = psi_grid()
    assert (np.abs(V.digamma(x + 1.0) - (V.digamma(x) + 1.0 / x)) <= 4e-15 * np.maximum(1.0, np.abs(V.digamma(x)))).all()


def test_digamma_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    x = psi_grid()
    want = np.array([float(mp.digamma(mp.mpf(float(v)))) for v in x])
    err = np.abs(V.digamma(x) - want) / np.maximum(1.0, np.abs(want))
    print("the restatement's digamma against mpmath at 40 digits: %.2e relative to max(1, |psi|)" % err.max())
    assert err.max() <= 2e-15


def test_digamma_against_scipy():
    sp = pytest.importorskip("scipy.special")
    x = psi_grid()
    want = sp.digamma(x)
    assert (np.abs(V.digamma(x) - want) / np.maximum(1.0, np.abs(want))).max() <= 4e-15


@pytest.mark.parametrize("alpha", [0.01, 0.5, 1.0])
def test_the_evidence_bound_does_not_decrease(alpha):
    rng = np.random.default_rng(5)
    for shape in ((9, 4), (30, 7), (12, 12), (3, 2)):
        n, F = V.shaped(rng, *shape, depth=400)
        e = [V.solve_locus(n, F, alpha, change_limit=1e-300, max_iter=k)["elbo"] for k in range(1, 9)]
        assert all(b >= a - 1e-9 * max(1.0, abs(a)) for a, b in zip(e, e[1:])), (shape, e)
        assert e[-1] > e[0] or shape == (3, 2)      # (two bins, one of them dropped: nothing to learn)


def test_the_edge_cases():
    r = V.solve_locus(*V.init_empty())
    assert r["status"] == V.INIT_EMPTY and r["iters"] == 0 and r["n_active"] == 0 and r["n_frag"] == 0 and not r["count"].any() and r["elbo"] == 0.0
    r = V.solve_locus(*V.no_fragments())
    assert r["status"] == V.OK and r["iters"] == 1 and r["n_frag"] == 0 and r["n_active"] == 2 and r["elbo"] == 0.0
    assert not r["count"].any() and not r["share"].any() and not r["share_sd"].any()
    r = V.solve_locus(*V.inactive_columns())
    assert r["status"] == V.OK and r["n_active"] == 2 and r["n_frag"] == 51 and (r["count"] > 0).tolist() == [True, False, True, False]
    assert abs(r["count"].sum() - 51) < 1e-9 and abs(r["share"].sum() - 1.0) < 1e-12 and (r["share_sd"][[1, 3]] == 0).all()
    r = V.solve_locus(*V.dying_private_bin(), **V.DYING_PARAMS)
    assert r["status"] == V.OK and r["count"][1] == 0.0 and r["count"][0] == 100003.0 and np.isfinite(r["elbo"])
    assert not np.isnan(np.concatenate([r["count"], r["share"], r["share_sd"]])).any() and r["share"][1] > 0.0
    r = V.solve_locus(*V.underflowing_bin(), **V.UNDERFLOW_PARAMS)
    assert r["status"] == V.DENOM_ZERO and r["iters"] == 2 and r["elbo"] == -math.inf
    np.testing.assert_allclose(r["count"][:400], 1.0 / 400, rtol=1e-12)
    r = V.solve_locus(*V.fast_locus(), max_iter=3)
    assert r["status"] == V.OK and r["iters"] == 2 and r["count"].tolist() == [40.0, 60.0]
    n, F = V.shaped(np.random.default_rng(2), 30, 7, depth=400)
    r = V.solve_locus(n, F, max_iter=3)
    assert r["status"] == V.MAXITER and r["iters"] == 3


def test_the_slow_and_the_fast_locus_are_what_the_position_test_needs():
    n, F = V.slow_locus(np.random.default_rng(31))
    r = V.solve_locus(n, F, trace=True)
    assert r["status"] == V.OK and 300 <= r["iters"] < V.MAX_ITER, r["iters"]
    assert 300 <= V.solve_locus(n, F, 1.0)["iters"] < V.MAX_ITER
    assert V.solve_locus(*V.fast_locus())["iters"] == 2


def test_alpha_below_one_empties_what_the_data_do_not_need():
    """Isoform 1 shares its one counted bin with isoform 0 and owns a bin without fragments; isoform 2 stands apart.  alpha =
    0.01 empties isoform 1; the flat prior leaves it more than a fragment"""
    n, F = [50, 0, 50], [[0.2, 0.2, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.3]]
    sparse = V.solve_locus(n, F, 0.01, change_limit=1e-9, max_iter=5000)
    flat = V.solve_locus(n, F, 1.0, change_limit=1e-9, max_iter=5000)
    assert sparse["count"][1] < 1e-3 and abs(sparse["count"][0] - 50) < 1e-2
    assert flat["count"][1] > 1.0

"""GPU parity of the tile kernels' column-lane exchange (em_device.h: col_lanes_scatter): loci of 9-64 isoforms, which
the plan gives 2, 4 or 8 column lanes of 5-8 columns (plan.h::layout_for), hold their rows in a per-column-lane order
and reduce-scatter their row denominators over the column lanes.  Rows without reads, dropped rows, and zero
denominators -- at the first iteration and late, after the column normalisation, in a row a non-zero column lane owns
-- against the oracle: status and iteration counts exact, theta within 1e-9 relative."""
import numpy as np
import pytest

from test_em_gpu import needs_experiments

pytestmark = pytest.mark.gpu

THETA_RTOL = 1e-9
THETA_FLOOR = 1e-9

# (isoforms, layout): CPL x CL with CPL = 5..8 on each of CL = 2, 4, 8 -- the row count per row lane of the tile is 6
# for 5-6 columns per lane and 4 for 7-8 (rh 2; 3 / 2 at rh 1, 12 / 8 at rh 4)
WIDTHS = [9, 12, 13, 16, 17, 22, 27, 32, 33, 45, 50, 64]


def theta_err(theta, ref):
    return np.abs(theta - ref) / np.maximum(np.abs(ref), THETA_FLOOR)


def _random_locus(rng, nrow, niso):
    F = np.where(rng.random((nrow, niso)) < 0.5, rng.uniform(1e-3, .3, (nrow, niso)), 0.0)
    F[rng.random(nrow) < 0.15] = 0.0                 # dropped rows: no weight above 1e-5
    F[rng.random(nrow) < 0.1] *= 1e-6                # dropped too, with non-zero weights
    cnt = rng.integers(1, 50, nrow)
    cnt[rng.random(nrow) < 0.3] = 0                  # kept rows without reads
    return cnt.astype(np.int32), F


def _zero_count_locus(rng, nrow, niso):
    # every count zero: theta0 = 0, every kept row's denominator is zero at the first iteration (estimate.cpp:451)
    _, F = _random_locus(rng, nrow, niso)
    F[0, :] = 0.2                                    # at least one kept row
    return np.zeros(nrow, np.int32), F


def _decaying_locus(niso, decay_rows, b_col, extra_rows):
    # test_em_gpu.py's tiny denominators, widened: isoform B (column b_col, in the last column lane) loses its reads to
    # A and decays until its theta flushes to zero -- then the rows that fit only B have a zero denominator -- while two
    # nearly equal isoforms C, D keep the EM running; every other isoform has rows of its own
    a, c, d = 0, 1, 2
    rows, cnt = [], []

    def row(w, n):
        r = np.zeros(niso)
        for j, v in w.items():
            r[j] = v
        rows.append(r)
        cnt.append(n)
    row({a: 1.0, b_col: 0.5}, 100)
    row({a: 1.0}, 100)
    for _ in range(decay_rows):
        row({b_col: 1.0}, 0)
    for k in range(6):
        x = 0.5 + 0.05 * k
        row({c: x, d: x * (1 + 1e-3 * (k - 2.5))}, 50 + k)
    for j in range(niso):
        if j not in (a, b_col, c, d):
            for e in range(extra_rows):
                row({j: 1.0, (j + 1 + e) % niso if (j + 1 + e) % niso not in (a, b_col, c, d) else j: 0.25}, 20 + e)
    return np.array(cnt, np.int32), np.array(rows)


def _batch(niso, seed):
    from strawberry_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    loci = []
    # row counts for one to many row lanes per group, and past the wave form's rows into the block forms
    for nrow in (3, 7, 20, 41, 90, 260):
        for _ in range(3):
            loci.append(_random_locus(rng, nrow, niso))
    loci.append(_zero_count_locus(rng, 12, niso))
    loci.append(_zero_count_locus(rng, 70, niso))
    for decay_rows, extra in ((2, 1), (5, 1), (11, 2)):
        loci.append(_decaying_locus(niso, decay_rows, niso - 1, extra))
    return synth.from_loci(loci)


def _check(ctx, oracle, niso):
    from strawberry_amd import em
    b = _batch(niso, 1000 + niso)
    s = em.EmBatchSolver(b, ctx)
    s.run_em()
    r = s.results()
    o_theta, o_status, o_iters = oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=2)
    # the batch holds what it is meant to: zero denominators at the first iteration and late ones
    assert (o_status[-5:-3] == 2).all() and (o_iters[-5:-3] == 1).all()
    assert (o_status[-3:] == 2).all() and o_iters[-3:].min() > 200
    np.testing.assert_array_equal(r["status"], o_status)
    np.testing.assert_array_equal(r["iters"], o_iters)
    err = theta_err(r["theta"], o_theta)
    assert err.max() < THETA_RTOL, (niso, err.max(), int(err.argmax()))


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.mark.parametrize("niso", WIDTHS)
def test_column_lane_exchange_against_oracle(ctx, oracle, niso):
    _check(ctx, oracle, niso)


@pytest.mark.parametrize("rmult", ["1", "4"])
@needs_experiments
def test_column_lane_exchange_every_tile_height(oracle, monkeypatch, rmult):
    """The wave kind's half and double tiles: 3 / 2 and 12 / 8 rows per row lane (3: no even split, the plain
    all-reduce; 12 and 8 split over two and three column-lane bits)."""
    from strawberry_amd import em
    monkeypatch.setenv("SBGPU_WAVE_RMULT", rmult)
    ctx = em.default_context(0)
    for niso in (9, 16, 17, 32, 33, 64):
        _check(ctx, oracle, niso)

"""GPU parity of the block form's row-lane reduce-scatter (em_device.h: row_lanes_scatter; the index math: em_row_scatter.h).
The fp64 block kernel holds a lane's columns in S = 6 or 8 slots -- the classes of 5 and 7 columns per lane run the 6- and 8-slot
instantiations -- in a slot order that depends on the lane, and sums the M-step's column partials over the row lanes by an
exchange that halves the live slots per step.  Every instantiation (S in {6, 8}) x (CL in {1, 2, 4, 8} column lanes) at the first
and last row count of its lowest and highest RU (rows used per row lane), at each the isoform counts at both ends of the
layouts it serves and the counts that leave the last column lane partly and entirely without a column; the tall kind (which
keeps the all-reduce) at its first row count; the per-locus events inside loci with RU < R; the split entry twice and the bias
entry -- against the oracle: status and iteration counts exact, theta within 1e-9 relative, every locus compared.  The batches
come from test_em_block_rows_gpu.py's helpers."""
import numpy as np
import pytest

import test_em_block_rows_gpu as rows

pytestmark = pytest.mark.gpu

KIND_BLOCK_TALL = 4     # plan.h: ClassKind::kBlockTall

# (S, CL) -> isoform counts: both ends of the classes the instantiation serves (S = 6: 5 and 6 columns per lane, S = 8: 7 and
# 8), and counts whose last column lane is partly empty (9: 3 of 6; 19: 1 of 6; 13: 5 of 8; 25: 1 of 8) or entirely empty
# (17: lane 3 of 4; 33: lanes 6 and 7 of 8, lane 5 half; 41 and 49: lane 7)
ISOFORMS = {
    (6, 1): [5, 6], (6, 2): [9, 12], (6, 4): [17, 19, 24], (6, 8): [33, 41, 48],
    (8, 1): [7, 8], (8, 2): [13, 16], (8, 4): [25, 32], (8, 8): [49, 64],
}


def row_counts(S, CL):
    """First and last row count of the lowest (2) and the highest (R) RU.  The tile is R = 6 rows for 6 slots and 4 for 8; below
    64 / CL * R + 1 rows the wave kind holds the locus, so that is where RU 2 starts when it is above 256 / CL + 1."""
    gr, R = 256 // CL, (6 if S == 6 else 4)
    return [max(gr + 1, 64 // CL * R + 1), 2 * gr, (R - 1) * gr + 1, R * gr]


CASES = [(S, CL, niso, nrow) for (S, CL), isos in ISOFORMS.items() for niso in isos for nrow in row_counts(S, CL)]
# (niso, nrow) -> seed offset, for a case whose seed puts a locus so close to the threshold that the oracle's own iteration
# count moves under a one-ulp change of F.  Checked on the CPU -- every batch of this file solved by the oracle with each weight
# moved to a neighbouring double at random, four times: no count moved, no seed replaced.
SEED_BUMP = {}


def shape_batch(niso, nrow):
    from strawberry_amd import synth
    rng = np.random.Generator(np.random.PCG64(niso * 100000 + nrow + 31 + SEED_BUMP.get((niso, nrow), 0)))
    return synth.from_loci([rows.random_locus(rng, nrow, niso) for _ in range(rows.LOCI_PER_SHAPE)])


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


@pytest.mark.parametrize("S,CL,niso,nrow", CASES)
def test_block_scatter_every_instantiation(ctx, oracle, S, CL, niso, nrow):
    cpl = -(-niso // CL)
    assert rows.column_lanes(niso) == CL and cpl + (cpl & 1) == S and rows.tile_rows(niso) == (6 if S == 6 else 4)
    assert rows.rows_used(niso, nrow) in (2, rows.tile_rows(niso))
    rows.solve_and_compare(ctx, oracle, shape_batch(niso, nrow))      # (asserts that the plan's kind is the block kind)


# ---------------------------------------------------------------- the tall kind: the first row count past the base tile
TALL_CASES = [(8, 1025), (22, 385)]      # 8 x 1, R 4 of 256 row lanes; 6 x 4, R 6 of 64 row lanes


@pytest.mark.parametrize("niso,nrow", TALL_CASES)
def test_block_scatter_tall_kind(ctx, oracle, niso, nrow):
    from strawberry_amd import em
    b = shape_batch(niso, nrow)
    s = em.EmBatchSolver(b, ctx)
    assert (s.plan.locus_kinds() == KIND_BLOCK_TALL).all(), s.plan.locus_kinds()
    s.run_em()
    rows.compare(s.results(), oracle.em_batch(b.row_off, b.iso_off, b.f_off, b.count, b.F, threads=2))


# ---------------------------------------------------------------- per-locus events, in loci with RU < R
# (isoforms, rows): 5 x 2 on the 6-slot instantiation, R 6, RU 3; 8 x 2 (the layout that bounds the benchmark), R 4, RU 3
EVENT_LAYOUTS = [(9, 300), (16, 300)]


@pytest.mark.parametrize("niso,nrow", EVENT_LAYOUTS)
def test_block_scatter_events(ctx, oracle, niso, nrow):
    """test_em_block_rows_gpu.py's event batch and its assertions, at these layouts: rows the 1e-5 filter drops, a zero
    denominator early and late, an underflowing denominator product (the exact re-run's column sums go through the exchange
    too), init-empty, the 1 000-iteration cap."""
    rows.test_block_rows_events(ctx, oracle, niso, nrow)


# ---------------------------------------------------------------- schedules
def mixed_batch():
    """Every (S, CL) instantiation through both classes it serves, at a few row counts, all block-form."""
    from strawberry_amd import synth
    rng = np.random.Generator(np.random.PCG64(1299))
    loci = []
    for (S, CL), isos in ISOFORMS.items():
        for k, niso in enumerate(isos):
            loci.append(rows.random_locus(rng, row_counts(S, CL)[(k + CL) % 4], niso))
    return synth.from_loci(loci)


def test_block_scatter_split_entry_twice(ctx, oracle):
    """The split entry (what a pipelined bench step uses), two steps back to back: each step's outputs are the unsplit run's,
    byte for byte, and the unsplit run's are the oracle's."""
    import torch
    from strawberry_amd import dist, em
    b = mixed_batch()
    _, want, _ = rows.solve_and_compare(ctx, oracle, b)
    s = em.EmBatchSolver(b, ctx)
    q = dist.ShardQuantifier(s, 10 ** 7, pipelined=True)
    assert q.pipelined
    snaps = []

    def observe():
        snaps.append({k: getattr(s, "d_" + k)[:n].clone() for k, n in (("theta", s.n_iso), ("status", b.n_loci),
                                                                       ("iters", b.n_loci))})
    q.step(observe=observe)
    q.step(observe=observe)
    q.finish()
    torch.cuda.synchronize()
    assert len(snaps) == 2
    for snap in snaps:
        for name, t in snap.items():
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(want[name]).tobytes(), name


def test_block_scatter_bias_entry(ctx, oracle):
    """The bias arrays set: the tile is loaded as F_ij 2^(row_bias_i iso_bias_j), the isoform's factor looked up by the column a
    slot holds.  Factors in {-1, 0, 1}: exact powers of two on the device and in numpy alike, so the oracle on the pre-multiplied
    weights is the reference for every locus, counts included."""
    import torch
    b = mixed_batch()
    rng = np.random.default_rng(6)
    row_bias = rng.integers(-1, 2, int(b.row_off[-1])).astype(np.float64)
    iso_bias = rng.integers(-1, 2, int(b.iso_off[-1])).astype(np.float64)
    Fb = b.F.copy()
    for l in range(b.n_loci):
        r0, r1, j0, j1 = b.row_off[l], b.row_off[l + 1], b.iso_off[l], b.iso_off[l + 1]
        Fb[b.f_off[l]:b.f_off[l + 1]] *= np.exp2(np.outer(row_bias[r0:r1], iso_bias[j0:j1])).reshape(-1)
    assert not np.array_equal(Fb, b.F)

    def setup(s):
        s.set_bias(torch.from_numpy(row_bias).to(s.dev), torch.from_numpy(iso_bias).to(s.dev))
    rows.solve_and_compare(ctx, oracle, b, F_oracle=Fb, solver_setup=setup)
